"""Every arm of the unfused embedding kernels (csrc/fx_embed.hip) and of fx_emb_grad_reduce[_scaled] on a real MI355X:
each row geometry of fx_row_geom, strided tables / id rows / records, the grid-stride loops behind the launch caps,
the edges of every argument guard.  Cases and references: tests/embed_cases.py.  Copies and single multiplies are
compared bit for bit; sums by rowopt_cases.within_yardstick against the fp64 reference, the yardstick being the fp32
left-to-right restatement of the same sum (never the kernel), the floor one fp32 rounding of the largest result."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import embed_cases as EC  # noqa: E402
from fuxictr_amd import _lib, layers, ops  # noqa: E402

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


def _dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def _flag(scal):
    return int(scal.view(torch.int32)[_lib.SC_ERR])


def _held(got, ref32, ref64, what, scale=None):
    e_nat, e_ref = EC.within_yardstick(got.detach().cpu(), ref32, ref64, EC.floor_of(ref64, scale), what)
    print("[embed arms] %s: |native - fp64| %.3g, fp32 yardstick %.3g" % (what, e_nat, e_ref))
    return e_nat, e_ref


# ---- gather ----------------------------------------------------------------------------------------------------------
def _run_gather(k):
    scal = ops.new_scalars(DEV)
    out = k.out.on(DEV)
    ids = k.ids.on(DEV)
    ops.emb_gather_fwd(k.table.on(DEV), k.D, ids if k.C else None, _dev(k.bases, torch.int64),
                       _dev(k.vocabs, torch.int32), _dev(k.col_off, torch.int64),
                       k.dense.on(DEV) if k.Fd else None, _dev(k.num_w) if k.Fd else None,
                       _dev(k.num_off, torch.int64) if k.Fd else None, out, scal,
                       n_cols=k.n_cols if k.C else None)
    torch.cuda.synchronize()
    ref, written, flag = EC.gather_ref(k)
    EC.same_bits(out, ref, ("gather", k.D, k.B, k.C, k.Fd))
    k.out.untouched("gather record D=%d" % k.D, written)
    assert _flag(scal) == flag
    return flag


@pytest.mark.parametrize("D", EC.ALL_D)
def test_gather_every_width_strided_with_edge_ids(D):
    """Table a column range of a wider block (table_ld > D), ids and dense column ranges (ids_ld > C), interleaved
    slots in a wider record; ids -1 and vocab zero their slot and raise the flag, vocab - 1 is a row."""
    assert _run_gather(EC.gather_case(D)) == EC.BAD_ID
    assert _run_gather(EC.gather_case(D, edge_ids=False, strided=False, seed=1)) == 0


@pytest.mark.parametrize("D", [16, 10, 65])
def test_gather_column_count_edges(D):
    assert _run_gather(EC.gather_case(D, C=0, Fd=2, edge_ids=False)) == 0          # no id column
    assert _run_gather(EC.gather_case(D, C=3, Fd=0, edge_ids=False)) == 0          # no numeric column
    assert _run_gather(EC.gather_case(D, C=5, Fd=1, n_cols=2, edge_ids=False)) == 0   # n_cols < ids.shape[1]
    k = EC.gather_case(D, C=2, Fd=0, edge_ids=False)                               # vocab - 1 alone: no flag
    k.ids.init[:, k.ids.cols][:, 0] = k.vocabs[0] - 1
    k.ids.block[:] = k.ids.init
    assert _run_gather(k) == 0


def test_gather_grid_stride_tail_items():
    c = EC.GATHER_STRIDE
    assert c["B"] * (c["C"] + c["Fd"]) > EC.limits().gather_blocks
    _run_gather(EC.gather_case(c["D"], B=c["B"], C=c["C"], Fd=c["Fd"], edge_ids=False))


def test_gather_rejections():
    def call(D, out_ld=None, table_ld=None):
        W = max(D, 1)
        table = torch.zeros(8 * W, device=DEV).as_strided((8, W), (W if table_ld is None else table_ld, 1))
        out = torch.zeros(4, W if out_ld is None else out_ld, device=DEV)
        ops.emb_gather_fwd(table, D, _dev(torch.zeros(4, 1), torch.int32), _dev([0], torch.int64),
                           _dev([8], torch.int32), _dev([0], torch.int64), None, None, None, out,
                           ops.new_scalars(DEV))
    for D in (0, 257):
        with pytest.raises(_lib.FxError, match=r"D=%d not in \[1,256\]" % D):
            call(D)
    with pytest.raises(_lib.FxError, match="out_ld=18 not a multiple of 4"):
        call(16, out_ld=18)
    with pytest.raises(_lib.FxError, match="out_ld=11 not a multiple of 2"):
        call(10, out_ld=11)
    with pytest.raises(_lib.FxError, match="table_ld=12 does not allow"):
        call(16, table_ld=12)
    call(16, out_ld=20)


# ---- pooled sequences ------------------------------------------------------------------------------------------------
def _run_pool(k):
    scal = ops.new_scalars(DEV)
    out = k.out.on(DEV)
    denom = torch.full((k.B, k.n_seq), -1.0, device=DEV)
    ops.emb_seq_pool_fwd(k.table.on(DEV), k.D, k.ids.on(DEV), _dev(k.col_base, torch.int64),
                         _dev(k.col_vocab, torch.int32), _dev(k.seq_col0, torch.int32), _dev(k.lens, torch.int32),
                         _dev(k.modes, torch.int32), _dev(k.out_off, torch.int64), out, denom, scal)
    torch.cuda.synchronize()
    r64, d64, flag = EC.pool_ref(k, F64)
    r32, d32, _ = EC.pool_ref(k, F32)
    EC.same_bits(denom, d64, ("pool denom", k.D))
    got = torch.stack([out[:, o:o + k.D] for o in k.out_off], 1)
    res = _held(got, r32, r64, "seq_pool D %d B %d lens %s" % (k.D, k.B, k.lens))
    written = torch.zeros(k.B, (k.n_seq + 1) * k.D, dtype=torch.bool)
    written[:, :k.n_seq * k.D] = True
    k.out.untouched("pool record D=%d" % k.D, written)
    assert _flag(scal) == flag
    return flag, res


@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("D", EC.POOL_D + [10, 13])
def test_seq_pool_every_position_group_count(D, bad):
    """P = 64 / lanes positions per wave and L of 1, P - 1, P, P + 1, 2P + 3 in one call, MEAN and SUM mixed; empty,
    full and mid-padded histories; a row summing to exactly 0 is not counted; strided table and id rows."""
    flag, _ = _run_pool(EC.pool_case(D, bad=bad))
    assert flag == (EC.BAD_ID if bad else 0)


def test_seq_pool_packed_operands_and_grid_stride():
    _run_pool(EC.pool_case(16, strided=False, seed=1))
    c = EC.POOL_STRIDE
    assert c["B"] * len(c["lens"]) > EC.limits().pool_blocks * EC.limits().pool_items
    _run_pool(EC.pool_case(c["D"], B=c["B"], lens=c["lens"]))


@pytest.mark.parametrize("D", EC.WIDE_D)
def test_seq_pool_refuses_rows_wider_than_a_wave(D):
    k = EC.pool_case(D, lens=[2])
    with pytest.raises(_lib.FxError, match=r"fx_emb_seq_pool_fwd: D=%d needs %d lanes per row \(max 64\)"
                       % (D, EC.geometry(D)[1])):
        _run_pool(k)


# ---- numeric gradient ------------------------------------------------------------------------------------------------
def _numgrad_direct(k, dout, dense, out, workspace):
    off = _dev(k.num_off, torch.int64)
    _lib.check(_lib.load().fx_emb_numeric_grad(_lib.ptr(dout), dout.stride(0), _lib.ptr(off),
                                               _lib.ptr(dense), dense.stride(0), k.Fd, k.D, k.B, _lib.ptr(out),
                                               _lib.ptr(workspace), _lib.stream_ptr(dout.device)),
               "fx_emb_numeric_grad")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", EC.NUMGRAD_B)
@pytest.mark.parametrize("D", EC.NUMGRAD_D)
def test_numeric_grad_both_arms(D, B):
    """The two-stage arm (ops: FX_NUMGRAD_CHUNKS row chunks, then their sum) and the one-launch arm (workspace NULL),
    strided dense, every second slot of a wider record; two calls, equal bits."""
    k = EC.numgrad_case(D, B)
    dout, dense = k.dout.on(DEV), k.dense.on(DEV)
    r64, r32 = EC.numgrad_ref(k, F64), EC.numgrad_ref(k, F32)
    outs = []
    for arm in ("workspace", "direct"):
        pair = []
        for _ in range(2):
            out = torch.full((k.Fd, D), float("nan"), device=DEV)
            if arm == "workspace":
                ops.emb_numeric_grad(dout, dout.stride(0), _dev(k.num_off, torch.int64), dense, D, out)
                torch.cuda.synchronize()
            else:
                _numgrad_direct(k, dout, dense, out, None)
            pair.append(out.cpu())
        EC.same_bits(pair[0], pair[1], ("numeric grad twice", arm, D, B))
        _held(pair[0], r32, r64, "numeric_grad %s D %d B %d" % (arm, D, B))
        outs.append(pair[0])
    k.dout.untouched("numeric grad dout")
    k.dense.untouched("numeric grad dense")


# ---- FM ----------------------------------------------------------------------------------------------------------------
def _run_fm(k, fwd=True):
    F, D, B = k.F, k.D, k.B
    emb = k.emb.on(DEV)
    e3 = k.emb.host().view(B, F, D)
    worst = []
    if fwd:
        for addend in (None, k.addend):
            out = torch.full((B, 1), float("nan"), device=DEV)
            ops.fm_fwd(emb, F, D, None if addend is None else _dev(addend), out)
            torch.cuda.synchronize()
            worst.append(_held(out[:, 0], EC.fm_ref(e3, addend, F32), EC.fm_ref(e3, addend, F64),
                               "fm_fwd F %d D %d B %d addend %s" % (F, D, B, addend is not None), EC.fm_scale(e3)))
    for acc in (False, True):
        base = k.demb0 if acc else None
        dv = EC.View(k.demb0 if acc else EC.filled(B, F * D), margin=2 * k.vec)
        demb = dv.on(DEV)
        ops.fm_bwd(emb, F, D, _dev(k.g), demb, accumulate=acc)
        torch.cuda.synchronize()
        worst.append(_held(demb.view(B, F, D), EC.fm_grad_ref(e3, k.g, base, F32), EC.fm_grad_ref(e3, k.g, base, F64),
                           "fm_bwd F %d D %d B %d accumulate %s" % (F, D, B, acc)))
        dv.untouched("fm demb F=%d D=%d" % (F, D))
    k.emb.untouched("fm emb")
    return worst


@pytest.mark.parametrize("F", EC.FM_F)
@pytest.mark.parametrize("D", EC.FM_D)
def test_fm_forward_backward_every_lane_count(D, F):
    """S = 16, 32, 64 lanes per sample, 1 ... 16 field-parallel lanes, B = 37 (no multiple of the samples per
    workgroup: the wave-uniform loop has invalid tail samples), emb_ld and demb_ld wider than F * D."""
    _run_fm(EC.fm_case(F, D))


def test_fm_grid_stride():
    c = EC.FM_STRIDE
    assert c["B"] > EC.limits().fm_blocks * (256 // EC.fm_lanes(c["D"]))
    _run_fm(EC.fm_case(c["F"], c["D"], B=c["B"]))


@pytest.mark.parametrize("D", EC.WIDE_D)
def test_fm_rows_wider_than_a_wave(D):
    """fx_fm_fwd reduces a sample with wave shuffles: rows of more than 64 lanes are refused by the C entry (before:
    out[b] was a multiple of the first wave's partial sum); fx_fm_bwd needs no such step and is held to fp64."""
    k = EC.fm_case(5, D)
    with pytest.raises(_lib.FxError, match=r"fx_fm_fwd: D=%d needs %d lanes per row \(max 64\)"
                       % (D, EC.geometry(D)[1])):
        ops.fm_fwd(k.emb.on(DEV), 5, D, None, torch.empty(k.B, 1, device=DEV))
    _run_fm(k, fwd=False)


@pytest.mark.parametrize("addend", [False, True])
@pytest.mark.parametrize("D", [65, 130, 64])
def test_fm_layer_function_matches_fp64_at_every_width(D, addend):
    """layers._FMFn, forward and gradient: the widths fx_fm_fwd refuses go through the torch expression (64: the
    kernels)."""
    k = EC.fm_case(5, D)
    e3 = k.emb.host().view(k.B, 5, D).contiguous()
    e = _dev(e3).requires_grad_(True)
    a = _dev(k.addend.view(-1, 1)).requires_grad_(True) if addend else None
    out = layers._FMFn.apply(e, a)
    assert out.shape == (k.B, 1)
    out.backward(_dev(k.g.view(-1, 1)))
    add = k.addend if addend else None
    _held(out[:, 0], EC.fm_ref(e3, add, F32), EC.fm_ref(e3, add, F64), "_FMFn forward D %d" % D, EC.fm_scale(e3))
    _held(e.grad, EC.fm_grad_ref(e3, k.g, None, F32), EC.fm_grad_ref(e3, k.g, None, F64), "_FMFn gradient D %d" % D)
    if addend:
        EC.same_bits(a.grad[:, 0], k.g, "_FMFn addend gradient")


# ---- LR ----------------------------------------------------------------------------------------------------------------
def _run_lr(k, bias):
    scal = ops.new_scalars(DEV)
    out = torch.full((k.B, 1), float("nan"), device=DEV)
    ops.lr_fwd(k.table1.on(DEV), k.ids.on(DEV) if k.C else None, _dev(k.bases, torch.int64),
               _dev(k.vocabs, torch.int32), k.dense.on(DEV) if k.Fd else None, _dev(k.w1) if k.Fd else None,
               _dev(k.bias) if bias else None, out, scal)
    torch.cuda.synchronize()
    r64, flag = EC.lr_ref(k, bias, F64)
    r32, _ = EC.lr_ref(k, bias, F32)
    _held(out[:, 0], r32, r64, "lr_fwd C %d Fd %d B %d bias %s" % (k.C, k.Fd, k.B, bias))
    assert _flag(scal) == flag
    return flag


@pytest.mark.parametrize("Fd", EC.LR_FD)
@pytest.mark.parametrize("C", EC.LR_C)
def test_lr_column_counts_around_the_sixteen_lanes(C, Fd):
    """table1_ld = 3 (a D = 1 column of a wider block), strided ids and dense, bias present and absent."""
    if C + Fd == 0:
        k = EC.lr_case(0, 0)
        assert _run_lr(k, True) == 0
        return
    assert _run_lr(EC.lr_case(C, Fd), True) == 0
    assert _run_lr(EC.lr_case(C, Fd, seed=1), False) == 0
    if C:
        assert _run_lr(EC.lr_case(C, Fd, bad=True), True) == EC.BAD_ID


def test_lr_grid_stride():
    c = EC.LR_STRIDE
    assert c["B"] > EC.limits().lr_blocks * EC.limits().lr_items
    _run_lr(EC.lr_case(c["C"], c["Fd"], B=c["B"]), True)


# ---- dot interaction ---------------------------------------------------------------------------------------------------
def _run_dot(k, keep=None):
    """-> (out, demb) host copies; keep: a dict the raw results go into (the cross-process comparison)."""
    F, D, B, tail = k.F, k.D, k.B, k.tail
    emb, out, demb, g = k.emb.on(DEV), k.out.on(DEV), k.demb.on(DEV), k.g.on(DEV)
    ops.dot_interact_fwd(emb, F, D, out, tail=tail)
    ops.dot_interact_bwd(emb, g, F, D, demb, tail=tail)
    torch.cuda.synchronize()
    e3 = k.emb.host().view(B, F, D)
    r64 = EC.dot_ref(e3, tail, F64)
    what = "F %d D %d B %d tail %d (%s)" % (F, D, B, tail, "MFMA" if EC.dot_mfma(F, D) else "plain")
    _held(out, EC.dot_ref(e3, tail, F32), r64, "dot_fwd " + what)
    if tail:
        EC.same_bits(out[:, k.P:], r64[:, k.P:].float(), "dot tail: the last field and zeros")
    _held(demb.view(B, F, D), EC.dot_grad_ref(e3, k.g.host(), tail, F32), EC.dot_grad_ref(e3, k.g.host(), tail, F64),
          "dot_bwd " + what)
    for v, name in ((k.emb, "emb"), (k.out, "out"), (k.demb, "demb"), (k.g, "g")):
        v.untouched("dot %s %s" % (name, what))
    return out.cpu().contiguous(), demb.cpu().contiguous()


def _tails(D):
    return [0, D, D + 3]


@pytest.mark.parametrize("F,D", EC.DOT_MFMA + EC.DOT_PLAIN)
def test_dot_interaction_both_arms_every_tail(F, D):
    """MFMA arm (F <= 32, even D <= 32; odd F: the K loop's padded row and column) and workgroup-per-sample arm (odd D,
    D = 34, F = 33, F * D = 4096), tail 0, D and D + 3, out_ld / emb_ld / g_ld / demb_ld wider than needed."""
    for tail in _tails(D):
        _run_dot(EC.dot_case(F, D, tail=tail))


def test_dot_interaction_grid_stride():
    lim = EC.limits()
    c = EC.DOT_MFMA_STRIDE
    assert c["B"] > lim.dot_mfma_blocks * lim.dot_mfma_items
    _run_dot(EC.dot_case(c["F"], c["D"], B=c["B"], tail=c["D"]))
    c = EC.DOT_PLAIN_STRIDE
    assert c["B"] > lim.dot_plain_blocks
    _run_dot(EC.dot_case(c["F"], c["D"], B=c["B"], tail=c["D"]))


def test_dot_interaction_mfma_shapes_on_the_plain_kernels():
    """fx_dot_mfma_ok reads FX_DOT_MFMA once per process: a fresh child with FX_DOT_MFMA=0 holds every MFMA-eligible
    shape of this file to the same fp64 references on the workgroup-per-sample kernels."""
    env = dict(os.environ, FX_DOT_MFMA="0")
    code = ("import sys; sys.path[:0] = %r\n"
            "import torch, embed_cases as EC, test_gpu_embed_arms as T\n"
            "for F, D in EC.DOT_MFMA:\n"
            "    for tail in T._tails(D):\n"
            "        T._run_dot(EC.dot_case(F, D, tail=tail))\n"
            "print('plain arm held')\n" % ([os.path.dirname(os.path.abspath(__file__)),
                                            os.path.dirname(os.path.dirname(os.path.abspath(__file__)))],))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "plain arm held" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_dot_interaction_rejections():
    def call(F, D, tail=0):
        P = F * (F - 1) // 2
        ops.dot_interact_fwd(torch.zeros(2, max(1, F * D), device=DEV), F, D,
                             torch.zeros(2, max(1, P + tail), device=DEV), tail=tail)
    with pytest.raises(_lib.FxError, match="F=1 D=4 outside the supported range"):
        call(1, 4)
    with pytest.raises(_lib.FxError, match="F=17 D=256 outside the supported range"):
        call(17, 256)
    with pytest.raises(_lib.FxError, match="tail must be 0 or >= D"):
        call(3, 4, tail=3)
    with pytest.raises(_lib.FxError, match="outside the supported range"):
        ops.dot_interact_bwd(torch.zeros(2, 4, device=DEV), torch.zeros(2, 1, device=DEV), 1, 4,
                             torch.zeros(2, 4, device=DEV))


# ---- gradient reduce ---------------------------------------------------------------------------------------------------
def _dd(k):
    dd = ops.DedupResult(k.n_max, k.C, DEV)
    dd.sorted_pos.copy_(k.sorted_pos)
    dd.seg_start.copy_(k.seg_start)
    dd.n_unique.fill_(k.nu)
    dd.uniq_row.copy_(torch.arange(k.n_max, dtype=torch.int32))
    return dd


def _run_reduce(k):
    dd = _dd(k)
    dout = k.dout.on(DEV)
    denom = k.denom.on(DEV)
    n_part = ops.emb_grad_reduce_partials(k.n_max, k.D)
    scr = torch.zeros(ops.emb_grad_reduce_scratch_ints(k.n_max), dtype=torch.int32, device=DEV)
    res = []
    for _ in range(2):
        Gv = EC.View(EC.filled(k.n_max, k.D), margin=0)
        G = Gv.on(DEV)
        assert G.is_contiguous()
        sq = torch.full((n_part,), float("nan"), device=DEV)
        ops.emb_grad_reduce(dout, dout.stride(0), _dev(k.col_off, torch.int64), k.C, k.D, dd, G, sq, scr,
                            _dev(k.col_denom, torch.int32) if k.scaled else None, denom if k.scaled else None)
        torch.cuda.synchronize()
        assert int(scr[0]) == 0                                 # the long-row counter is left reset
        written = torch.zeros(k.n_max, k.D, dtype=torch.bool)
        written[:k.nu] = True
        Gv.untouched("reduce G D=%d" % k.D, written)            # rows behind n_unique and the guard rows
        res.append((G[:k.nu].cpu(), sq.cpu()))
    EC.same_bits(res[0][0], res[1][0], ("reduce twice: G", k.D))
    EC.same_bits(res[0][1], res[1][1], ("reduce twice: sq_partials", k.D))
    r64, r32 = EC.reduce_ref(k, F64), EC.reduce_ref(k, F32)
    what = "grad_reduce D %d scaled %s rows %d longest run %d" % (k.D, k.scaled, k.nu, max(k.runs))
    e_nat, e_ref = _held(res[0][0], r32, r64, what)
    rpb = 256 // EC.geometry(k.D)[1]
    bound = EC.sqnorm_bound(r64, max(EC.floor_of(r64), 1.5 * e_ref), rpb * k.D)
    total = float(res[0][1].double().sum())
    assert abs(total - float((r64 ** 2).sum())) <= bound, (what, total, float((r64 ** 2).sum()), bound)
    k.dout.untouched("reduce dout")
    return e_nat, e_ref


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("D", EC.ALL_D)
def test_grad_reduce_every_width_run_length_and_padding(D, scaled):
    """Runs of 1, 31, 32, 33, 64 around FX_LONG_RUN and a hot row with four fifths of the lookups; padding lookups
    (sorted_pos = 0xFFFFFFFF) inside a chunk of 4, a remainder chunk and a chunk of 8; with and without the pooling
    denominators; G behind n_unique untouched; sq_partials sums to ||G||^2; two calls, equal bits."""
    _run_reduce(EC.reduce_standard(D, scaled))


def test_grad_reduce_more_long_rows_than_workgroups():
    c = EC.REDUCE_MANY_LONG
    assert c["n_rows"] > EC.limits().long_blocks
    _run_reduce(EC.reduce_case(c["D"], [c["run"]] * c["n_rows"], C=1))


def test_grad_reduce_padding_through_col_pad():
    """The de-dup's own padding (col_pad; column-sorted path: padding keeps its place with sorted_pos = 0xFFFFFFFF)
    feeding the reduce: == index_add_ of the lookups that are not padding."""
    D, B, vocabs, pads = 10, 300, [3, 40], [0, 1]
    g = EC.rng(8)
    ids = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocabs], 1).int()
    bases = [0, vocabs[0]]
    ws = torch.empty(ops.dedup_workspace_bytes(B * 2), dtype=torch.uint8, device=DEV)
    dout = torch.randn(B, 2 * D, generator=g)
    refs = []
    for dt in (F32, F64):
        ref = torch.zeros(sum(vocabs), D, dtype=dt)
        for c in range(2):
            live = ids[:, c] != pads[c]
            ref.index_add_(0, ids[live, c].long() + bases[c], dout[live, c * D:(c + 1) * D].to(dt))
        refs.append(ref)
    for columns_sorted in (True, False):
        dd = ops.dedup(_dev(ids), _dev(bases, torch.int64), _dev(vocabs, torch.int32), _dev(pads, torch.int32),
                       sum(vocabs), ws, columns_sorted=columns_sorted)
        G = torch.zeros(dd.n_max, D, device=DEV)
        sq = torch.empty(ops.emb_grad_reduce_partials(dd.n_max, D), device=DEV)
        scr = torch.zeros(ops.emb_grad_reduce_scratch_ints(dd.n_max), dtype=torch.int32, device=DEV)
        ops.emb_grad_reduce(_dev(dout), 2 * D, _dev([0, D], torch.int64), 2, D, dd, G, sq, scr)
        nu = int(dd.n_unique.item())
        rows = dd.uniq_row[:nu].cpu().long()
        _held(G[:nu], refs[0][rows], refs[1][rows], "grad_reduce after dedup columns_sorted %s" % columns_sorted)
        untouched = torch.ones(sum(vocabs), dtype=torch.bool)
        untouched[rows] = False
        assert not refs[1][untouched].any() and int(scr[0]) == 0


def test_grad_reduce_of_no_lookups():
    """n_max = 0: the one partial is zeroed, nothing else is read."""
    sq = torch.full((1,), float("nan"), device=DEV)
    scr = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert ops.emb_grad_reduce_partials(0, 16) == 1 and ops.emb_grad_reduce_scratch_ints(0) == 2
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    _lib.check(lib.fx_emb_grad_reduce(null, 0, null, 1, 16, null, null, null, 0, null, _lib.ptr(sq), _lib.ptr(scr),
                                      _lib.stream_ptr(sq.device)), "fx_emb_grad_reduce")
    torch.cuda.synchronize()
    assert float(sq[0]) == 0.0 and int(scr[0]) == 0
