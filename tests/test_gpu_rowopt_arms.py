"""Every arm of the sparse row optimizer (csrc/fx_rowopt.hip) and the bf16 arm of the gather (fx_emb_fm_fwd) on a real
MI355X: each row geometry of fx_row_geom (vec 4 / 2 / 1, 1 ... 256 lanes, lane groups with an idle lane), fp32 and
bf16 tables, packed arrays and the row record, 1 ... 6 table groups per call, the clip and the regularizer inside the
update.  Cases, references and acceptance rules: tests/rowopt_cases.py (37 rows between guard rows; dense torch Adam /
SGD in fp32 and fp64; the fp64 yardstick, 1e-6 on the moments, bit equality — nothing new)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rowopt_cases as RC  # noqa: E402
from fuxictr_amd import _lib, ops  # noqa: E402
from rowopt_cases import DS, IDS, LR, R, ROWS, T0  # noqa: E402

DEV = "cuda:0"
UPTO = T0 + 5                       # the catch-ups bring rows from step T0 (never-touched rows: 0) to this step
L1, L2 = 3e-3, 2e-2
FORMS = ["fp32-packed", "fp32-record", "bf16-packed"]
ALL_ROWS = list(range(R))


def _dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def test_the_width_list_reaches_every_geometry():
    geo = [RC.geometry(D) for D in DS]
    assert {v for v, _ in geo} == {1, 2, 4} and {l for _, l in geo} == {1, 4, 16, 64, 128, 256}
    assert all(RC.idle_lane(D) for D in (6, 12, 40, 130))


@functools.lru_cache(maxsize=None)
def _dd():
    """The de-dup result every launch of this file takes: 40 lookups, 25 unique rows (rows 0 and R - 1 among them; not
    a multiple of any lane group's rows per workgroup), n_max = 40 > n_unique; the stale tail of uniq_row names the
    guard row behind the table, so a launch that reads it as rows fails guards_intact."""
    ids = np.asarray(IDS).reshape(-1, 1)
    ws = torch.empty(ops.dedup_workspace_bytes(len(IDS)), dtype=torch.uint8, device=DEV)
    dd = ops.dedup(_dev(ids, torch.int32), _dev([0], torch.int64), _dev([R], torch.int32), _dev([-1], torch.int32),
                   R, ws)
    nu = int(dd.n_unique.item())
    assert nu == len(ROWS) and dd.uniq_row[:nu].cpu().tolist() == ROWS and dd.n_max == len(IDS) > nu
    assert all(nu % (256 // lanes) != 0 for _, lanes in map(RC.geometry, DS) if lanes < 256)
    dd.uniq_row[nu:] = R
    return dd


def _grad(D, seed=0):
    g = torch.Generator().manual_seed(77 * D + seed)
    G = torch.zeros(len(IDS), D)
    G[:len(ROWS)] = torch.randn(len(ROWS), D, generator=g) * 0.1
    return G


def _update_scal(Gs, reg):
    """The scalars of step T0 + 1 with a clip coefficient of about 0.4 (and the regularizer weights)."""
    total = float(torch.sqrt(sum((G.double() ** 2).sum() for G in Gs)))
    scal = ops.new_scalars(DEV, lr=LR, max_norm=0.4 * total)
    scal.view(torch.int32)[_lib.SC_STEP] = T0
    ops.opt_begin_step(scal)
    ops.clip_coef([_dev([total * total], torch.float32)], scal)
    if reg:
        scal[_lib.SC_REG_L1:_lib.SC_REG_L1 + 1].fill_(L1)
        scal[_lib.SC_REG_L2:_lib.SC_REG_L2 + 1].fill_(L2)
    clip = float(scal[_lib.SC_CLIP])
    assert 0.39 < clip < 0.41
    return scal, clip


def _catchup_scal():
    scal = ops.new_scalars(DEV, lr=LR)
    scal.view(torch.int32)[_lib.SC_STEP] = UPTO
    return scal


def _listed(fields, rows):
    return tuple(None if x is None else x[rows] for x in fields)


def _state(D, form, seed=0, adam=True, widened=False):
    dtype, layout = form.split("-")
    return RC.make_state(D, R, dtype, layout, seed, device=DEV, adam=adam,
                         representable=True if widened else None)


# ---- a. one table, every geometry ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed_update(D, kind, reg, widened):
    """The fp32 packed run of an update case, held to the references; -> (fields after the launch, error / yardstick).
    widened: the table holds bf16 values (the fp32 twin of the bf16 case)."""
    p, m, v, last, st = _state(D, "fp32-packed", adam=kind == "adam", widened=widened)
    G = _grad(D)
    scal, clip = _update_scal([G], reg)
    st.G = _dev(G)
    ops.sparse_update_multi(kind, [st], _dd(), scal)
    torch.cuda.synchronize()
    RC.guards_intact(st)
    l1, l2 = (L1, L2) if reg else (0.0, 0.0)
    refs = [RC.ref_update(kind, p[ROWS], m[ROWS], v[ROWS], G[:len(ROWS)], T0 + 1, LR, clip, l1, l2, f64)
            for f64 in (False, True)]
    got = st.fields()
    ratio = RC.check_fp32(_listed(got, ROWS), refs[0], refs[1], T0 + 1, ("update", D, kind, reg, widened))
    return got, ratio


@pytest.mark.parametrize("kind,reg", [("adam", True), ("sgd", True), ("adam", False)])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("D", DS)
def test_update_of_one_table(D, form, kind, reg):
    """fx_sparse_adam_multi / fx_sparse_sgd_multi on one table with clip_coef ~ 0.4 and the L1 + L2 regularizer (reg
    False: both weights zero, the early return of fx_add_reg): the packed fp32 table against dense torch steps in fp32
    and fp64; the record bit-identical to packed; the bf16 table the fp32 result on the widened table rounded once."""
    base, ratio = _packed_update(D, kind, reg, form == "bf16-packed")
    if form != "fp32-packed":
        _, _, _, _, st = _state(D, form, adam=kind == "adam")
        scal, _ = _update_scal([_grad(D)], reg)
        st.G = _dev(_grad(D))
        ops.sparse_update_multi(kind, [st], _dd(), scal)
        torch.cuda.synchronize()
        RC.guards_intact(st)
        if form == "fp32-record":
            RC.check_same_bits(st.fields(), base, ("record == packed", D, kind))
        else:
            RC.check_bf16(st.fields(), base, ("bf16 == rounded fp32", D, kind))
    print("[rowopt arms] update %s D %d %s reg %s: |native - fp64| / yardstick %.2f" % (kind, D, form, reg, ratio))


@functools.lru_cache(maxsize=None)
def _catchup_refs(D, widened, seed=0):
    p, m, v, last = RC.host_case(D, seed, widened)
    return [RC.ref_catchup(p, m, v, last, UPTO, LR, f64) for f64 in (False, True)]


def _send_width(D):
    return -(-D // 4) * 4 + 4


def _catchup(st, way):
    """One catch-up of a single state up to UPTO: -> the rows it may write and, for the owner fetch, the send block."""
    scal, dd = _catchup_scal(), _dd()
    if way == "rows":
        ops.adam_catchup_rows([st], dd, 0, scal)
    elif way == "flush":
        ops.adam_catchup_all(st, R, 0, scal)
    else:
        send = torch.full((len(IDS), _send_width(st.D)), 7.0, device=DEV)
        zero_row = torch.full((_send_width(st.D),), 3.0, device=DEV)
        ops.owner_fetch_rows([st], [0], dd, send, True, scal, upto_offset=0, zero_row=zero_row)
        torch.cuda.synchronize()
        assert float(zero_row.abs().max()) == 0.0
        return ROWS, send.cpu()
    torch.cuda.synchronize()
    return (ROWS if way == "rows" else ALL_ROWS), None


@functools.lru_cache(maxsize=None)
def _packed_catchup(D, way, widened):
    _, _, _, _, st = _state(D, "fp32-packed", widened=widened)
    rows, send = _catchup(st, way)
    RC.guards_intact(st, rows)
    got = st.fields()
    refs = _catchup_refs(D, widened)
    ratio = RC.check_fp32(_listed(got, rows), _listed(refs[0], rows), _listed(refs[1], rows), UPTO,
                          ("catch-up", D, way, widened))
    return got, send, ratio


@pytest.mark.parametrize("way", ["rows", "flush", "fetch"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("D", DS)
def test_catchup_of_one_table(D, form, way):
    """fx_adam_catchup_rows, fx_adam_catchup_all (the flush) and fx_owner_fetch_rows with catchup on one table, 5 steps
    behind (never-touched rows: 8): the packed fp32 table against dense zero-gradient torch Adam in fp32 and fp64, the
    record bit-identical to packed, the bf16 table the rounded fp32 result.  The owner fetch leaves the state
    fx_adam_catchup_rows leaves and sends the rows as plain indexing of that table reads them, bit for bit."""
    widened = form == "bf16-packed"
    base, base_send, ratio = _packed_catchup(D, way, widened)
    got, send = base, base_send
    if form != "fp32-packed":
        _, _, _, _, st = _state(D, form)
        rows, send = _catchup(st, way)
        RC.guards_intact(st, rows)
        got = st.fields()
        if form == "fp32-record":
            RC.check_same_bits(got, base, ("record == packed", D, way))
        else:
            RC.check_bf16(got, base, ("bf16 == rounded fp32", D, way))
    if way == "fetch":
        _, _, _, _, twin = _state(D, form)
        _catchup(twin, "rows")
        RC.check_same_bits(got, twin.fields(), ("owner fetch leaves the state of adam_catchup_rows", D, form))
        ref = torch.zeros(len(IDS), _send_width(D))
        ref[:, :D] = twin.table.cpu().float()[IDS]
        RC.check_same_bits((send,), (ref,), ("send block", D, form))
    print("[rowopt arms] catch-up %s D %d %s: |native - fp64| / yardstick %.2f" % (way, D, form, ratio))


# ---- b. several tables in one launch -------------------------------------------------------------------------
LISTS = [(12, 1), (40, 5), (16, 1), (1, 16), (130, 16, 1, 6), (255, 2, 12, 1)]
LAYOUTS = ["packed", "record", "bf16first"]


def _forms(dims, layout, widened=False):
    """The form of each table of a list; bf16first: the first table bf16 (or, widened, its fp32 twin)."""
    forms = ["fp32-record" if layout == "record" else "fp32-packed"] * len(dims)
    if layout == "bf16first" and not widened:
        forms[0] = "bf16-packed"
    return forms


def _multi_states(dims, layout, adam=True, widened=False):
    return [_state(D, form, seed=i, adam=adam, widened=widened and i == 0)[4]
            for i, (D, form) in enumerate(zip(dims, _forms(dims, layout, widened)))]


@functools.lru_cache(maxsize=None)
def _update_one_by_one(dims, kind, widened):
    """One launch per packed fp32 table under the scalars of the whole list."""
    Gs = [_grad(D, i) for i, D in enumerate(dims)]
    scal, _ = _update_scal(Gs, True)
    out = []
    for st, G in zip(_multi_states(dims, "bf16first" if widened else "packed", kind == "adam", widened), Gs):
        st.G = _dev(G)
        ops.sparse_update_multi(kind, [st], _dd(), scal)
        torch.cuda.synchronize()
        RC.guards_intact(st)
        out.append(st.fields())
    return out


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", LISTS)
def test_update_of_several_tables_equals_one_launch_per_table(dims, layout, kind):
    """One fx_sparse_*_multi launch over a list — the (vec 4, vec 1) pair fast path at (12, 1), (40, 5), (16, 1); the
    same two widths the other way round; a 128- and a 256-lane group with narrow siblings — equals one launch per
    table bit for bit, as records too; with a bf16 first table it is the rounded result of the widened list."""
    Gs = [_grad(D, i) for i, D in enumerate(dims)]
    scal, _ = _update_scal(Gs, True)
    sts = _multi_states(dims, layout, kind == "adam")
    for st, G in zip(sts, Gs):
        st.G = _dev(G)
    ops.sparse_update_multi(kind, sts, _dd(), scal)
    torch.cuda.synchronize()
    ref = _update_one_by_one(dims, kind, layout == "bf16first")
    for i, (st, one) in enumerate(zip(sts, ref)):
        RC.guards_intact(st)
        if st.table.dtype == torch.bfloat16:
            RC.check_bf16(st.fields(), one, ("bf16 table of a list", dims, i))
        else:
            RC.check_same_bits(st.fields(), one, ("list == one launch per table", dims, layout, i))


@functools.lru_cache(maxsize=None)
def _catchup_one_by_one(dims, widened):
    """The plain replay of every table of a list, one launch per packed fp32 table: fx_adam_catchup_rows, which for one
    table is fx_catchup_row on each listed row.  A D = 16 table alone would take the quad replay there; its plain
    replay is RC.flush_listed.  With the stamps put back, guards_intact holds every unlisted row, all fields, to its
    first bits."""
    out = []
    for st in _multi_states(dims, "bf16first" if widened else "packed", True, widened):
        if st.D == 16:
            RC.flush_listed(st, ROWS, R, UPTO, 0, _catchup_scal())
        else:
            ops.adam_catchup_rows([st], _dd(), 0, _catchup_scal())
        torch.cuda.synchronize()
        RC.guards_intact(st)
        out.append(st.fields())
    return out


@pytest.mark.parametrize("D", [12, 16])
def test_flush_of_the_listed_rows_is_the_plain_replay(D):
    """RC.flush_listed, the twin _catchup_one_by_one builds for D = 16.  At D = 12, where fx_adam_catchup_rows has no
    quad replay, it is that launch bit for bit, unlisted rows included.  At D = 16 this test only holds it to the
    references of the listed rows, which the quad replay meets too: that it is the plain replay there rests on the
    code (k_catchup_all and the non-quad arm of k_catchup_rows call the same fx_catchup_row with the same sc, upto,
    lg, ser) and on the lists (1, 16) and (130, 16, 1, 6) below, whose D = 16 table leaves k_catchup_rows by the
    non-quad arm and equals this twin to the bit."""
    _, _, _, _, twin = _state(D, "fp32-packed")
    RC.flush_listed(twin, ROWS, R, UPTO, 0, _catchup_scal())
    torch.cuda.synchronize()
    RC.guards_intact(twin)
    if D == 12:
        _, _, _, _, st = _state(D, "fp32-packed")
        ops.adam_catchup_rows([st], _dd(), 0, _catchup_scal())
        torch.cuda.synchronize()
        RC.check_same_bits(twin.fields(), st.fields(), ("flush of the listed rows == fx_adam_catchup_rows", D))
    refs = _catchup_refs(D, False)
    RC.check_fp32(_listed(twin.fields(), ROWS), _listed(refs[0], ROWS), _listed(refs[1], ROWS), UPTO,
                  ("flush of the listed rows", D))


def _check_catchup_list(dims, layout, sts, plain, quad_from):
    """Tables before `quad_from` bit-identical to their plain replays; the ones from there on left through the quad
    replay, which the project documents as equal to rounding: the fp64 yardstick."""
    worst = 0.0
    for i, (st, one) in enumerate(zip(sts, plain)):
        RC.guards_intact(st)
        got = st.fields()
        if i >= quad_from:
            assert st.table.dtype == torch.float32      # (a bf16 quad pair is held to the rounded fp32 launch)
            refs = _catchup_refs(dims[i], False, i)
            worst = max(worst, RC.check_fp32(_listed(got, ROWS), _listed(refs[0], ROWS), _listed(refs[1], ROWS),
                                             UPTO, ("quad replay", dims, layout, i)))
        elif st.table.dtype == torch.bfloat16:
            RC.check_bf16(got, one, ("bf16 table of a list", dims, i))
        else:
            RC.check_same_bits(got, one, ("list == the plain replay of each table", dims, layout, i))
    return worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", LISTS)
def test_catchup_of_several_tables_equals_the_plain_replays(dims, layout):
    """One fx_adam_catchup_rows launch over the same lists.  (12, 1) and (1, 16) share the quad's lane group and must
    NOT take the quad replay: bit-identical to the plain replays, like every other list.  (16, 1) is the quad pair: the
    fp64 yardstick; with a bf16 first table, the rounded result of the same launch on the widened table."""
    sts = _multi_states(dims, layout)
    ops.adam_catchup_rows(sts, _dd(), 0, _catchup_scal())
    torch.cuda.synchronize()
    quad = dims == (16, 1)
    if quad and layout == "bf16first":
        twin = _multi_states(dims, layout, True, widened=True)
        ops.adam_catchup_rows(twin, _dd(), 0, _catchup_scal())
        torch.cuda.synchronize()
        RC.check_bf16(sts[0].fields(), twin[0].fields(), ("bf16 quad pair == rounded fp32 quad pair", dims))
        RC.check_same_bits(sts[1].fields(), twin[1].fields(), ("the D = 1 table of the pair", dims))
        for st in sts + twin:
            RC.guards_intact(st)
        sts, layout = twin, "packed-widened"
        worst = 0.0
        for i, st in enumerate(sts):
            refs = _catchup_refs(dims[i], i == 0, i)
            worst = max(worst, RC.check_fp32(_listed(st.fields(), ROWS), _listed(refs[0], ROWS),
                                             _listed(refs[1], ROWS), UPTO, ("quad replay", dims, layout, i)))
    else:
        plain = [None] * len(dims) if quad else _catchup_one_by_one(dims, layout == "bf16first")
        worst = _check_catchup_list(dims, layout, sts, plain, 0 if quad else len(dims))
    if quad:
        print("[rowopt arms] quad pair %s %s: |native - fp64| / yardstick %.2f" % (dims, layout, worst))


@pytest.mark.parametrize("layout", ["packed", "record"])
def test_catchup_of_six_tables_is_two_launches(layout):
    """ops.adam_catchup_rows splits a list longer than FX_MAX_TABLES: (40, 6, 3, 130) in one launch — bit-identical
    to the plain replays — and (16, 1) in a second, which is the quad pair (fp64 yardstick)."""
    dims = (40, 6, 3, 130, 16, 1)
    assert len(dims) > _lib.FX_MAX_TABLES
    sts = _multi_states(dims, layout)
    ops.adam_catchup_rows(sts, _dd(), 0, _catchup_scal())
    torch.cuda.synchronize()
    worst = _check_catchup_list(dims, layout, sts, _catchup_one_by_one(dims, False), _lib.FX_MAX_TABLES)
    print("[rowopt arms] six tables %s, quad pair in the second launch: |native - fp64| / yardstick %.2f"
          % (layout, worst))


# ---- c. argument guard ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["table", "m"])
@pytest.mark.parametrize("D", [16, 6])
def test_a_misaligned_field_is_refused_before_any_launch(D, field):
    """A [:, 1:1 + D] view of a wider block starts 4 bytes into a row: the float4 (D = 16) / float2 (D = 6) accesses of
    the kernels would be misaligned.  Every row-state entry point refuses it with the table and the field in the
    message, and launches nothing."""
    _, _, _, _, st = _state(D, "fp32-packed")
    wide = torch.zeros(R, D + 4, device=DEV)
    view = wide[:, 1:1 + D]
    view.copy_(getattr(st, field))
    setattr(st, field, view)
    st.G = _dev(_grad(D))
    before = [x.clone() for x in (wide, st.table, st.m, st.v, st.last_step)]
    scal, _ = _update_scal([_grad(D)], True)
    send = torch.full((len(IDS), _send_width(D)), 7.0, device=DEV)
    calls = [lambda: ops.sparse_update_multi("adam", [st], _dd(), scal),
             lambda: ops.adam_catchup_rows([st], _dd(), 0, _catchup_scal()),
             lambda: ops.adam_catchup_all(st, R, 0, _catchup_scal()),
             lambda: ops.owner_fetch_rows([st], [0], _dd(), send, True, _catchup_scal(), upto_offset=0)]
    for call in calls:
        with pytest.raises(_lib.FxError, match=r"table 0 field %s \(D=%d\) is not aligned" % (field, D)):
            call()
    torch.cuda.synchronize()
    for was, now in zip(before, (wide, st.table, st.m, st.v, st.last_step)):
        assert torch.equal(was, now)
    assert float(send.min()) == 7.0 and float(send.max()) == 7.0


# ---- d. the gather's bf16 arm --------------------------------------------------------------------------------
@pytest.mark.parametrize("fwd2", ["1", "0"])
@pytest.mark.parametrize("D", DS)
def test_bf16_gather_equals_fp32_gather_of_the_widened_table_at_every_width(D, fwd2):
    """fx_emb_fm_fwd reading a bf16 table: the record, S, fm_out and lr_out carry the bits of the fp32 call on the
    widened table, by k_emb_fm_fwd2 and by k_emb_fm_fwd (FX_EMB_FWD2=0); widths of more than 64 lanes are refused."""
    rng = np.random.default_rng(D)
    g = torch.Generator().manual_seed(D)
    B, vocabs, Fd = 70, [5, 3, 41], 1
    bases = np.concatenate([[0], np.cumsum(vocabs)[:-1]]).astype(np.int64)
    rows, C = int(sum(vocabs)), len(vocabs)
    table16 = torch.randn(rows, D, generator=g).bfloat16()
    num_w, num_w1 = torch.randn(Fd, D, generator=g), torch.randn(Fd, 1, generator=g)
    table1 = torch.randn(rows, 1, generator=g)
    ids = np.stack([rng.integers(0, v, B) for v in vocabs], axis=1)
    dense = torch.rand(B, Fd, generator=g)
    F = C + Fd
    off_c = _dev([(Fd + c) * D for c in range(C)], torch.int64)
    off_n = _dev([j * D for j in range(Fd)], torch.int64)
    outs = []
    os.environ["FX_EMB_FWD2"] = fwd2
    try:
        for tab in (table16.to(DEV), table16.float().to(DEV)):
            scal = ops.new_scalars(DEV)
            rec = torch.full((B, F * D), 5.0, device=DEV)
            lr, fm, S = torch.empty(B, 1, device=DEV), torch.empty(B, 1, device=DEV), torch.empty(B, D, device=DEV)

            def call():
                ops.emb_fm_fwd(tab, D, _dev(ids, torch.int32), _dev(bases, torch.int64), _dev(vocabs, torch.int32),
                               off_c, _dev(dense), _dev(num_w), off_n, rec, scal, table1=_dev(table1),
                               num_w1=_dev(num_w1), lr_out=lr, fm_out=fm, S=S)
            if RC.geometry(D)[1] > 64:
                with pytest.raises(_lib.FxError, match=r"D=%d needs %d lanes per row \(max 64\)"
                                   % (D, RC.geometry(D)[1])):
                    call()
                torch.cuda.synchronize()
                assert float(rec.min()) == 5.0 and float(rec.max()) == 5.0
                continue
            call()
            torch.cuda.synchronize()
            assert int(scal.view(torch.int32)[_lib.SC_ERR]) == 0
            outs.append((rec.cpu(), lr.cpu(), fm.cpu(), S.cpu()))
    finally:
        os.environ.pop("FX_EMB_FWD2")
    if outs:
        RC.check_same_bits(outs[0], outs[1], ("bf16 gather == fp32 gather of the widened table", D, fwd2))
        ref = torch.zeros(B, F, D)
        for c in range(C):
            ref[:, Fd + c] = table16.float()[torch.from_numpy(ids[:, c] + bases[c])]
        assert torch.equal(outs[0][0].view(B, F, D)[:, Fd:], ref[:, Fd:])
