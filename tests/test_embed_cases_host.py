"""tests/embed_cases.py without a GPU: each fp64 reference against an independent statement of the same operation
(torch autograd of F.embedding and oracle.ctr_oracle's pooling / FM / dot interaction, index_add_), the fp32
yardstick's left-to-right order, and the conditions the case lists of tests/test_gpu_embed_arms.py claim: every
(vec, lanes) class, every grid-stride case above its launch cap, every run-length bucket."""
import pytest
import torch
import torch.nn.functional as Fn

import embed_cases as EC
from fuxictr_amd import _lib
from oracle import ctr_oracle as O

F64 = torch.float64


def test_the_width_list_reaches_every_vec_and_lane_class():
    geo = {D: EC.geometry(D) for D in EC.ALL_D}
    for vec, ds in EC.WIDTHS.items():
        assert all(geo[D][0] == vec for D in ds)
    assert {geo[D] for D in EC.WIDTHS[4]} >= {(4, 1), (4, 4), (4, 16), (4, 64)}
    assert {geo[D] for D in EC.WIDTHS[2]} >= {(2, 1), (2, 8), (2, 64), (2, 128)}
    assert {geo[D] for D in EC.WIDTHS[1]} >= {(1, 1), (1, 4), (1, 16), (1, 64), (1, 128), (1, 256)}
    assert EC.WIDE_D == [65, 130, 255] and all(EC.geometry(D)[1] == _lib.row_lanes(D) for D in range(1, 257))
    assert {EC.fm_lanes(D) for D in EC.FM_D} == {16, 32, 64}
    assert {v for v, _ in map(EC.geometry, EC.FM_D)} == {1, 2, 4}
    assert [EC.pool_positions(D) for D in EC.POOL_D] == [64, 16, 4, 1, 1]
    assert EC.pool_lens(1) == [1, 63, 64, 65, 131] and EC.pool_lens(256) == [1, 2, 5]


def test_every_grid_stride_case_exceeds_its_launch_cap():
    lim = EC.limits()
    assert lim.numgrad_chunks == _lib.FX_NUMGRAD_CHUNKS == 16 and lim.long_run == 32 and lim.dot_max_fd == 4096
    c = EC.GATHER_STRIDE
    per = 256 // EC.geometry(c["D"])[1]
    assert per == 1 and lim.gather_blocks * per < c["B"] * (c["C"] + c["Fd"]) < 2 * lim.gather_blocks * per
    c = EC.POOL_STRIDE
    assert lim.pool_blocks * lim.pool_items < c["B"] * len(c["lens"]) < 2 * lim.pool_blocks * lim.pool_items
    c = EC.FM_STRIDE
    per = 256 // EC.fm_lanes(c["D"])
    assert lim.fm_blocks * per < c["B"] < 2 * lim.fm_blocks * per and c["B"] % per != 0
    assert lim.lr_blocks * lim.lr_items < EC.LR_STRIDE["B"] < 2 * lim.lr_blocks * lim.lr_items
    c = EC.DOT_MFMA_STRIDE
    assert EC.dot_mfma(c["F"], c["D"]) and lim.dot_mfma_blocks * lim.dot_mfma_items < c["B"]
    c = EC.DOT_PLAIN_STRIDE
    assert not EC.dot_mfma(c["F"], c["D"]) and lim.dot_plain_blocks < c["B"]
    c = EC.REDUCE_MANY_LONG
    assert c["n_rows"] > lim.long_blocks and c["run"] > lim.long_run
    assert all(37 % (256 // EC.fm_lanes(D)) != 0 for D in EC.FM_D)     # invalid tail samples at the default B
    assert all(EC.dot_mfma(F, D) for F, D in EC.DOT_MFMA) and not any(EC.dot_mfma(F, D) for F, D in EC.DOT_PLAIN)
    assert any(F * D == lim.dot_max_fd for F, D in EC.DOT_PLAIN) and any(F % 2 for F, _ in EC.DOT_MFMA)
    assert {2, 3, 31, 32} <= {F for F, _ in EC.DOT_MFMA} and {2, 16, 30, 32} <= {D for _, D in EC.DOT_MFMA}
    assert {1, 15, 16, 17} <= set(EC.NUMGRAD_B) and max(EC.NUMGRAD_B) == 1000


@pytest.mark.parametrize("D", [2, 16, 255])
def test_the_reduce_case_fills_every_run_length_bucket_and_places_its_padding(D):
    lim = EC.limits()
    k = EC.reduce_standard(D)
    rpb = 256 // EC.geometry(D)[1]
    for L in (1, lim.long_run - 1, lim.long_run, lim.long_run + 1, 2 * lim.long_run):
        assert k.runs.count(L) >= 1, L
    assert k.runs[-1] >= 8 * rpb + 1 and k.runs[-1] > 0.5 * k.n            # the hot row
    seg = k.seg_start[:k.nu + 1].long()
    assert int(seg[-1]) == k.n <= k.n_max and k.seg_start.shape == (k.n_max + 1,)
    sp = k.sorted_pos[:k.n].long() & 0xFFFFFFFF
    dead = (sp == EC.NO_POS).nonzero().view(-1).tolist()
    assert len(dead) == 4 and not k.live[dead].any()
    where = [(int(k.row_of[i]), i - int(seg[k.row_of[i]])) for i in dead]
    # a short run's first chunk of 4, a short run's remainder, and lane group 0's first chunk of 8 of the hot row
    assert where[0] == (1, 1) and k.runs[1] >= 4 and k.runs[1] <= lim.long_run
    assert where[1][0] == 4 and k.runs[4] > lim.long_run                    # a long row without a chunk of 8
    assert where[2][0] == 8 and k.runs[8] <= lim.long_run and k.runs[8] > where[2][1] >= 4 * (k.runs[8] // 4)
    assert where[3] == (k.nu - 1, 3 * rpb) and k.runs[-1] >= 8 * rpb
    for u in range(k.nu):                                       # ascending positions inside a run, all distinct
        run = k.pos[seg[u]:seg[u + 1]]
        assert bool((run[1:] > run[:-1]).all())
    assert k.pos.unique().numel() == k.n
    many = EC.reduce_case(2, [EC.REDUCE_MANY_LONG["run"]] * EC.REDUCE_MANY_LONG["n_rows"], C=1)
    assert sum(r > lim.long_run for r in many.runs) > lim.long_blocks


def test_seq_sum_is_the_left_to_right_fp32_sum():
    x = torch.randn(7, 300, 5, generator=EC.rng(0)) * 1e3
    acc = torch.zeros(7, 5)
    for b in range(7):
        for d in range(5):
            for i in range(300):
                acc[b, d] = acc[b, d] + x[b, i, d]
    assert torch.equal(EC.seq_sum(x, 1), acc) and EC.seq_sum(x, 1).dtype == torch.float32
    assert not torch.equal(acc.double(), EC.seq_sum(x.double(), 1))
    assert EC.seq_sum(torch.zeros(3, 0, 2), 1).shape == (3, 2)


@pytest.mark.parametrize("D", [1, 10, 65])
def test_gather_reference_is_embedding_lookup_and_numeric_expansion(D):
    k = EC.gather_case(D, edge_ids=False)
    out, written, flag = EC.gather_ref(k)
    assert flag == 0
    ids, table = k.ids.host().long(), k.table.host()
    for c in range(k.C):
        want = Fn.embedding(ids[:, c] + k.bases[c], table)
        assert torch.equal(out[:, k.col_off[c]:k.col_off[c] + D], want)
    for j in range(k.Fd):                                       # feature_embedding.py:280-282: x.view(-1, 1) @ W^T
        want = k.dense.host()[:, j].view(-1, 1) @ k.num_w[j].view(1, D)
        assert torch.equal(out[:, k.num_off[j]:k.num_off[j] + D], want)
    assert int(written.sum()) == k.B * (k.C + k.Fd) * D < out.numel()
    EC.same_bits(out[~written], EC.filled(int((~written).sum())), "nobody's slot")
    # the edges: -1 and vocab zero the slot and raise the flag, vocab - 1 is a row
    k = EC.gather_case(D)
    out, _, flag = EC.gather_ref(k)
    o = k.col_off[0]
    assert flag == EC.BAD_ID and not out[:2, o:o + D].any()
    assert torch.equal(out[2, o:o + D], k.table.host()[k.vocabs[0] - 1])
    assert k.table.block.stride(0) > D and k.table.block.stride(0) % k.vec == 0 and k.ids.block.shape[1] > k.C


@pytest.mark.parametrize("D", [1, 16, 126])
def test_pool_reference_is_the_oracle_pooling_of_embedding_rows(D):
    k = EC.pool_case(D)
    pooled, denom, flag = EC.pool_ref(k, F64)
    assert flag == 0 and EC.POOL_MEAN in k.modes and EC.POOL_SUM in k.modes
    ids, table = k.ids.host().long(), k.table.host().double()
    for s, L in enumerate(k.lens):
        x = ids[:, k.seq_col0[s]:k.seq_col0[s] + L]
        e = Fn.embedding(x + s * k.V, table)
        want = (O.masked_average_pooling if k.modes[s] == EC.POOL_MEAN else O.masked_sum_pooling)(e)
        assert (pooled[:, s] - want).abs().max().item() <= 1e-13
        cnt = (e.sum(-1) != 0).float().sum(-1)
        assert torch.equal(denom[:, s], cnt + 1e-12)
        assert cnt[0] == 0 and cnt[1] == L and (x[2] == 0).any() and (L < 3 or x[2, L - 1] != 0)
        if D >= 2 and L >= 2:                                   # the zero-sum row is a row, yet it is not counted
            assert x[4, 0] == 1 and table[s * k.V + 1].abs().sum() == 2 and cnt[4] == (x[4, 1:] != 0).sum()
    kb = EC.pool_case(D, bad=True)
    pb, db, flag = EC.pool_ref(kb, F64)
    assert flag == EC.BAD_ID
    # a bad id contributes nothing: the same sample with the id replaced by padding
    ids_b = kb.ids.host()
    fixed = ids_b.clone()
    fixed[(ids_b < 0) | (ids_b >= kb.V)] = 0
    kb.ids.block[kb.ids.rows, kb.ids.cols] = fixed
    pf, df, flag = EC.pool_ref(kb, F64)
    assert flag == 0 and torch.equal(pb, pf) and torch.equal(db, df)


@pytest.mark.parametrize("D,B", [(3, 17), (16, 1000)])
def test_numeric_gradient_reference_is_autograd_of_the_expansion(D, B):
    k = EC.numgrad_case(D, B)
    W = torch.zeros(k.Fd, D, dtype=F64, requires_grad=True)
    dense, dout = k.dense.host().double(), k.dout.host().double()
    rec = torch.zeros(B, dout.shape[1], dtype=F64)
    parts = [dense[:, j:j + 1] * W[j] for j in range(k.Fd)]
    loss = sum((p * dout[:, o:o + D]).sum() for p, o in zip(parts, k.num_off)) + rec.sum()
    loss.backward()
    ref = EC.numgrad_ref(k, F64)
    assert (ref - W.grad).abs().max().item() <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert EC.numgrad_ref(k, torch.float32).dtype == torch.float32


@pytest.mark.parametrize("F,D", [(1, 3), (5, 16), (39, 65)])
def test_fm_reference_is_the_oracle_product_sum_and_its_autograd(F, D):
    k = EC.fm_case(F, D)
    e = k.emb.host().double().view(k.B, F, D).clone().requires_grad_(True)
    want = O.fm_product_sum(e)[:, 0] + k.addend.double()
    ref = EC.fm_ref(k.emb.host().view(k.B, F, D), k.addend, F64)
    assert (ref - want.detach()).abs().max().item() <= 1e-12
    want.backward(k.g.double())
    gref = EC.fm_grad_ref(k.emb.host().view(k.B, F, D), k.g, None, F64)
    assert (gref - e.grad).abs().max().item() <= 1e-12
    acc = EC.fm_grad_ref(k.emb.host().view(k.B, F, D), k.g, k.demb0, F64)
    assert (acc - gref - k.demb0.double().view(k.B, F, D)).abs().max().item() <= 1e-12
    if F == 1:
        assert ref.sub(k.addend.double()).abs().max().item() <= 1e-15      # no pairs: the term is zero


@pytest.mark.parametrize("C,Fd", [(0, 1), (17, 0), (40, 17)])
def test_lr_reference_is_the_sum_of_the_one_wide_rows(C, Fd):
    k = EC.lr_case(C, Fd)
    ref, flag = EC.lr_ref(k, True, F64)
    t = k.table1.host().double()
    want = torch.zeros(k.B, dtype=F64) + k.bias.double()
    for c in range(C):
        want = want + Fn.embedding(k.ids.host()[:, c].long() + k.bases[c], t)[:, 0]
    if Fd:
        want = want + k.dense.host().double() @ k.w1.double()
    assert flag == 0 and (ref - want).abs().max().item() <= 1e-13
    assert k.table1.block.stride(0) == 3
    if C:
        kb = EC.lr_case(C, Fd, bad=True)
        rb, flag = EC.lr_ref(kb, False, F64)
        assert flag == EC.BAD_ID and torch.isfinite(rb).all()


@pytest.mark.parametrize("F,D,tail", [(2, 2, 0), (5, 34, 37), (31, 30, 30), (33, 4, 0)])
def test_dot_reference_is_bmm_triu_and_its_autograd(F, D, tail):
    k = EC.dot_case(F, D, tail=tail)
    e = k.emb.host().double().view(k.B, F, D).clone().requires_grad_(True)
    want = O.dot_interaction(e)
    if tail:
        want = torch.cat([want, e[:, F - 1], torch.zeros(k.B, tail - D, dtype=F64)], 1)
    ref = EC.dot_ref(k.emb.host().view(k.B, F, D), tail, F64)
    assert ref.shape == (k.B, k.P + tail) and (ref - want.detach()).abs().max().item() <= 1e-12
    want.backward(k.g.host().double())
    gref = EC.dot_grad_ref(k.emb.host().view(k.B, F, D), k.g.host(), tail, F64)
    assert (gref - e.grad).abs().max().item() <= 1e-12


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("D", [2, 65])
def test_reduce_reference_is_index_add_over_the_lookups(D, scaled):
    k = EC.reduce_standard(D, scaled)
    ref = EC.reduce_ref(k, F64)
    dout = k.dout.host().double()
    want = torch.zeros(k.nu, D, dtype=F64)
    for i in range(k.n):                                        # one lookup at a time
        if not k.live[i]:
            continue
        b, c = int(k.pos[i]) // k.C, int(k.pos[i]) % k.C
        v = dout[b, k.col_off[c]:k.col_off[c] + D]
        if scaled and k.col_denom[c] >= 0:
            v = v / k.denom.host()[b, k.col_denom[c]].double()
        want[k.row_of[i]] += v
    assert (ref - want).abs().max().item() <= 1e-12 * max(1.0, float(want.abs().max()))
    r32 = EC.reduce_ref(k, torch.float32)                       # the yardstick: fp32, one lookup after the other
    assert r32.dtype == torch.float32
    if not scaled:
        acc = torch.zeros(k.nu, D)
        for i in range(k.n):
            if k.live[i]:
                b, c = int(k.pos[i]) // k.C, int(k.pos[i]) % k.C
                acc[k.row_of[i]] += k.dout.host()[b, k.col_off[c]:k.col_off[c] + D]
        assert torch.equal(r32, acc)
    # a padding lookup counted after all would be seen
    k.live[:] = True
    assert (EC.reduce_ref(k, F64) - ref).abs().max().item() > 1e-3


def test_the_acceptance_helpers_raise_on_what_they_are_there_to_catch():
    k = EC.fm_case(5, 16)
    e = k.emb.host().view(k.B, 5, 16)
    r64, r32 = EC.fm_ref(e, None, F64), EC.fm_ref(e, None, torch.float32)
    EC.within_yardstick(r32, r32, r64, EC.floor_of(r64), "stand-in")
    off = r32.clone()
    off[3] *= 1 + 1e-5
    with pytest.raises(AssertionError, match="stand-in"):
        EC.within_yardstick(off, r32, r64, EC.floor_of(r64), "stand-in")
    with pytest.raises(AssertionError, match="differs"):
        EC.same_bits(off, r32, "stand-in")
    v = EC.View(torch.zeros(4, 6), margin=2)
    v.on("cpu")[:] = 1.0
    v.untouched("stand-in")
    v.dev_block[0, 3] = 0.0                                      # the guard row above
    with pytest.raises(AssertionError, match="written outside its slots"):
        v.untouched("stand-in")
    v.on("cpu")[1, 2] = 5.0                                      # inside the view, outside what a launch may write
    with pytest.raises(AssertionError, match="written outside its slots"):
        v.untouched("stand-in", written=torch.zeros(4, 6, dtype=torch.bool))
