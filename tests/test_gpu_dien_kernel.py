"""fx_gru_seq_* and fx_seq_score_* alone, through ops, on a real MI355X against the fp64 torch-autograd restatement of
the layers' formulas (test_dien_host.gru_seq / seq_score; no nn.GRU, no packing).

Yardstick (that of tests/test_gpu_mhsa.py and tests/test_gpu_bst_kernel.py): per compared tensor e32 = max |the same
formulas in fp32 torch on the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  The observed
err / bound is printed per tensor.  tanh and sigmoid have no kinks: no sample is left out.

Lengths per sample in turn: 0, 1, L, about L / 2, and a history with zero ids inside its first len positions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_dien_host import gru_seq, seq_score  # noqa: E402

DEV = torch.device("cuda", 0)


def make_ids(B, L, rng):
    ids = rng.integers(1, 50, size=(B, L)).astype(np.int32)
    for b in range(B):
        kind = b % 5
        if kind == 0:
            ids[b, :] = 0
        elif kind == 1:
            ids[b, 1:] = 0
        elif kind == 3:
            ids[b, max(1, L // 2):] = 0
        elif kind == 4 and L >= 3:
            ids[b, 1] = 0                     # inside the first len = L - 2 positions
            ids[b, L - 1] = 0
    return torch.from_numpy(ids)


def bound_check(tag, name, hip, r64, r32):
    assert torch.isfinite(hip).all(), (tag, name)
    e32 = float((r32.double() - r64).abs().max())
    bound = 4.0 * e32 + 1e-6 * float(r64.abs().max())
    err = float((hip.double() - r64).abs().max())
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print("%s %-8s err %.3e bound %.3e ratio %.3f" % (tag, name, err, bound, ratio))
    assert err <= bound, (tag, name, err, bound)


def gru_case(B, L, H, n_parts, mode, seed):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, s=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * s
    D = H // n_parts
    u = 1.0 / H ** 0.5
    parts = [rnd(B, L, D, s=0.8) for _ in range(n_parts)]
    w = [rnd(3 * H, H, s=u), rnd(3 * H, H, s=u), rnd(3 * H, s=0.2), rnd(3 * H, s=0.2)]
    ids = make_ids(B, L, np.random.default_rng(seed))
    scores = torch.rand(B, L, generator=g, dtype=torch.float64) if mode != "GRU" else None
    gs, gf = rnd(B, L, H), rnd(B, H)
    return parts, ids, scores, w, gs, gf


def gru_reference(case, mode, dtype):
    parts, ids, scores, w, gs, gf = case

    def leaf(t):
        return None if t is None else t.to(dtype).clone().requires_grad_(True)
    lp, la, lw = [leaf(t) for t in parts], leaf(scores), [leaf(t) for t in w]
    s, f = gru_seq(lp, ids, la, mode, *lw)
    wanted = {"dx%d" % i: t for i, t in enumerate(lp)}
    wanted.update(zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), lw))
    if la is not None:
        wanted["dscores"] = la
    got = torch.autograd.grad((s * gs.to(dtype)).sum() + (f * gf.to(dtype)).sum(), list(wanted.values()))
    out = {"states": s.detach(), "final": f.detach()}
    out.update(zip(wanted.keys(), [t.detach() for t in got]))
    return out


def gru_hip(case, mode):
    parts, ids, scores, w, gs, gf = case

    def d(t):
        return None if t is None else t.float().to(DEV).contiguous()
    B, L, D = parts[0].shape
    H = D * len(parts)
    hp, hw, ha, hid = [d(t) for t in parts], [d(t) for t in w], d(scores), ids.to(DEV)
    states = torch.full((B, L, H), float("nan"), dtype=torch.float32, device=DEV)
    final = torch.full((B, H), float("nan"), dtype=torch.float32, device=DEV)
    ops.gru_seq_fwd(hp, hid, ha, mode, *hw, states, final)
    dparts = [torch.full_like(t, float("nan")) for t in hp]
    dsc = torch.full((B, L), float("nan"), dtype=torch.float32, device=DEV) if ha is not None else None
    grads = torch.empty(ops.gru_grad_floats(H), dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.gru_workspace_floats(B, H), dtype=torch.float32, device=DEV)
    ops.gru_seq_bwd(hp, hid, ha, mode, *hw, states, d(gs), d(gf), dparts, dsc, grads, ws)
    torch.cuda.synchronize()
    HH = 3 * H * H
    out = {"states": states, "final": final, "dw_ih": grads[:HH].view(3 * H, H), "dw_hh": grads[HH:2 * HH].view(3 * H, H),
           "db_ih": grads[2 * HH:2 * HH + 3 * H], "db_hh": grads[2 * HH + 3 * H:]}
    out.update({"dx%d" % i: t for i, t in enumerate(dparts)})
    if dsc is not None:
        out["dscores"] = dsc
    return {k: v.cpu() for k, v in out.items()}


def gru_shapes():
    """(B, L, H, parts): every H and L of the list, B = 1, 7, 33 and one just past two sample tiles (H = 4: 128 rows
    per tile, H = 64: 8), one and two parts; H = 24 leaves 16 of the 256 threads without a unit."""
    return [(1, 1, 4, 1), (7, 3, 8, 2), (33, 6, 24, 2), (2 * ops.gru_tile_rows(64) + 1, 51, 64, 1),
            (2 * ops.gru_tile_rows(4) + 1, 6, 4, 1), (33, 51, 32, 2)]


@pytest.mark.parametrize("mode", ["GRU", "AGRU", "AUGRU"])
@pytest.mark.parametrize("shape", range(6))
def test_gru_layer_against_fp64(shape, mode):
    B, L, H, n_parts = gru_shapes()[shape]
    case = gru_case(B, L, H, n_parts, mode, seed=300 + shape)
    tag = "B%d L%d H%d p%d %s" % (B, L, H, n_parts, mode)
    r64, r32, hip = gru_reference(case, mode, torch.float64), gru_reference(case, mode, torch.float32), \
        gru_hip(case, mode)
    for name in r64:
        bound_check(tag, name, hip[name], r64[name], r32[name])
    ids = case[1]
    lens = (ids != 0).sum(dim=1)
    past = torch.arange(L).unsqueeze(0) >= lens.unsqueeze(1)
    assert float(hip["states"][past].abs().max() if past.any() else 0) == 0          # exact zeros past len
    empty = lens == 0
    if empty.any():
        assert float(hip["final"][empty].abs().max()) == 0
        for i in range(n_parts):
            assert float(hip["dx%d" % i][empty].abs().max()) == 0                      # and in their gradients
        if mode != "GRU":
            assert float(hip["dscores"][empty].abs().max()) == 0
    if mode == "AGRU":                                    # the unused u chunk: exact zeros, not rounding residue
        for name in ("dw_ih", "dw_hh", "db_ih", "db_hh"):
            assert float(hip[name][:H].abs().max()) == 0, name
            assert float(hip[name][H:].abs().max()) > 0 or not (lens > 0).any(), name      # (B = 1: an empty history)


def test_gru_only_one_upstream_gradient():
    """d_states alone (the extraction layer under "GRU") and d_final alone (the evolution layer)."""
    case = gru_case(9, 6, 8, 1, "AUGRU", seed=41)
    parts, ids, scores, w, gs, gf = case
    for which in ("states", "final"):
        zs, zf = (gs, torch.zeros_like(gf)) if which == "states" else (torch.zeros_like(gs), gf)
        sub = (parts, ids, scores, w, zs, zf)
        r64, r32 = gru_reference(sub, "AUGRU", torch.float64), gru_reference(sub, "AUGRU", torch.float32)

        def d(t):
            return t.float().to(DEV).contiguous()
        hp, hw, ha, hid = [d(t) for t in parts], [d(t) for t in w], d(scores), ids.to(DEV)
        states, final = torch.empty(9, 6, 8, device=DEV), torch.empty(9, 8, device=DEV)
        ops.gru_seq_fwd(hp, hid, ha, "AUGRU", *hw, states, final)
        dx, dsc = torch.empty_like(hp[0]), torch.empty(9, 6, device=DEV)
        grads = torch.empty(ops.gru_grad_floats(8), device=DEV)
        ws = torch.empty(ops.gru_workspace_floats(9, 8), device=DEV)
        ops.gru_seq_bwd(hp, hid, ha, "AUGRU", *hw, states, d(gs) if which == "states" else None,
                        d(gf) if which == "final" else None, [dx], dsc, grads, ws)
        torch.cuda.synchronize()
        bound_check(which, "dx0", dx.cpu(), r64["dx0"], r32["dx0"])
        bound_check(which, "dscores", dsc.cpu(), r64["dscores"], r32["dscores"])
        bound_check(which, "dw_hh", grads[192:384].view(24, 8).cpu(), r64["dw_hh"], r32["dw_hh"])


def score_case(B, L, H, n_parts, bilinear, seed):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, s=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * s
    interest = torch.tanh(rnd(B, L, H))
    tgts = [rnd(B, H // n_parts, s=0.8) for _ in range(n_parts)]
    W = torch.eye(H, dtype=torch.float64) + rnd(H, H, s=0.1) if bilinear else None
    return interest, tgts, make_ids(B, L, np.random.default_rng(seed)), W, rnd(B, L)


def score_reference(case, softmax, dtype):
    interest, tgts, ids, W, gy = case

    def leaf(t):
        return None if t is None else t.to(dtype).clone().requires_grad_(True)
    li, lt, lw = leaf(interest), [leaf(t) for t in tgts], leaf(W)
    s = seq_score(li, lt, ids, lw, softmax)
    wanted = {"dinterest": li}
    wanted.update({"dtgt%d" % i: t for i, t in enumerate(lt)})
    if lw is not None:
        wanted["dW"] = lw
    got = torch.autograd.grad(s, list(wanted.values()), gy.to(dtype))
    out = {"scores": s.detach()}
    out.update(zip(wanted.keys(), [t.detach() for t in got]))
    return out


def score_hip(case, softmax):
    interest, tgts, ids, W, gy = case

    def d(t):
        return None if t is None else t.float().to(DEV).contiguous()
    B, L, H = interest.shape
    hi, ht, hw, hid = d(interest), [d(t) for t in tgts], d(W), ids.to(DEV)
    scores = torch.full((B, L), float("nan"), dtype=torch.float32, device=DEV)
    ops.seq_score_fwd(hi, ht, hid, hw, softmax, scores)
    di = torch.full_like(hi, float("nan"))
    dt = [torch.full_like(t, float("nan")) for t in ht]
    dW = torch.empty(H, H, dtype=torch.float32, device=DEV) if hw is not None else None
    ws = torch.empty(ops.seq_score_workspace_floats(B, H), dtype=torch.float32, device=DEV)
    ops.seq_score_bwd(hi, ht, hid, hw, softmax, scores, d(gy), di, dt, dW, ws)
    torch.cuda.synchronize()
    out = {"scores": scores, "dinterest": di}
    out.update({"dtgt%d" % i: t for i, t in enumerate(dt)})
    if dW is not None:
        out["dW"] = dW
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("bilinear", [True, False])
@pytest.mark.parametrize("shape", [(1, 1, 4, 1), (7, 3, 8, 2), (33, 6, 24, 2), (17, 51, 64, 1), (1027, 6, 4, 1),
                                   (33, 256, 32, 2)], ids=str)
def test_scores_against_fp64(shape, bilinear, softmax):
    """B = 1027 is past the 256-workgroup grid of four samples each; L = 256 fills the four positions of a lane."""
    B, L, H, n_parts = shape
    case = score_case(B, L, H, n_parts, bilinear, seed=500 + B + L)
    tag = "B%d L%d H%d p%d %s sm%d" % (B, L, H, n_parts, "bil" if bilinear else "dot", softmax)
    r64, r32, hip = score_reference(case, softmax, torch.float64), score_reference(case, softmax, torch.float32), \
        score_hip(case, softmax)
    for name in r64:
        bound_check(tag, name, hip[name], r64[name], r32[name])
    empty = (case[2] != 0).sum(dim=1) == 0
    if empty.any():                                       # len 0: zero scores and zero gradients, nothing NaN
        assert float(hip["scores"][empty].abs().max()) == 0 and float(hip["dinterest"][empty].abs().max()) == 0
        for i in range(n_parts):
            assert float(hip["dtgt%d" % i][empty].abs().max()) == 0
    closed = case[2] == 0
    assert float(hip["scores"][closed].abs().max() if closed.any() else 0) == 0


SENTINEL = 3.0


def _only_views_written(records, views):
    """Every element of the sentinel-filled `records` outside the listed (record index, slices) is still the sentinel."""
    for k, rec in enumerate(records):
        touched = torch.zeros_like(rec, dtype=torch.bool)
        for r, where in views:
            if r == k:
                touched[where] = True
        assert bool((rec[~touched] == SENTINEL).all()), "record %d written outside its views" % k


def test_gru_parts_in_a_wider_record_and_null_destinations():
    """The two parts are views into NaN-filled records [B, L + 3, D + 3] at slot and column offsets of their own
    (one record per part: two [L, D] blocks at different offsets do not fit one [L + 3, D + 3] slab side by side),
    read in place; the gradients go through views of sentinel-filled records with the same strides and the bytes
    around them stay untouched; a null destination is skipped and changes nothing else."""
    B, L, D, mode = 9, 6, 4, "AUGRU"
    H = 2 * D
    case = gru_case(B, L, H, 2, mode, seed=77)
    parts, ids, scores, w, gs, gf = case
    r64, r32 = gru_reference(case, mode, torch.float64), gru_reference(case, mode, torch.float32)
    where = [(slice(None), slice(1, 1 + L), slice(0, D)), (slice(None), slice(3, 3 + L), slice(2, 2 + D))]
    recs = [torch.full((B, L + 3, D + 3), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2)]
    views = [rec[s] for rec, s in zip(recs, where)]
    for view, src in zip(views, parts):
        view.copy_(src.float())
    assert all(v.stride() == ((L + 3) * (D + 3), D + 3, 1) for v in views)

    def d(t):
        return t.float().to(DEV).contiguous()
    hw, ha, hid = [d(t) for t in w], d(scores), ids.to(DEV)
    states = torch.full((B, L, H), float("nan"), dtype=torch.float32, device=DEV)
    final = torch.full((B, H), float("nan"), dtype=torch.float32, device=DEV)
    ops.gru_seq_fwd(views, hid, ha, mode, *hw, states, final)
    torch.cuda.synchronize()
    bound_check("wide", "states", states.cpu(), r64["states"], r32["states"])
    bound_check("wide", "final", final.cpu(), r64["final"], r32["final"])

    def backward(wanted):
        drecs = [torch.full_like(rec, SENTINEL) for rec in recs]
        dparts = [drec[s] if keep else None for drec, s, keep in zip(drecs, where, wanted)]
        dsc = torch.full((B, L), float("nan"), dtype=torch.float32, device=DEV)
        grads = torch.empty(ops.gru_grad_floats(H), dtype=torch.float32, device=DEV)
        ws = torch.empty(ops.gru_workspace_floats(B, H), dtype=torch.float32, device=DEV)
        ops.gru_seq_bwd(views, hid, ha, mode, *hw, states, d(gs), d(gf), dparts, dsc, grads, ws)
        torch.cuda.synchronize()
        _only_views_written(drecs, [(k, where[k]) for k in range(2) if wanted[k]])
        return dparts, dsc, grads
    dparts, dsc, grads = backward((True, True))
    for i in range(2):
        bound_check("wide", "dx%d" % i, dparts[i].cpu(), r64["dx%d" % i], r32["dx%d" % i])
    bound_check("wide", "dscores", dsc.cpu(), r64["dscores"], r32["dscores"])
    bound_check("wide", "dw_ih", grads[:3 * H * H].view(3 * H, H).cpu(), r64["dw_ih"], r32["dw_ih"])
    again, dsc2, grads2 = backward((True, False))
    assert again[1] is None and torch.equal(again[0], dparts[0])
    assert torch.equal(dsc2, dsc) and torch.equal(grads2, grads)


def test_score_targets_in_a_wider_record_and_null_destinations():
    """The same for the scores' target: two parts as views rec[:, 1, :D] and rec[:, 2, 1:D + 1] of one NaN-filled
    record, their gradients through the same views of a sentinel-filled one, then with part 0's destination null."""
    B, L, D = 9, 6, 4
    H = 2 * D
    case = score_case(B, L, H, 2, True, seed=78)
    interest, tgts, ids, W, gy = case
    r64, r32 = score_reference(case, True, torch.float64), score_reference(case, True, torch.float32)
    where = [(slice(None), 1, slice(0, D)), (slice(None), 2, slice(1, D + 1))]
    rec = torch.full((B, 4, D + 3), float("nan"), dtype=torch.float32, device=DEV)
    views = [rec[s] for s in where]
    for view, src in zip(views, tgts):
        view.copy_(src.float())
    assert all(v.stride() == (4 * (D + 3), 1) for v in views)

    def d(t):
        return t.float().to(DEV).contiguous()
    hi, hw, hid = d(interest), d(W), ids.to(DEV)
    scores = torch.full((B, L), float("nan"), dtype=torch.float32, device=DEV)
    ops.seq_score_fwd(hi, views, hid, hw, True, scores)
    torch.cuda.synchronize()
    bound_check("wide", "scores", scores.cpu(), r64["scores"], r32["scores"])

    def backward(wanted):
        drec = torch.full_like(rec, SENTINEL)
        dtgts = [drec[s] if keep else None for s, keep in zip(where, wanted)]
        di = torch.full_like(hi, float("nan"))
        dW = torch.empty(H, H, dtype=torch.float32, device=DEV)
        ws = torch.empty(ops.seq_score_workspace_floats(B, H), dtype=torch.float32, device=DEV)
        ops.seq_score_bwd(hi, views, hid, hw, True, scores, d(gy), di, dtgts, dW, ws)
        torch.cuda.synchronize()
        _only_views_written([drec], [(0, where[k]) for k in range(2) if wanted[k]])
        return dtgts, di, dW
    dtgts, di, dW = backward((True, True))
    for i in range(2):
        bound_check("wide", "dtgt%d" % i, dtgts[i].cpu(), r64["dtgt%d" % i], r32["dtgt%d" % i])
    bound_check("wide", "dinterest", di.cpu(), r64["dinterest"], r32["dinterest"])
    bound_check("wide", "dW", dW.cpu(), r64["dW"], r32["dW"])
    again, di2, dW2 = backward((False, True))
    assert again[0] is None and torch.equal(again[1], dtgts[1])
    assert torch.equal(di2, di) and torch.equal(dW2, dW)


def test_two_runs_give_the_same_bits():
    case = gru_case(33, 51, 32, 2, "AUGRU", seed=5)
    a, b = gru_hip(case, "AUGRU"), gru_hip(case, "AUGRU")
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sc = score_case(33, 51, 32, 2, True, seed=6)
    a, b = score_hip(sc, True), score_hip(sc, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_limits_are_rejected_before_any_launch():
    with pytest.raises(NotImplementedError, match="4 <= H <= 64"):
        gru_hip(gru_case(2, 3, 68, 1, "GRU", seed=1), "GRU")
    with pytest.raises(NotImplementedError, match="1 <= L <= 256"):
        score_hip(score_case(2, 257, 8, 1, True, seed=1), True)
