"""The field-pair kernels (csrc/fx_pairfm.hip) alone, through fuxictr_amd.ops, on a real MI355X against the fp64
restatement of tests/test_pairfm_host.py (pairfm_composition and torch autograd of it):
    out = sum_p u_p(x_i) . x_j (+ wlin . x) (+ bias) (+ addend),  u_p = r_p x / w_p * x / x^T M_p.

The tolerance is the yardstick of tests/test_gpu_layernorm.py (`compare`, `f32_exact`), the rule of
tests/test_gpu_afm_attn.py: the same composition in fp32 torch on the CPU has an error e32 against the fp64 result, per
output tensor (max |.|); the HIP result must lie within
    4 * e32 + 1e-6 * max|ref|.
Every case prints its observed ratio err / bound.  The inputs are fp32 numbers of O(1), so all three computations
start from the same values and no term underflows.  No element is left out of any comparison.

The record and dX are the columns [off, off + F*D) of wider rows with `tail` more columns behind them, sentinels
outside: off 0 / tail 0 is the packed case (the 16-byte arm when D % 4 == 0), off 4 the 16-byte arm through a row
stride, off 1 a base that is only 4-byte aligned and tail 3 a row stride that is no multiple of 4 (the 4-byte arm,
also at D = 8)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402
from test_pairfm_host import pairfm_composition  # noqa: E402

DEV = "cuda:0"
LIM = ops.pairfm_limits()
MODES = ("scalar", "vector", "matrix")
SHAPES = [(mode, F, D) for mode in MODES for F in (2, 3, 9) for D in (4, 8, 10, 16)] + \
         [(mode, F, 1) for mode in ("scalar", "vector") for F in (2, 3, 9) if ops.pairfm_in_envelope(F, 1)]


def w_shape(mode, F, D):
    P = F * (F - 1) // 2
    return (P, D, D) if mode == "matrix" else (P, D) if mode == "vector" else (P,)


def draw_once(mode, B, F, D, seed):
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s, scale=1.0):
        return f32_exact(scale * torch.randn(*s, generator=gen, dtype=torch.float64))
    return dict(x=rnd(B, F, D), W=rnd(*w_shape(mode, F, D), scale=(D ** -0.5 if mode == "matrix" else 1.0)),
                wlin=rnd(F * D), bias=rnd(1), add=rnd(B, 1), g=rnd(B, 1))


def draw(mode, B, F, D, seed):
    """Inputs from the first of 8 consecutive seeds whose fp64 reference is no cancellation residue.  dbias = sum_b g_b
    is the one output that is a single bare sum of inputs: where the g_b cancel to a small fraction of sum_b |g_b| and
    torch's fp32 sum of so few terms happens to be exact (e32 = 0), the yardstick's floor 1e-6 |ref| lies below one
    rounding of ANY fp32 partial sum.  The condition is on the reference alone (as the ReLU margin of
    tests/test_gpu_afm_attn.py): |sum g| >= 0.05 sum |g|."""
    for s in range(seed, seed + 8):
        inp = draw_once(mode, B, F, D, s)
        if float(inp["g"].sum().abs()) >= 0.05 * float(inp["g"].abs().sum()):
            return inp
    raise AssertionError("no seed in [%d, %d) keeps |sum g| >= 0.05 sum |g|" % (seed, seed + 8))


def run_torch(inp, mode, dtype, wlin=True, bias=True, addend=True):
    t = {k: v.to(dtype).clone() for k, v in inp.items()}
    names = ["x", "W"] + (["wlin"] if wlin else []) + (["bias"] if bias else []) + (["add"] if addend else [])
    for k in names:
        t[k].requires_grad_(True)
    out = pairfm_composition(t["x"], t["W"], mode, t["wlin"] if wlin else None, t["bias"] if bias else None,
                             t["add"] if addend else None)
    grads = dict(zip(names, torch.autograd.grad(out, [t[k] for k in names], t["g"])))
    B = t["x"].shape[0]
    res = {"out": out.detach(), "dX": grads["x"].reshape(B, -1), "dW": grads["W"]}
    if wlin:
        res["dwlin"] = grads["wlin"]
    if bias:
        res["dbias"] = grads["bias"]
    if addend:
        res["dadd"] = grads["add"]
    return {k: v.double() for k, v in res.items()}


def run_hip(inp, mode, off=0, tail=0, wlin=True, bias=True, addend=True):
    B, F, D = inp["x"].shape
    FD = F * D
    recw = torch.full((B, off + FD + tail), 7.0, dtype=torch.float32, device=DEV)
    rec = recw[:, off:off + FD]
    rec.copy_(inp["x"].reshape(B, FD).float())
    dxw = torch.full((B, off + FD + tail), 3.0, dtype=torch.float32, device=DEV)
    dX = dxw[:, off:off + FD]
    w = {k: inp[k].float().to(DEV).contiguous() for k in ("W", "wlin", "bias", "add", "g")}
    out = torch.full((B, 1), 5.0, dtype=torch.float32, device=DEV)
    ops.pairfm_fwd(rec, F, D, mode, w["W"], w["wlin"] if wlin else None, w["bias"] if bias else None,
                   w["add"] if addend else None, out)
    n = ops.pairfm_grad_floats(mode, F, D, wlin, bias)
    grads = torch.full((n + 2,), 4.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.pairfm_workspace_floats(mode, B, F, D), dtype=torch.float32, device=DEV)
    ops.pairfm_bwd(w["g"], rec, F, D, mode, w["W"], w["wlin"] if wlin else None, bias, dX, grads[:n], ws)
    torch.cuda.synchronize()
    # nobody's columns, and the floats behind grads
    for buf, fill in ((recw, 7.0), (dxw, 3.0)):
        assert bool((buf[:, :off] == fill).all()) and bool((buf[:, off + FD:] == fill).all())
    assert bool((grads[n:] == 4.0).all())
    # the inputs are read only
    assert torch.equal(rec.cpu(), inp["x"].reshape(B, FD).float())
    for k in ("W", "wlin", "bias", "add", "g"):
        assert torch.equal(w[k].cpu(), inp[k].float()), k
    nW = w["W"].numel()
    res = {"out": out.clone(), "dX": dX.contiguous(), "dW": grads[:nW].reshape(w["W"].shape).clone()}
    o = nW
    if wlin:
        res["dwlin"] = grads[o:o + FD].clone()
        o += FD
    if bias:
        res["dbias"] = grads[o:o + 1].clone()
    if addend:
        res["dadd"] = w["g"].clone()                # the addend's gradient is g itself (layers._PairFMFn)
    return res


def check(tag, inp, mode, ref, f32, **kw):
    got = run_hip(inp, mode, **kw)
    assert sorted(got) == sorted(ref)
    compare(tag, got, ref, f32)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-F%d-D%d" % s)
def test_forward_and_gradients_within_the_fp32_yardstick(shape):
    """B one sample, one below, at and above a workgroup's tile, and two tiles and three (more than one slab of the
    weight gradient); wlin / bias / addend all present and all absent; at the largest B every layout."""
    mode, F, D = shape
    T = ops.pairfm_tile_rows(mode, F, D)
    assert T >= 16
    sizes = sorted({1, T - 1, T, T + 1, 2 * T + 3})
    # the weight gradient at 2 T + 3 samples spans more than one slab: partial rows and the reduce's own workspace
    n_all = ops.pairfm_weight_floats(mode, F, D) + F * D + 1
    assert ops.pairfm_workspace_floats(mode, 2 * T + 3, F, D) >= 2 * n_all
    assert ops.pairfm_workspace_floats(mode, T, F, D) < n_all or n_all <= 4
    for k, B in enumerate(sizes):
        inp = draw(mode, B, F, D, seed=1000 * B + 100 * F + D + len(mode))
        last = B == sizes[-1]
        for opts in ([True, False] if last else [k % 2 == 0]):
            kw = dict(wlin=opts, bias=opts, addend=opts)
            ref, f32 = run_torch(inp, mode, torch.float64, **kw), run_torch(inp, mode, torch.float32, **kw)
            layouts = [(0, 0), (4, 0), (1, 0), (0, 3), (1, 3)] if (last and opts) else [(0, 0)]
            for off, tail in layouts:
                tag = "pairfm %s B %d off %d tail %d opts %d" % (shape, B, off, tail, opts)
                first = check(tag, inp, mode, ref, f32, off=off, tail=tail, **kw)
                if last and (off, tail) in ((0, 0), (1, 3)):
                    again = run_hip(inp, mode, off=off, tail=tail, **kw)      # the same inputs: the same bits
                    for name in first:
                        assert torch.equal(first[name], again[name]), (tag, name)


@pytest.mark.parametrize("opts", [(True, False, False), (False, True, False), (False, False, True)],
                         ids=["wlin", "bias", "addend"])
@pytest.mark.parametrize("mode", MODES)
def test_each_optional_term_alone(mode, opts):
    wlin, bias, addend = opts
    B, F, D = 19, 5, 8
    inp = draw(mode, B, F, D, seed=31)
    kw = dict(wlin=wlin, bias=bias, addend=addend)
    ref, f32 = run_torch(inp, mode, torch.float64, **kw), run_torch(inp, mode, torch.float32, **kw)
    for off, tail in ((0, 0), (1, 3)):
        check("pairfm %s only %s off %d" % (mode, opts, off), inp, mode, ref, f32, off=off, tail=tail, **kw)


@pytest.mark.parametrize("mode", MODES)
def test_pair_order_is_that_of_triu_indices(mode):
    """W zero except at one pair — the first, a middle one, the last: out is that pair's term alone, written here from
    the pair's (i, j) of a plain double loop, and dW is non-zero there only."""
    B, F, D = 5, 9, 8
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    for p in (0, len(pairs) // 2, len(pairs) - 1):
        inp = draw(mode, B, F, D, seed=50 + p)
        keep = inp["W"][p].clone()
        inp["W"] = torch.zeros_like(inp["W"])
        inp["W"][p] = keep
        i, j = pairs[p]
        xi, xj = inp["x"][:, i, :], inp["x"][:, j, :]
        if mode == "matrix":
            want = torch.einsum("bd,de,be->b", xi, keep, xj)
        else:
            want = (xi * keep * xj).sum(dim=1)
        kw = dict(wlin=False, bias=False, addend=False)
        ref, f32 = run_torch(inp, mode, torch.float64, **kw), run_torch(inp, mode, torch.float32, **kw)
        assert torch.allclose(ref["out"].reshape(-1), want, rtol=1e-12, atol=1e-12)
        got = check("pairfm %s one pair %d" % (mode, p), inp, mode, ref, f32, **kw)
        touched = [f for f in range(F) if bool((got["dX"].reshape(B, F, D)[:, f, :] != 0).any())]
        assert touched == [i, j], (p, touched)


def test_scalar_mode_with_unit_weights_is_the_fm_pair_sum():
    B, F, D = 35, 9, 8
    inp = draw("scalar", B, F, D, seed=77)
    inp["W"] = torch.ones_like(inp["W"])
    kw = dict(wlin=False, bias=False, addend=True)
    ref, f32 = run_torch(inp, "scalar", torch.float64, **kw), run_torch(inp, "scalar", torch.float32, **kw)
    check("pairfm scalar W = 1", inp, "scalar", ref, f32, **kw)
    rec = inp["x"].reshape(B, F * D).float().to(DEV)
    fm = torch.empty(B, 1, dtype=torch.float32, device=DEV)
    ops.fm_fwd(rec, F, D, inp["add"].float().to(DEV), fm)
    torch.cuda.synchronize()
    compare("fm_fwd against the same reference", {"out": fm}, {"out": ref["out"]}, {"out": f32["out"]})


def test_the_criteo_shape_runs_every_mode_once():
    """F 39, D 16: the shape of scripts/bench_pairfm.py, several workgroup rounds per tile, W in LDS (scalar, vector)."""
    B, F, D = 33, 39, 16
    for mode in MODES:
        inp = draw(mode, B, F, D, seed=9)
        ref, f32 = run_torch(inp, mode, torch.float64), run_torch(inp, mode, torch.float32)
        check("pairfm %s criteo" % mode, inp, mode, ref, f32)


def test_a_wide_record_takes_the_smaller_tile():
    B, F, D = 19, 40, 64                      # F * D = 2560: 8 samples per workgroup
    T = ops.pairfm_tile_rows("matrix", F, D)
    assert 1 <= T < 16
    for mode in ("vector", "matrix"):
        inp = draw(mode, B, F, D, seed=13)
        ref, f32 = run_torch(inp, mode, torch.float64), run_torch(inp, mode, torch.float32)
        check("pairfm %s wide" % mode, inp, mode, ref, f32)


def test_a_shape_outside_the_limits_is_refused_and_launches_nothing():
    from fuxictr_amd._lib import FxError
    B = 4
    for F, D in ((3, LIM["D_max"] + 1), (LIM["FD_max"] // 8 + 1, 8)):
        assert not ops.pairfm_in_envelope(F, D)
        rec = torch.ones(B, F * D, device=DEV)
        W = torch.ones(F * (F - 1) // 2, device=DEV)
        out = torch.full((B, 1), 5.0, device=DEV)
        dX = torch.full((B, F * D), 3.0, device=DEV)
        grads = torch.full((W.numel(),), 4.0, device=DEV)
        ws = torch.zeros(max(4, ops.pairfm_workspace_floats("scalar", B, F, D)), device=DEV)
        with pytest.raises(FxError, match="limit"):
            ops.pairfm_fwd(rec, F, D, "scalar", W, None, None, None, out)
        with pytest.raises(FxError, match="limit"):
            ops.pairfm_bwd(out, rec, F, D, "scalar", W, None, False, dX, grads, ws)
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()) and bool((dX == 3.0).all()) and bool((grads == 4.0).all())
    rec = torch.zeros(B, 24, device=DEV)
    with pytest.raises(AssertionError):
        ops.pairfm_fwd(rec, 4, 8, "scalar", torch.zeros(6, device=DEV), None, None, None, torch.zeros(B, 1, device=DEV))
    with pytest.raises(AssertionError):
        ops.pairfm_fwd(rec, 3, 8, "matrix", torch.zeros(3, 8, device=DEV), None, None, None,
                       torch.zeros(B, 1, device=DEV))
    with pytest.raises(FxError, match="GPU"):
        ops.pairfm_fwd(rec.cpu(), 3, 8, "scalar", torch.zeros(3), None, None, None, torch.zeros(B, 1))
    torch.cuda.synchronize()
