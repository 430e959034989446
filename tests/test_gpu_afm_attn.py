"""AFM's kernels (csrc/fx_afm.hip) alone, through fuxictr_amd.ops, on a real MI355X against an fp64 torch-autograd
restatement of AFM.forward's composition (tests/test_afm_host.py: afm_reference):
    e_p = x_i * x_j,  z_p = W1 e_p + b1,  s_p = w2 . relu(z_p),  a = softmax_p(s),  out = sum_p a_p (wp . e_p) (+ addend)

The tolerance is the yardstick of tests/test_gpu_layernorm.py (`compare`, `f32_exact`): the same composition in fp32
torch on the CPU has an error e32 against the fp64 result, per output tensor (max |.|); the HIP result must lie within
    4 * e32 + 1e-6 * max|ref|.
Every case prints its observed ratio err / bound.  The inputs are fp32 numbers, so all three computations start from
the same values.  No element is left out of any comparison.  The stats row (softmax max, denominator, y without the
addend) is held to the fp64 values by the same yardstick.

A pre-activation within rounding of zero would let the fp64 and the fp32 ReLU masks differ legitimately: the inputs are
drawn from consecutive seeds, at most 8, until the fp64 reference has min |z_p| >= 1e-5 max |z_p|.

The record and dX are the columns [off, off + F*D) of wider rows with `tail` more columns behind them, sentinels
outside: off 0 / tail 0 is the packed case (the 16-byte arm when D % 4 == 0), off 4 the 16-byte arm through a row
stride, off 1 a base that is only 4-byte aligned and tail 3 a row stride that is no multiple of 4 (the scalar arm)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_afm_host import afm_reference, afm_stats_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402

DEV = "cuda:0"
TILE = ops.afm_attn_tile_rows()            # samples one workgroup owns at a time
LIM = ops.afm_attn_limits()

SHAPES = [(1, 2, 1, 1), (3, 3, 4, 1), (5, 4, 5, 3), (7, 11, 10, 10), (7, 12, 8, 8), (5, 39, 16, 16), (3, 64, 8, 4),
          (2, 16, 64, 64)]


def _edge_shapes():
    """The envelope's own edge: the most pairs with the widest D they leave room for, and F * D, D and A at their
    limits together."""
    F = 2
    while (F + 1) * F // 2 <= LIM["P_max"]:
        F += 1
    D = min(LIM["D_max"], LIM["FD_max"] // F)
    F2 = LIM["FD_max"] // LIM["D_max"]
    return [(2, F, D, LIM["A_max"]), (2, F2, LIM["D_max"], LIM["A_max"])]


SHAPES += _edge_shapes()
# one sample below, at and above a workgroup's tile and two tiles and one: the scalar and the 16-byte arm
TILE_SHAPES = [(b, 5, d, a) for b in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1) for d, a in ((6, 3), (8, 4)) if b >= 1]
LAYOUTS = [(off, tail) for off in (0, 1, 4) for tail in (0, 3)]
NAMES = ("out", "m", "den", "y", "dX", "dW1", "db1", "dw2", "dwp", "dadd")


def draw(shape, seed):
    """Up to 2000 pre-activations: W1 e of unit scale around a small b1, so the ReLU masks differ from pair to pair.
    More than that many cannot all keep clear of zero by the margin below unless few come near it: there b1 is
    +-[1, 1.5) and W1 e a fifth of that scale (products of normals: the tails still flip some units)."""
    B, F, D, A = shape
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s, scale=1.0):
        return f32_exact(scale * torch.randn(*s, generator=gen, dtype=torch.float64))
    many = B * (F * (F - 1) // 2) * A > 2000
    inp = dict(x=rnd(B, F, D), W1=rnd(A, D, scale=(0.2 if many else 1.0) * D ** -0.5), b1=rnd(A, scale=0.3), w2=rnd(A),
               wp=rnd(D, scale=D ** -0.5), add=rnd(B, 1), g=rnd(B, 1))
    if many:
        inp["b1"] = f32_exact(torch.sign(inp["b1"]) * (1.0 + 0.5 * torch.rand(A, generator=gen, dtype=torch.float64)))
    return inp


def relu_margin(inp):
    _, z, _, _, _ = afm_reference(inp["x"], inp["W1"], inp["b1"], inp["w2"], inp["wp"], parts=True)
    return float(z.abs().min()), float(z.abs().max())


def make_inputs(shape, seed):
    """inputs from the first of 8 consecutive seeds whose fp64 pre-activations keep clear of zero"""
    for s in range(seed, seed + 8):
        inp = draw(shape, s)
        lo, hi = relu_margin(inp)
        if lo >= 1e-5 * hi:
            return inp
    raise AssertionError("no seed in [%d, %d) keeps min |z| >= 1e-5 max |z| for %s" % (seed, seed + 8, (shape,)))


def run_torch(inp, dtype, addend=True):
    t = {k: v.to(dtype).clone() for k, v in inp.items()}
    for k in ("x", "W1", "b1", "w2", "wp", "add"):
        t[k].requires_grad_(True)
    out = afm_reference(t["x"], t["W1"], t["b1"], t["w2"], t["wp"], t["add"] if addend else None)
    grads = torch.autograd.grad(out, [t["x"], t["W1"], t["b1"], t["w2"], t["wp"]] + ([t["add"]] if addend else []),
                                t["g"])
    with torch.no_grad():
        st = afm_stats_reference(t["x"], t["W1"], t["b1"], t["w2"], t["wp"])
    B = t["x"].shape[0]
    res = {"out": out.detach(), "m": st[:, 0], "den": st[:, 1], "y": st[:, 2], "dX": grads[0].reshape(B, -1),
           "dW1": grads[1], "db1": grads[2], "dw2": grads[3], "dwp": grads[4]}
    if addend:
        res["dadd"] = grads[5]
    return {k: v.double() for k, v in res.items()}


def run_hip(inp, off=0, tail=0, addend=True):
    B, F, D = inp["x"].shape
    A = inp["W1"].shape[0]
    FD = F * D
    recw = torch.full((B, off + FD + tail), 7.0, dtype=torch.float32, device=DEV)
    rec = recw[:, off:off + FD]
    rec.copy_(inp["x"].reshape(B, FD).float())
    dxw = torch.full((B, off + FD + tail), 3.0, dtype=torch.float32, device=DEV)
    dX = dxw[:, off:off + FD]
    w = {k: inp[k].float().to(DEV).contiguous() for k in ("W1", "b1", "w2", "wp", "add", "g")}
    out = torch.full((B, 1), 5.0, dtype=torch.float32, device=DEV)
    stats = torch.full((B, 3), 5.0, dtype=torch.float32, device=DEV)
    ops.afm_attn_fwd(rec, F, D, w["W1"], w["b1"], w["w2"], w["wp"], w["add"] if addend else None, out, stats)
    n = ops.afm_attn_grad_floats(D, A)
    grads = torch.full((n + 2,), 4.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.afm_attn_workspace_floats(B, F, D, A), dtype=torch.float32, device=DEV)
    ops.afm_attn_bwd(w["g"], rec, F, D, w["W1"], w["b1"], w["w2"], w["wp"], stats, dX, grads[:n], ws)
    torch.cuda.synchronize()
    # nobody's columns, and the floats behind grads
    for buf in (recw, dxw):
        fill = 7.0 if buf is recw else 3.0
        assert bool((buf[:, :off] == fill).all()) and bool((buf[:, off + FD:] == fill).all())
    assert bool((grads[n:] == 4.0).all())
    # the inputs are read only
    assert torch.equal(rec.cpu(), inp["x"].reshape(B, FD).float())
    for k in ("W1", "b1", "w2", "wp", "add", "g"):
        assert torch.equal(w[k].cpu(), inp[k].float()), k
    AD = A * D
    res = {"out": out.clone(), "m": stats[:, 0].clone(), "den": stats[:, 1].clone(), "y": stats[:, 2].clone(),
           "dX": dX.contiguous(), "dW1": grads[:AD].reshape(A, D).clone(), "db1": grads[AD:AD + A].clone(),
           "dw2": grads[AD + A:AD + 2 * A].clone(), "dwp": grads[AD + 2 * A:n].clone()}
    if addend:
        res["dadd"] = w["g"].clone()                # the addend's gradient is g itself (layers._AFMAttnFn)
    return res


def check(tag, inp, ref, f32, **kw):
    got = run_hip(inp, **kw)
    assert sorted(got) == sorted(ref)
    compare(tag, got, ref, f32)
    return got


@pytest.mark.parametrize("shape", SHAPES + TILE_SHAPES, ids=lambda s: "B%d-F%d-D%d-A%d" % s)
def test_forward_and_gradients_within_the_fp32_yardstick_in_every_layout(shape):
    inp = make_inputs(shape, seed=8 * (11 + shape[0] + 3 * shape[1] + 5 * shape[2] + 7 * shape[3]))
    refs = {add: (run_torch(inp, torch.float64, add), run_torch(inp, torch.float32, add)) for add in (True, False)}
    big = shape[1] * shape[2] > 1024                 # (the edge shapes: two layouts, both arms where D % 4 == 0)
    for off, tail in (LAYOUTS if not big else [(0, 0), (1, 3)]):
        for addend in ((True, False) if (off, tail) in ((0, 0), (1, 3)) else (True,)):
            ref, f32 = refs[addend]
            tag = "afm_attn %s off %d tail %d addend %d" % (shape, off, tail, addend)
            first = check(tag, inp, ref, f32, off=off, tail=tail, addend=addend)
            if addend and (off, tail) in ((0, 0), (1, 3)):
                again = run_hip(inp, off=off, tail=tail, addend=addend)       # the same inputs: the same bits
                for name in first:
                    assert torch.equal(first[name], again[name]), name


def test_scores_of_plus_and_minus_80_stay_finite_and_the_dominant_pair_wins():
    shape = (4, 5, 6, 4)
    found = None
    for seed in range(300, 308):
        inp = draw(shape, seed)
        _, _, s, t, _ = afm_reference(inp["x"], inp["W1"], inp["b1"], inp["w2"], inp["wp"], parts=True)
        k = int(s.abs().argmax())
        scale = 80.0 / float(s.reshape(-1)[k])       # (negative when the largest |s| is a negative score)
        inp["w2"] = f32_exact(inp["w2"] * scale)
        _, z, s, t, _ = afm_reference(inp["x"], inp["W1"], inp["b1"], inp["w2"], inp["wp"], parts=True)
        top2 = s.topk(2, dim=1).values
        rows = (top2[:, 0] - top2[:, 1] >= 25.0).nonzero().reshape(-1)
        if len(rows) and float(s.max()) >= 79.0 and float(s.min()) <= -40.0 \
                and relu_margin(inp)[0] >= 1e-5 * relu_margin(inp)[1]:
            found = (inp, s, t, rows)
            break
    assert found is not None
    inp, s, t, rows = found
    ref, f32 = run_torch(inp, torch.float64, False), run_torch(inp, torch.float32, False)
    for off, tail in ((0, 0), (1, 3)):
        got = check("afm_attn scores +-80 off %d tail %d" % (off, tail), inp, ref, f32, off=off, tail=tail,
                    addend=False)                    # (compare() asserts that every output is finite)
        for r in rows.tolist():
            tp = float(t[r, int(s[r].argmax())])     # exp(-25) = 1.4e-11: the other pairs are below the yardstick
            bound = 4.0 * float((f32["out"] - ref["out"]).abs().max()) + 1e-6 * float(ref["out"].abs().max())
            assert abs(float(got["out"][r]) - tp) <= bound + 1e-9 * float(t[r].abs().max()), (r, tp)


@pytest.mark.parametrize("dead", [False, True], ids=["zero-W1", "dead-relu"])
def test_uniform_attention(dead):
    """W1 = 0 and b1 = 0: every score is 0; b1 = -100: every ReLU is dead and every score is 0 again: the attention is
    uniform, out = wp . mean_p e_p, and with the dead ReLU dW1, db1 and dw2 are exactly zero."""
    shape = (2 * TILE + 1, 6, 6, 5)
    inp = draw(shape, 77)
    if dead:
        inp["b1"] = torch.full_like(inp["b1"], -100.0)
    else:
        inp["W1"], inp["b1"] = torch.zeros_like(inp["W1"]), torch.zeros_like(inp["b1"])
    ref, f32 = run_torch(inp, torch.float64), run_torch(inp, torch.float32)
    x = inp["x"]
    i, j = torch.triu_indices(shape[1], shape[1], offset=1)
    mean_e = (x[:, i, :] * x[:, j, :]).mean(dim=1)
    want = (mean_e @ inp["wp"]).reshape(-1, 1) + inp["add"]
    assert torch.allclose(ref["out"], want, rtol=1e-12, atol=1e-12)
    for off, tail in ((0, 0), (1, 3)):
        got = check("afm_attn uniform dead %d off %d tail %d" % (dead, off, tail), inp, ref, f32, off=off, tail=tail)
        assert bool((got["m"] == 0).all()) and bool((got["den"] == float(len(i))).all())
        if dead:
            for name in ("dW1", "db1", "dw2"):
                assert bool((got[name] == 0).all()), name


def test_bad_arguments_are_rejected_before_the_launch():
    from fuxictr_amd._lib import FxError
    B, F, D, A = 4, 3, 8, 4
    rec = torch.zeros(B, F * D, device=DEV)
    W1, b1, w2, wp = (torch.zeros(*s, device=DEV) for s in ((A, D), (A,), (A,), (D,)))
    out, stats = torch.zeros(B, 1, device=DEV), torch.zeros(B, 3, device=DEV)
    grads = torch.zeros(ops.afm_attn_grad_floats(D, A), device=DEV)
    ws = torch.zeros(ops.afm_attn_workspace_floats(B, F, D, A), device=DEV)
    with pytest.raises(AssertionError):
        ops.afm_attn_fwd(rec, F + 1, D, W1, b1, w2, wp, None, out, stats)                 # F * D != the columns
    with pytest.raises(AssertionError):
        ops.afm_attn_fwd(rec, F, D, W1, b1[:3], w2, wp, None, out, stats)
    with pytest.raises(AssertionError):
        ops.afm_attn_fwd(rec, F, D, W1, b1, w2, wp, None, out, stats[:, :2])
    with pytest.raises(AssertionError):                                                   # outside the envelope
        ops.afm_attn_fwd(rec[:, :D], 1, D, W1, b1, w2, wp, None, out, stats)
    wide = torch.zeros(LIM["A_max"] + 1, D, device=DEV)
    with pytest.raises(AssertionError):
        ops.afm_attn_fwd(rec, F, D, wide, wide[:, 0].contiguous(), wide[:, 0].contiguous(), wp, None, out, stats)
    with pytest.raises(AssertionError):
        ops.afm_attn_bwd(out, rec, F, D, W1, b1, w2, wp, stats, torch.zeros(B, F * D + 1, device=DEV), grads, ws)
    with pytest.raises(AssertionError):
        ops.afm_attn_bwd(out, rec, F, D, W1, b1, w2, wp, stats, torch.zeros_like(rec), grads[:-1], ws)
    with pytest.raises(AssertionError):
        ops.afm_attn_bwd(out, rec, F, D, W1, b1, w2, wp, stats, torch.zeros_like(rec), grads, ws[:8])
    with pytest.raises(FxError, match="GPU"):
        ops.afm_attn_fwd(rec.cpu(), F, D, W1.cpu(), b1.cpu(), w2.cpu(), wp.cpu(), None, out.cpu(), stats.cpu())
    with pytest.raises(FxError, match="GPU"):
        ops.afm_attn_bwd(out.cpu(), rec.cpu(), F, D, W1.cpu(), b1.cpu(), w2.cpu(), wp.cpu(), stats.cpu(),
                         torch.zeros(B, F * D), grads.cpu(), ws.cpu())
    torch.cuda.synchronize()
