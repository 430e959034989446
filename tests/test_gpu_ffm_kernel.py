"""The field-aware interaction kernels (csrc/fx_ffm.hip) alone, through fuxictr_amd.ops, on a real MI355X against the
same composition in fp64 torch on the CPU (layers.field_aware_composition and torch autograd of it).

The yardstick is that of tests/test_gpu_layernorm.py (`compare`, `f32_exact`): with e32 the error of the composition in
fp32 torch on the CPU, per output tensor, |hip - ref64| <= 4 * e32 + 1e-6 * max|ref|; every case prints err / bound.
The inputs are fp32 numbers of O(1); no element is left out.  The record and dX are the columns [off, off + F*C*D) of
wider rows with `tail` more columns behind, sentinels outside: (0, 0) packed (the 16-byte arm when F*C*D % 4 == 0),
off 4 the 16-byte arm through a stride, off 1 / tail 3 a base / a stride that only the 4-byte arm can take."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from fuxictr_amd.layers import field_aware_composition  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402

DEV = "cuda:0"
LIM = ops.ffm_limits()
SHAPES = [(mode, F, D) for mode in ("onn", "ffm") for F in (2, 3, 9) for D in (1, 2, 4, 6, 10)]
LAYOUTS = [(0, 0), (4, 0), (1, 0), (0, 3), (1, 3)]


def draw_once(mode, B, F, D, seed):
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s):
        return f32_exact(torch.randn(*s, generator=gen, dtype=torch.float64))
    return dict(x=rnd(B, F, ops.ffm_slots(mode, F) * D), add=rnd(B, 1), g=rnd(B, ops.ffm_out_floats(mode, F, D)))


def draw(mode, B, F, D, seed):
    """Inputs from the first of 8 consecutive seeds whose fp64 reference is no cancellation residue.  "ffm" `out` is one
    bare sum per sample: where max |out| is a small fraction of the terms' absolute sum and torch's fp32 sum happens to
    be exact (e32 = 0), the floor 1e-6 |ref| lies below one rounding of ANY fp32 partial sum.  The condition is on the
    reference alone (as in tests/test_gpu_pairfm_kernel.py): max_b |out_b| >= 0.05 max_b (sum of |terms|)."""
    for s in range(seed, seed + 8):
        inp = draw_once(mode, B, F, D, s)
        if mode == "onn":
            return inp
        E = inp["x"].reshape(B, F, F - 1, D)
        i, j = torch.triu_indices(F, F, offset=1)
        mass = (E[:, i, j - 1, :] * E[:, j, i, :]).abs().sum(dim=(1, 2)) + inp["add"].abs().reshape(-1)
        out = field_aware_composition(inp["x"], F, D, mode, inp["add"])
        if float(out.abs().max()) >= 0.05 * float(mass.max()):
            return inp
    raise AssertionError("no seed in [%d, %d) keeps max |out| >= 0.05 max sum |terms|" % (seed, seed + 8))


def run_torch(inp, mode, F, D, dtype):
    x, add = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("x", "add"))
    out = field_aware_composition(x, F, D, mode, add if mode == "ffm" else None)
    dx, = torch.autograd.grad(out, [x], inp["g"].to(dtype))
    return {"out": out.detach().double(), "dX": dx.reshape(dx.shape[0], -1).double()}


def run_hip(inp, mode, F, D, off=0, tail=0):
    B, N = inp["x"].shape[0], inp["x"][0].numel()
    W = ops.ffm_out_floats(mode, F, D)
    recw = torch.full((B, off + N + tail), 7.0, dtype=torch.float32, device=DEV)
    rec = recw[:, off:off + N]
    rec.copy_(inp["x"].reshape(B, N).float())
    dxw = torch.full((B, off + N + tail), 3.0, dtype=torch.float32, device=DEV)
    dX = dxw[:, off:off + N]
    outw = torch.full((B, W + tail), 5.0, dtype=torch.float32, device=DEV)
    out = outw[:, :W]
    add, g = (inp[k].float().to(DEV).contiguous() for k in ("add", "g"))
    ops.ffm_fwd(rec, F, D, mode, add if mode == "ffm" else None, out)
    ops.ffm_bwd(g, rec, F, D, mode, dX)
    torch.cuda.synchronize()
    for buf, fill in ((recw, 7.0), (dxw, 3.0)):          # nobody's columns
        assert bool((buf[:, :off] == fill).all()) and bool((buf[:, off + N:] == fill).all())
    assert bool((outw[:, W:] == 5.0).all())
    assert torch.equal(rec.cpu(), inp["x"].reshape(B, N).float())          # the inputs are read only
    assert torch.equal(add.cpu(), inp["add"].float()) and torch.equal(g.cpu(), inp["g"].float())
    return {"out": out.contiguous(), "dX": dX.contiguous()}


def check(tag, inp, mode, F, D, layouts=((0, 0),), twice=False):
    ref, f32 = run_torch(inp, mode, F, D, torch.float64), run_torch(inp, mode, F, D, torch.float32)
    for off, tail in layouts:
        got = run_hip(inp, mode, F, D, off, tail)
        compare("%s off %d tail %d" % (tag, off, tail), got, ref, f32)
        if twice:
            again = run_hip(inp, mode, F, D, off, tail)              # the same inputs: the same bits
            assert all(torch.equal(got[k], again[k]) for k in got), tag
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-F%d-D%d" % s)
def test_forward_and_gradient_within_the_fp32_yardstick(shape):
    """B one sample, one below, at and above a workgroup's tile, and two tiles and three; at the largest B every layout,
    each run twice."""
    mode, F, D = shape
    T = ops.ffm_tile_rows(mode, F, D)
    assert 2 <= T <= LIM["tile_samples"]
    sizes = sorted({1, T - 1, T, T + 1, 2 * T + 3})
    for B in sizes:
        last = B == sizes[-1]
        check("ffm %s B %d" % (shape, B), draw(mode, B, F, D, seed=1000 * B + 100 * F + D), mode, F, D,
              LAYOUTS if last else LAYOUTS[:1], twice=last)


def test_slot_and_pair_order():
    """"onn", g one-hot on the first pair, a middle one and the last: dX is non-zero at [i][j] and [j][i] only, (i, j)
    from a plain double loop; one-hot on a diagonal column: [i][i] only.  "ffm" (one g for every pair): every slot of
    every field is written, and the values are held to the reference, which spells the j - 1 / j rule out."""
    B, F, D = 3, 7, 2
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]

    def touched(mode, g):
        inp = draw_once(mode, B, F, D, seed=5)
        inp["x"] = inp["x"].abs() + 1.0             # no zero in the record
        inp["g"] = g
        dX = check("ffm %s one-hot" % mode, inp, mode, F, D)["dX"].reshape(B, F, ops.ffm_slots(mode, F), D).cpu()
        return sorted({(i, c, d) for _, i, c, d in dX.nonzero().tolist()})
    for p in (0, len(pairs) // 2, len(pairs) - 1):
        i, j = pairs[p]
        g = torch.zeros(B, F * D + len(pairs), dtype=torch.float64)
        g[:, F * D + p] = 1.0
        assert touched("onn", g) == sorted([(i, j, d) for d in range(D)] + [(j, i, d) for d in range(D)]), p
    g = torch.zeros(B, F * D + len(pairs), dtype=torch.float64)
    g[:, 4 * D + 1] = 1.0
    assert touched("onn", g) == [(4, 4, 1)]
    every = [(i, c, d) for i in range(F) for c in range(F - 1) for d in range(D)]
    assert touched("ffm", torch.ones(B, 1, dtype=torch.float64)) == every


@pytest.mark.parametrize("shape", [("onn", 39, 2), ("onn", 39, 4), ("ffm", 39, 4)], ids=lambda s: "%s-F%d-D%d" % s)
def test_the_criteo_shapes_with_a_wrapped_grid(shape):
    """More tiles than a launch has workgroups: the grid stride wraps."""
    mode, F, D = shape
    B = LIM["workgroups"] * ops.ffm_tile_rows(mode, F, D) + 5
    check("ffm %s criteo B %d" % (shape, B), draw(mode, B, F, D, seed=9), mode, F, D)


def test_the_widest_shape_takes_the_smallest_tile():
    mode, F, D = "onn", 64, 4                      # C * D = 256
    T = ops.ffm_tile_rows(mode, F, D)
    assert 1 <= T <= 2
    check("ffm widest", draw(mode, 2 * T + 3, F, D, seed=13), mode, F, D)


def test_a_shape_outside_the_limits_is_refused_and_launches_nothing():
    from fuxictr_amd._lib import FxError
    B = 4
    for mode, F, D in (("onn", 5, 52), ("ffm", 6, 52), ("onn", 65, 1), ("ffm", 65, 1)):
        C = ops.ffm_slots(mode, F)
        assert (C * D == 260 or F == 65) and not ops.ffm_in_envelope(mode, F, D) and ops.ffm_tile_rows(mode, F, D) == 0
        rec = torch.ones(B, F * C * D, device=DEV)
        out = torch.full((B, ops.ffm_out_floats(mode, F, D)), 5.0, device=DEV)
        dX = torch.full((B, F * C * D), 3.0, device=DEV)
        with pytest.raises(FxError, match="limit"):
            ops.ffm_fwd(rec, F, D, mode, None, out)
        with pytest.raises(FxError, match="limit"):
            ops.ffm_bwd(out, rec, F, D, mode, dX)
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()) and bool((dX == 3.0).all())
    rec = torch.zeros(B, 3 * 2 * 4, device=DEV)
    with pytest.raises(AssertionError):
        ops.ffm_fwd(rec, 3, 4, "onn", None, torch.zeros(B, 15, device=DEV))          # an "ffm" record
    with pytest.raises(AssertionError):
        ops.ffm_fwd(rec, 3, 4, "ffm", None, torch.zeros(B, 2, device=DEV))
    with pytest.raises(AssertionError):
        ops.ffm_bwd(torch.zeros(B, 1, device=DEV), rec, 3, 4, "ffm", torch.zeros(B, 20, device=DEV))
    with pytest.raises(FxError, match="GPU"):
        ops.ffm_fwd(rec.cpu(), 3, 4, "ffm", None, torch.zeros(B, 1))
    torch.cuda.synchronize()
