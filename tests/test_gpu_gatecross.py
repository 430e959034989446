"""GDCN's kernels (csrc/fx_gatecross.hip) alone, through fuxictr_amd.ops, on a real MI355X against fp64
torch-autograd restatements written from the formulas (tests/test_gdcn_host.py):
    forward   xn = x0 * (u0 + b) * sigmoid(v) + xi,   h = [u0 | v]
    backward  dh = [dxn x0 g | dxn x0 u g (1 - g)],  dx0 (= | +=) dxn u g (+ dxn),   u = u0 + b, g = sigmoid(v)

The tolerance is the yardstick of tests/test_gpu_layernorm.py (`compare`, `f32_exact`): the same formulas in fp32
torch on the CPU have an error e32 against the fp64 result, per output tensor (max |.|); the HIP result must lie
within
    4 * e32 + 1e-6 * max|ref|.
Every case prints its observed ratio err / bound.  The inputs are fp32 numbers, so all three computations start from
the same values.  No element is left out of any comparison.  Where dx0 is ADDED to a buffer that holds 3.0 and the
3.0 is taken off again here, that round trip's one rounding (2^-22 max(1, |.|)) is allowed for, as
test_gpu_layernorm.py / test_gpu_finalmlp_kernels.py do.

Every matrix (and b) is handed over as the columns [off, off + width) of wider rows with `tail` more columns behind
them, sentinels outside: off 0 / tail 0 is the packed case (the 16-byte arm when cols % 4 == 0), off 4 the 16-byte
arm through row strides, off 1 a base that is only 4-byte aligned and tail 3 a row stride that is no multiple of 4
(the scalar arm whatever cols is)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_gdcn_host import gate_cross_fwd_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402

DEV = "cuda:0"
TILE = ops.gate_cross_tile_rows()          # rows of one workgroup's tile

SHAPES = [(1, 1), (3, 3), (5, 4), (7, 5), (33, 65), (65, 624), (2, 4100)]
# one row below, at and above a workgroup's tile of rows, and two tiles: the scalar and the 16-byte arm
SHAPES += [(r, c) for r in (TILE - 1, TILE, TILE + 1, 2 * TILE) for c in (6, 8)]
LAYOUTS = [(off, tail) for off in (0, 1, 4) for tail in (0, 3)]
FLAGS = [(init, add_dxn) for init in (True, False) for add_dxn in (True, False)]


def make_inputs(shape, seed, saturate=False):
    rows, cols = shape
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s):
        return f32_exact(torch.randn(*s, generator=gen, dtype=torch.float64))
    inp = dict(h=rnd(rows, 2 * cols), x0=rnd(rows, cols), xi=rnd(rows, cols), b=rnd(cols), dxn=rnd(rows, cols))
    if saturate:                            # the sigmoid's two saturated tails, in a pattern over v
        v = inp["h"][:, cols:].reshape(-1).clone()
        v[0::7], v[1::7], v[2::7], v[3::7] = 30.0, -30.0, 100.0, -100.0
        inp["h"][:, cols:] = v.reshape(rows, cols)
    return inp


def run_torch(inp, dtype):
    """-> xn, dh, and the four dx0 results of the flag pairs (not init: what is added to the buffer)"""
    t = {k: v.to(dtype).clone() for k, v in inp.items()}
    for k in ("h", "x0", "xi"):
        t[k].requires_grad_(True)
    xn = gate_cross_fwd_reference(t["h"], t["x0"], t["xi"], t["b"])
    dh, dx0, dxi = torch.autograd.grad(xn, [t["h"], t["x0"], t["xi"]], t["dxn"])
    out = {"xn": xn.detach().double(), "dh": dh.double()}
    for init, add_dxn in FLAGS:
        # (at layer 0 x_i IS x_0: the residual's gradient, d xn / d xi = dxn, joins dx0)
        out["dx0 %d%d" % (init, add_dxn)] = (dx0 + dxi if add_dxn else dx0).double()
    return out


def run_hip(inp, off=0, tail=0):
    rows, cols = inp["x0"].shape
    held = []

    def wide(width, fill, src=None):
        buf = torch.full((rows, off + width + tail), fill, dtype=torch.float32, device=DEV)
        view = buf[:, off:off + width]
        if src is not None:
            view.copy_(src.float())
        held.append((buf, width, fill))
        return view
    h, x0, xi = wide(2 * cols, 7.0, inp["h"]), wide(cols, 7.5, inp["x0"]), wide(cols, 8.0, inp["xi"])
    dxn = wide(cols, 9.0, inp["dxn"])
    bw = torch.full((off + cols + tail,), 6.0, dtype=torch.float32, device=DEV)
    b = bw[off:off + cols]
    b.copy_(inp["b"].float())
    xn = wide(cols, 5.0)
    ops.gate_cross_fwd(h, x0, xi, b, xn)
    out = {"xn": xn.contiguous()}
    dh = None
    for init, add_dxn in FLAGS:
        dh, dx0 = wide(2 * cols, 4.0), wide(cols, 3.0)
        ops.gate_cross_bwd(dxn, h, x0, b, dh, dx0, init, add_dxn)
        out["dx0 %d%d" % (init, add_dxn)] = dx0.contiguous() if init else dx0 - 3.0
        if "dh" in out:
            assert torch.equal(out["dh"], dh)           # the flags do not touch dh
        out["dh"] = dh.contiguous()
    torch.cuda.synchronize()
    for buf, width, fill in held:                       # nobody's columns
        assert bool((buf[:, :off] == fill).all()) and bool((buf[:, off + width:] == fill).all())
    assert bool((bw[:off] == 6.0).all()) and bool((bw[off + cols:] == 6.0).all())
    # the inputs are read only
    for view, src in ((h, "h"), (x0, "x0"), (xi, "xi"), (dxn, "dxn"), (b, "b")):
        assert torch.equal(view.cpu(), inp[src].float())
    return out


def check(tag, inp, ref, f32, **layout):
    got = run_hip(inp, **layout)
    assert sorted(got) == sorted(ref)
    # (3 + dx0) - 3 in fp32: one rounding at magnitude <= 4 max(1, |dx0|)
    extra = {k: 2.0 ** -22 * max(1.0, float(ref[k].abs().max())) for k in ref if k.startswith("dx0 0")}
    compare(tag, got, ref, f32, extra=extra)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d-c%d" % s)
def test_forward_and_gradients_within_the_fp32_yardstick_in_every_layout(shape):
    inp = make_inputs(shape, seed=41 + 3 * shape[0] + shape[1])
    ref, f32 = run_torch(inp, torch.float64), run_torch(inp, torch.float32)
    for off, tail in LAYOUTS:
        tag = "gate_cross %s off %d tail %d" % (shape, off, tail)
        first = check(tag, inp, ref, f32, off=off, tail=tail)
        if (off, tail) in ((0, 0), (1, 3)):
            again = run_hip(inp, off=off, tail=tail)                    # the same inputs: the same bits
            for name in first:
                assert torch.equal(first[name], again[name]), name


@pytest.mark.parametrize("shape", [(7, 5), (33, 64), (2 * TILE + 1, 8)], ids=lambda s: "r%d-c%d" % s)
def test_saturated_gates_stay_finite_and_within_the_yardstick(shape):
    """v = +-30 and +-100: sigmoid is 1, 9.4e-14, 1, 3.8e-44 and g (1 - g) is 9.4e-14 / 3.8e-44 or 0; compare()
    asserts that every output is finite."""
    rows, cols = shape
    inp = make_inputs(shape, seed=5 + rows, saturate=True)
    ref, f32 = run_torch(inp, torch.float64), run_torch(inp, torch.float32)
    v = inp["h"][:, cols:]
    assert all(bool((v == s).any()) for s in (30.0, -30.0, 100.0, -100.0))
    for off, tail in ((0, 0), (1, 3)):
        got = check("gate_cross saturated %s off %d tail %d" % (shape, off, tail), inp, ref, f32, off=off, tail=tail)
        xn, dh = got["xn"].cpu(), got["dh"].cpu()
        x0, xi, u = inp["x0"].float(), inp["xi"].float(), (inp["h"][:, :cols] + inp["b"]).float()
        for s in (30.0, 100.0):             # an open gate: the plain cross term, and no gradient toward v
            assert torch.allclose(xn[v == s], (x0 * u + xi)[v == s], rtol=1e-6, atol=1e-6)
            assert bool((dh[:, cols:][v == s].abs() <= 1e-12 * (1.0 + u.abs() * x0.abs())[v == s] * 10.0).all())
        for s in (-30.0, -100.0):           # a shut gate: the residual alone
            assert bool(((xn - xi)[v == s].abs() <= (1e-12 * (x0 * u).abs() + 2.0 ** -23 * xi.abs())[v == s]).all())
            assert bool((dh[:, :cols][v == s].abs() <= 1e-12 * (inp["dxn"].float() * x0).abs()[v == s]).all())


def test_bad_arguments_are_rejected_before_the_launch():
    from fuxictr_amd._lib import FxError
    h, x = torch.zeros(4, 16, device=DEV), torch.zeros(4, 8, device=DEV)
    b = torch.zeros(8, device=DEV)
    with pytest.raises(AssertionError):
        ops.gate_cross_fwd(torch.zeros(4, 12, device=DEV), x, x, b, torch.empty_like(x))
    with pytest.raises(AssertionError):
        ops.gate_cross_bwd(x, h, x, b[:4], torch.empty_like(h), torch.empty_like(x), True, False)
    with pytest.raises(FxError, match="GPU"):
        ops.gate_cross_fwd(h.cpu(), x.cpu(), x.cpu(), b.cpu(), torch.empty(4, 8))
    torch.cuda.synchronize()
