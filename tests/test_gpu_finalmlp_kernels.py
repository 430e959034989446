"""FinalMLP's kernels (csrc/fx_finalmlp.hip) alone, through fuxictr_amd.ops, on a real MI355X against fp64
torch-autograd restatements written from the formulas (tests/test_finalmlp_host.py):
    gates   F_i = E * 2 sigmoid(Z_i),  Z_i [B, W] or one row for all samples
    head    out[b] = b_x + b_y + X[b] . w_x + Y[b] . (w_y + T[b]) (+ out_add[b]),  T[:, h] = X_h W_h

The tolerance is the yardstick of tests/test_gpu_bilinear.py / test_gpu_layernorm.py: the same formulas in fp32
torch on the CPU have an error e32 against the fp64 result, per output tensor (max |.|); the HIP result must lie
within
    4 * e32 + 1e-6 * max|ref|.
Every case prints its observed ratio err / bound.  The inputs are fp32 numbers, so all three computations start from
the same values.  No element is left out of any comparison.  Where a gradient is ADDED to a buffer that holds 3.0
and the 3.0 is taken off again here, that round trip's one rounding (2^-22 max(1, |.|)) is allowed for, as
test_gpu_layernorm.py does.

The head is run as its callers run it: the per-head products through ops.gemm_batch on column slices, then the
kernels (layers._AggregationFn)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import layers, ops  # noqa: E402
from test_finalmlp_host import gate_reference, head_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402

DEV = "cuda:0"
SLAB = ops.finalmlp_slab_rows(64)          # rows of one slab of the backward's batch sums at these sizes

GATE_SHAPES = [(1, 1), (3, 3), (5, 4), (7, 5), (33, 65), (65, 624), (2, 4100)]
# one below, at and one above a slab, and two slabs: the scalar and the 16-byte arm
GATE_SHAPES += [(r, w) for r in (SLAB - 1, SLAB, SLAB + 1, 2 * SLAB) for w in (6, 8)]
# a broadcast gate's dZ is a row sum over the slabs, 2 W columns and 64 of them per workgroup of four waves: four and
# nine slabs (the shapes above have 1, 2, 3 and 5), 62, 64 and 66 columns
GATE_SHAPES += [(SLAB + 1, 31), (3 * SLAB + 1, 32), (8 * SLAB + 1, 33)]
# gate 1 / gate 2: b = one broadcast row, p = per sample, - = no second gate
GATE_MODES = ["bb", "bp", "pb", "pp", "b-", "p-"]


def gate_inputs(shape, mode, seed, saturate=False):
    B, W = shape
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s):
        return f32_exact(torch.randn(*s, generator=gen, dtype=torch.float64))
    E = rnd(B, W)
    Z = [rnd(1 if m == "b" else B, W) for m in mode if m != "-"]
    if saturate:                            # the sigmoid's two saturated tails
        for z in Z:
            flat = z.view(-1)
            flat[::3] = 30.0
            flat[1::5] = -30.0
    dF = [rnd(B, W) for _ in Z]
    return E, Z, dF


def gate_torch(E, Z, dF, dtype):
    e = E.to(dtype).clone().requires_grad_(True)
    zs = [z.to(dtype).clone().requires_grad_(True) for z in Z]
    fs = [gate_reference(e, z) for z in zs]
    grads = torch.autograd.grad(fs, [e] + zs, [d.to(dtype) for d in dF])
    out = {"dE": grads[0].double()}
    for i, f in enumerate(fs):
        out["F%d" % (i + 1)] = f.detach().double()
        out["dZ%d" % (i + 1)] = grads[1 + i].double()
    return out


def gate_hip(E, Z, dF, off=0, tail=0, accumulate=False):
    """E, F, dF and dE as the columns [off, off + W) of rows with off + W + tail floats (sentinels elsewhere);
    accumulate: dE is ADDED to the buffer's 3.0, taken off again here."""
    B, W = E.shape

    def wide(fill):
        return torch.full((B, off + W + tail), fill, dtype=torch.float32, device=DEV)

    def cols(t):
        return t[:, off:off + W]
    ebuf, bufs = wide(7.0), []
    cols(ebuf).copy_(E.float())
    zs = [z.float().to(DEV).contiguous() for z in Z]
    two = len(zs) == 2
    fb = [wide(5.0) for _ in zs]
    ops.gate2_fwd(cols(ebuf), zs[0], zs[1] if two else None, cols(fb[0]), cols(fb[1]) if two else None)
    torch.cuda.synchronize()
    gb = [wide(9.0) for _ in zs]
    for gbuf, d in zip(gb, dF):
        cols(gbuf).copy_(d.float())
    debuf = wide(3.0)
    dz = [torch.empty_like(z) for z in zs]
    ws = torch.empty(max(1, ops.gate2_workspace_floats(B, W)), dtype=torch.float32, device=DEV)
    ops.gate2_bwd(cols(gb[0]), cols(gb[1]) if two else None, cols(ebuf), zs[0], zs[1] if two else None, cols(debuf),
                  dz[0], dz[1] if two else None, ws, de_accumulate=accumulate)
    torch.cuda.synchronize()
    for t, fill in [(ebuf, 7.0), (debuf, 3.0)] + [(f, 5.0) for f in fb] + [(gq, 9.0) for gq in gb]:
        assert bool((t[:, :off] == fill).all()) and bool((t[:, off + W:] == fill).all())       # nobody's columns
    out = {"dE": cols(debuf) - 3.0 if accumulate else cols(debuf).contiguous()}
    for i in range(len(zs)):
        out["F%d" % (i + 1)] = cols(fb[i]).contiguous()
        out["dZ%d" % (i + 1)] = dz[i]
    return out


def gate_check(tag, E, Z, dF, **layout):
    got = gate_hip(E, Z, dF, **layout)
    ref, f32 = gate_torch(E, Z, dF, torch.float64), gate_torch(E, Z, dF, torch.float32)
    extra = None
    if layout.get("accumulate"):        # (3 + dE) - 3 in fp32: one rounding at magnitude <= 4 max(1, |dE|)
        extra = {"dE": 2.0 ** -22 * max(1.0, float(ref["dE"].abs().max()))}
    compare(tag, got, ref, f32, extra=extra)
    return got


@pytest.mark.parametrize("mode", GATE_MODES)
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "B%d-W%d" % s)
def test_gates_forward_and_gradients_within_the_fp32_yardstick(shape, mode):
    E, Z, dF = gate_inputs(shape, mode, seed=29 + 3 * shape[0] + shape[1] + GATE_MODES.index(mode))
    tag = "gate2 %s %s" % (shape, mode)
    first = gate_check(tag, E, Z, dF)
    again = gate_hip(E, Z, dF)                                          # the same inputs: the same bits
    for name in first:
        assert torch.equal(first[name], again[name]), name
    # inside wider rows: at an aligned column offset with dE added to the buffer, and at an unaligned one (a row
    # stride that is no multiple of 4 and a base that is only 4-byte aligned: the scalar arm whatever W is)
    gate_check(tag + " in place", E, Z, dF, off=8, tail=4, accumulate=True)
    gate_check(tag + " unaligned", E, Z, dF, off=3, tail=2, accumulate=True)
    gate_check(tag + " unaligned write", E, Z, dF, off=1, tail=0, accumulate=False)


@pytest.mark.parametrize("mode", GATE_MODES)
@pytest.mark.parametrize("shape", [(7, 5), (33, 65), (2 * SLAB + 1, 8)], ids=lambda s: "B%d-W%d" % s)
def test_saturated_gates_stay_finite_and_within_the_yardstick(shape, mode):
    """Z = +-30: 2 sigmoid is 2 or 1.9e-13 and sigmoid (1 - sigmoid) is 9.4e-14; compare() asserts finiteness."""
    E, Z, dF = gate_inputs(shape, mode, seed=5 + shape[0], saturate=True)
    got = gate_check("gate2 saturated %s %s" % (shape, mode), E, Z, dF)
    z0 = Z[0].expand(shape[0], shape[1])
    f1 = got["F1"].cpu()
    assert torch.equal(f1[z0 == 30.0], (2.0 * E.float())[z0 == 30.0])
    assert bool((f1[z0 == -30.0].abs() <= 1e-12 * E.float()[z0 == -30.0].abs()).all())


# ---- the aggregation head -----------------------------------------------------------------------------------
#               B  dx  dy  H
HEAD_SHAPES = [(1, 1, 1, 1), (3, 2, 3, 1), (5, 4, 4, 2), (33, 6, 10, 2), (65, 64, 64, 4), (9, 512, 256, 2),
               (4, 3, 5, 1)]
# lanes per row switch at 4 | 5 and 16 | 17 chunks, a lane starts a second round beyond 64 chunks: widths one below,
# at and one above, chunks of one float (odd widths, the scalar arm) and of four (the 16-byte arm)
HEAD_SHAPES += [(5, w, w, 1) for w in (15, 17, 63, 65)] + [(5, 3, 5, 1), (5, 16, 13, 1), (5, 64, 7, 1)]
HEAD_SHAPES += [(5, w, w, 1) for w in (12, 16, 20, 60, 64, 68, 252, 256, 260)]
# row counts around a slab of the backward's batch sums
HEAD_SHAPES += [(r, 8, 12, 2) for r in (SLAB - 1, SLAB, SLAB + 1, 2 * SLAB)]
# dw_x | dw_y | db: a row sum over the slabs of dx + dy + 1 columns, 64 per workgroup of four waves: 63, 64 and 65
# columns (db the last of a workgroup, alone in the next), four and nine slabs (the shapes above have 1, 2, 3 and 5)
HEAD_SHAPES += [(5, 31, 31, 1), (3 * SLAB + 1, 31, 32, 1), (8 * SLAB + 1, 32, 32, 2)]
HEAD_NAMES = ["out", "dX", "dY", "dw_x", "dw_y", "db_x", "db_y", "dw_xy", "dadd"]


def head_inputs(shape, seed):
    B, dx, dy, H = shape
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s, scale=1.0):
        return f32_exact(scale * torch.randn(*s, generator=gen, dtype=torch.float64))
    return dict(X=rnd(B, dx), Y=rnd(B, dy), w_x=rnd(1, dx), b_x=rnd(1), w_y=rnd(1, dy), b_y=rnd(1),
                w_xy=rnd(dx * dy // H, 1, scale=0.5), add=rnd(B, 1), g=rnd(B, 1))


def head_torch(inp, H, with_add, dtype):
    t = {k: v.to(dtype).clone().requires_grad_(k != "g") for k, v in inp.items()}
    out = head_reference(t["X"], t["Y"], t["w_x"], t["b_x"], t["w_y"], t["b_y"], t["w_xy"], H,
                         t["add"] if with_add else None)
    wrt = ["X", "Y", "w_x", "w_y", "b_x", "b_y", "w_xy"] + (["add"] if with_add else [])
    grads = torch.autograd.grad(out, [t[k] for k in wrt], t["g"])
    res = {"out": out.detach().double()}
    for k, gr in zip(wrt, grads):
        res["d" + k] = gr.double()
    return res


def head_hip(inp, H, with_add, off=0, tail=0):
    """X and Y as the columns [off, off + d) of wider buffers (7.0 elsewhere; their gradients arrive in the wide
    buffers through autograd's own slice: zero outside the columns)."""
    B, dx = inp["X"].shape
    dy = inp["Y"].shape[1]
    xw = torch.full((B, off + dx + tail), 7.0, dtype=torch.float32, device=DEV)
    yw = torch.full((B, off + dy + tail), 7.0, dtype=torch.float32, device=DEV)
    xw[:, off:off + dx] = inp["X"].float().to(DEV)
    yw[:, off:off + dy] = inp["Y"].float().to(DEV)
    xw.requires_grad_(True), yw.requires_grad_(True)
    p = {k: inp[k].float().to(DEV).requires_grad_(True) for k in ("w_x", "b_x", "w_y", "b_y", "w_xy", "add")}
    x, y = xw[:, off:off + dx], yw[:, off:off + dy]
    out = layers._AggregationFn.apply(x, y, p["add"] if with_add else None, H, p["w_x"], p["b_x"], p["w_y"],
                                      p["b_y"], p["w_xy"])
    wrt = [xw, yw, p["w_x"], p["w_y"], p["b_x"], p["b_y"], p["w_xy"]] + ([p["add"]] if with_add else [])
    grads = torch.autograd.grad(out, wrt, inp["g"].float().to(DEV))
    torch.cuda.synchronize()
    for gw, d in ((grads[0], dx), (grads[1], dy)):
        assert not bool(gw[:, :off].any()) and not bool(gw[:, off + d:].any())
    res = {"out": out.detach(), "dX": grads[0][:, off:off + dx].contiguous(),
           "dY": grads[1][:, off:off + dy].contiguous()}
    for k, gr in zip(["w_x", "w_y", "b_x", "b_y", "w_xy"] + (["add"] if with_add else []), grads[2:]):
        res["d" + k] = gr.contiguous()
    return res


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "out_add"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "B%d-dx%d-dy%d-H%d" % s)
def test_head_forward_and_gradients_within_the_fp32_yardstick(shape, with_add):
    B, dx, dy, H = shape
    inp = head_inputs(shape, seed=31 + B + 3 * dx + 5 * dy + H + with_add)
    ref, f32 = head_torch(inp, H, with_add, torch.float64), head_torch(inp, H, with_add, torch.float32)
    assert sorted(ref) == sorted(n for n in HEAD_NAMES if with_add or n != "dadd")
    tag = "biagg %s %s" % (shape, "out_add" if with_add else "plain")
    first = head_hip(inp, H, with_add)
    compare(tag, first, ref, f32)
    again = head_hip(inp, H, with_add)                                  # the same inputs: the same bits
    for name in first:
        assert torch.equal(first[name], again[name]), name
    assert torch.equal(first["db_x"], first["db_y"])
    # X and Y as column slices of wider buffers: at an aligned offset, and at an unaligned one (the scalar arm)
    compare(tag + " sliced", head_hip(inp, H, with_add, off=4, tail=4), ref, f32)
    compare(tag + " unaligned", head_hip(inp, H, with_add, off=3, tail=2), ref, f32)


def test_bad_arguments_are_rejected_before_the_launch():
    from fuxictr_amd._lib import FxError
    e = torch.zeros(4, 8, device=DEV)
    with pytest.raises(AssertionError):
        ops.gate2_fwd(e, torch.zeros(3, 8, device=DEV), None, torch.empty_like(e), None)
    with pytest.raises(FxError, match="GPU"):
        ops.gate2_fwd(e.cpu(), torch.zeros(1, 8), None, torch.empty(4, 8), None)
    with pytest.raises(NotImplementedError, match="output_dim=3"):
        layers.InteractionAggregation(8, 8, output_dim=3)
    torch.cuda.synchronize()
