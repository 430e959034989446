"""SAM's fused SAM2A / SAM2E block-and-head kernels (csrc/fx_sam.hip) alone, through fuxictr_amd.ops, on a real MI355X
against the formula in plain torch (tests/test_sam_host.py:sam_reference, which forms the [B, F, F, D] tensor) under
fp64 autograd: logit, dX, dw, dbias and, for SAM2A, dW; and one SAM3A / SAM3E layer (sam_layer_reference), with and
without the residual: out, dX, dK, dQ and, for SAM3A, dW.  K and Q are randn / sqrt(D): a transposed K cannot pass.

Yardstick (that of tests/test_gpu_euler_kernel.py): per compared tensor e32 = max |the same arithmetic in fp32 torch on
the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  Every case prints its observed err / bound.
Outputs and workspace are pre-filled with NaN and every element is compared.  Inputs are drawn in fp32 and widened.
W = 1 + 0.1 randn, and w is a plain randn, so w[n, m, :] != w[m, n, :]: a kernel that uses the symmetry of S must still
keep the two triangles of W and w apart."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_gpu_euler_kernel import compare  # noqa: E402
from test_sam_host import sam_layer_reference, sam_reference  # noqa: E402

GRID = "grid"        # B = workgroups x samples per tile + 3: the grid stride wraps, dW has all its slabs (sam_limits)
SHAPES = [(1, 1, 1), (2, 3, 1), (7, 5, 6), (33, 39, 10), (9, 64, 4), (5, 3, 64), (3, 17, 17), (GRID, 4, 4)]
LEAVES = ["X", "w", "bias", "W"]


def make_inputs(shape, seed):
    B, F, D = shape
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)    # noqa: E731
    t = {"X": rnd(B, F, D), "w": rnd(F, F, D) / (F * D ** 0.5), "bias": rnd(1), "W": 1 + 0.1 * rnd(F, F, D),
         "dlogit": rnd(B), "dX0": rnd(B, F, D), "K": rnd(D, D) / D ** 0.5, "Q": rnd(D, D) / D ** 0.5,
         "dout": rnd(B, F, D)}
    return {k: v.double() for k, v in t.items()}


def run_torch(t, kind, dtype, accumulate):
    leaves = [t[k].to(dtype).clone().requires_grad_(True) for k in LEAVES[:4 if kind == "SAM2A" else 3]]
    logit = sam_reference(kind, leaves[0], leaves[3] if kind == "SAM2A" else None, *leaves[1:3])
    grads = torch.autograd.grad(logit, leaves, t["dlogit"].to(dtype))
    out = {"logit": logit.detach()}
    out.update(("d" + k, g) for k, g in zip(LEAVES, grads))
    if accumulate:
        out["dX"] = out["dX"] + t["dX0"].to(dtype)
    return {k: v.double() for k, v in out.items()}


def run_hip(t, kind, pad=0):
    """pad > 0: X and dX are the first F fields of records of F + pad; dX is added to what the view holds."""
    dev = torch.device("cuda:0")
    B, F, D = t["X"].shape
    full = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)    # noqa: E731
    rec, drec = torch.full((B, F + pad, D), 7.0, dtype=torch.float32, device=dev), full(B, F + pad, D)
    X, dX = rec[:, :F, :], drec[:, :F, :]
    X.copy_(t["X"])
    if pad:
        dX.copy_(t["dX0"])
    w, bias, dlogit = (t[k].float().to(dev) for k in ("w", "bias", "dlogit"))
    W = t["W"].float().to(dev) if kind == "SAM2A" else None
    logit, dw, dbias, ws = full(B), full(F, F, D), full(1), full(ops.sam_workspace_floats(B, F, D, kind))
    dW = full(F, F, D) if kind == "SAM2A" else None
    ops.sam_logit_fwd(X, kind, W, w, bias, logit, ws)
    ws.fill_(float("nan"))
    ops.sam_logit_bwd(X, kind, W, w, dlogit, dX, dW, dw, dbias, ws, dx_accumulate=bool(pad))
    torch.cuda.synchronize()
    if pad:                                  # the slots behind the fields are nobody's to write
        assert bool((rec[:, F:, :] == 7.0).all()) and bool(torch.isnan(drec[:, F:, :]).all())
    out = {"logit": logit, "dX": dX.contiguous(), "dw": dw, "dbias": dbias}
    if kind == "SAM2A":
        out["dW"] = dW
    return out


@pytest.mark.parametrize("kind", ["SAM2A", "SAM2E"])
@pytest.mark.parametrize("shape,pad", [(s, 0) for s in SHAPES] + [((7, 5, 6), 2)],
                         ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else "pad%d" % v)
def test_logit_and_gradients_within_the_fp32_yardstick(shape, pad, kind):
    if shape[0] == GRID:
        lim = ops.sam_limits()
        shape = (lim["workgroups"] * lim["tile_samples"] + 3,) + shape[1:]
    t = make_inputs(shape, seed=sum(shape))
    ref, f32 = run_torch(t, kind, torch.float64, bool(pad)), run_torch(t, kind, torch.float32, bool(pad))
    compare("sam %s %s pad=%d" % (kind, shape, pad), ref, f32, run_hip(t, kind, pad))


def run_torch_layer(t, kind, res, dtype, accumulate):
    names = ["X", "K"] + (["Q"] if res else []) + (["W"] if kind == "SAM3A" else [])
    v = {k: t[k].to(dtype).clone().requires_grad_(True) for k in names}
    out = sam_layer_reference(kind, v["X"], v["K"], v.get("Q"), v.get("W"))
    grads = torch.autograd.grad(out, [v[k] for k in names], t["dout"].to(dtype))
    res_ = {"out": out.detach()}
    res_.update(("d" + k, g) for k, g in zip(names, grads))
    if accumulate:
        res_["dX"] = res_["dX"] + t["dX0"].to(dtype)
    return {k: x.double() for k, x in res_.items()}


def run_hip_layer(t, kind, res, pad=0):
    dev = torch.device("cuda:0")
    B, F, D = t["X"].shape
    full = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)    # noqa: E731
    rec, drec = torch.full((B, F + pad, D), 7.0, dtype=torch.float32, device=dev), full(B, F + pad, D)
    X, dX = rec[:, :F, :], drec[:, :F, :]
    X.copy_(t["X"])
    if pad:
        dX.copy_(t["dX0"])
    K, dout = t["K"].float().to(dev), t["dout"].float().to(dev)
    Q = t["Q"].float().to(dev) if res else None
    W = t["W"].float().to(dev) if kind == "SAM3A" else None
    out, dK, ws = full(B, F, D), full(D, D), full(ops.sam_workspace_floats(B, F, D, kind))
    dQ, dW = full(D, D) if res else None, full(F, F, D) if kind == "SAM3A" else None
    ops.sam_layer_fwd(X, kind, K, Q, W, out, ws)
    ws.fill_(float("nan"))
    ops.sam_layer_bwd(X, kind, K, Q, W, dout, dX, dK, dQ, dW, ws, dx_accumulate=bool(pad))
    torch.cuda.synchronize()
    if pad:
        assert bool((rec[:, F:, :] == 7.0).all()) and bool(torch.isnan(drec[:, F:, :]).all())
    got = {"out": out, "dX": dX.contiguous(), "dK": dK, "dQ": dQ, "dW": dW}
    return {k: v for k, v in got.items() if v is not None}


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("kind", ["SAM3A", "SAM3E"])
@pytest.mark.parametrize("shape,pad", [(s, 0) for s in SHAPES] + [((7, 5, 6), 2)],
                         ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else "pad%d" % v)
def test_layer_and_gradients_within_the_fp32_yardstick(shape, pad, kind, res):
    if shape[0] == GRID:
        lim = ops.sam_limits()
        shape = (lim["workgroups"] * lim["tile_samples"] + 3,) + shape[1:]
    t = make_inputs(shape, seed=sum(shape))
    ref, f32 = (run_torch_layer(t, kind, res, dt, bool(pad)) for dt in (torch.float64, torch.float32))
    compare("sam %s res=%d %s pad=%d" % (kind, res, shape, pad), ref, f32, run_hip_layer(t, kind, res, pad))
