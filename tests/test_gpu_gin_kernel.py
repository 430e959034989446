"""AOANet's fused generalized-interaction stack (csrc/fx_gin.hip) alone, through fuxictr_amd.ops, on a real MI355X
against the reference's formula in plain torch (tests/test_aoanet_host.py:gin_reference, which forms the
[B, S * F, D, D] tensor) under fp64 autograd: every layer's saved output (the last is the result), dB_0 and dW, dalpha,
dh of every layer.

Yardstick (that of tests/test_gpu_euler_kernel.py): per compared tensor e32 = max |the same arithmetic in fp32 torch on
the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  Every case prints its observed err / bound.
Outputs and workspace are pre-filled with NaN and every element is compared.  Inputs are drawn in fp32 and widened.
W = randn / sqrt(D) (not symmetric: a transposed W cannot pass), alpha = randn / sqrt(S F), h = randn, all different in
every layer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_aoanet_host import gin_reference  # noqa: E402
from test_gpu_euler_kernel import compare  # noqa: E402

GRID = "grid"        # B = workgroups x samples per tile + 3: the grid stride wraps, every partial row is live (gin_limits)
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 1, 2, 2), (7, 5, 6, 3, 3), (33, 39, 10, 4, 3), (4, 39, 40, 4, 3), (9, 64, 4, 8, 2),
          (5, 3, 64, 4, 2), (3, 17, 17, 5, 1), (GRID, 4, 4, 4, 3)]


def make_inputs(shape, seed):
    B, F, D, O, L = shape
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)    # noqa: E731
    t = {"B0": rnd(B, F, D), "dout": rnd(B, O, D), "dB0_0": rnd(B, F, D)}
    for l in range(L):
        S = O if l else F
        t.update({"W%d" % l: rnd(O, D, D) / D ** 0.5, "alpha%d" % l: rnd(S * F, O) / (S * F) ** 0.5, "h%d" % l: rnd(O, D, 1)})
    return {k: v.double() for k, v in t.items()}


def run_torch(t, L, dtype, accumulate):
    names = ["B0"] + [k + str(l) for l in range(L) for k in ("W", "alpha", "h")]
    v = {k: t[k].to(dtype).clone().requires_grad_(True) for k in names}
    outs = gin_reference(v["B0"], [tuple(v[k + str(l)] for k in ("W", "alpha", "h")) for l in range(L)])
    grads = torch.autograd.grad(outs[-1], [v[k] for k in names], t["dout"].to(dtype))
    res = {"outs": torch.stack(outs).detach()}
    res.update(("d" + k, g) for k, g in zip(names, grads))
    if accumulate:
        res["dB0"] = res["dB0"] + t["dB0_0"].to(dtype)
    return {k: x.double() for k, x in res.items()}


def run_hip(t, shape, pad=0):
    """pad > 0: B_0 and dB_0 are the first F fields of records of F + pad; dB_0 is added to what the view holds."""
    dev = torch.device("cuda:0")
    B, F, D, O, L = shape
    full = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)    # noqa: E731
    rec, drec = torch.full((B, F + pad, D), 7.0, dtype=torch.float32, device=dev), full(B, F + pad, D)
    B0, dB0 = rec[:, :F, :], drec[:, :F, :]
    B0.copy_(t["B0"])
    if pad:
        dB0.copy_(t["dB0_0"])
    names = [k + str(l) for l in range(L) for k in ("W", "alpha", "h")]
    params = torch.cat([t[k].float().reshape(-1) for k in names]).to(dev)
    outs, dparams, ws = full(L, B, O, D), full(params.numel()), full(ops.gin_workspace_floats(B, F, D, O, L))
    ops.gin_fwd(B0, O, L, params, outs)
    ops.gin_bwd(t["dout"].float().to(dev), B0, O, L, params, outs, dB0, dparams, ws, dx_accumulate=bool(pad))
    torch.cuda.synchronize()
    if pad:                                  # the slots behind the fields are nobody's to write
        assert bool((rec[:, F:, :] == 7.0).all()) and bool(torch.isnan(drec[:, F:, :]).all())
    got = {"outs": outs, "dB0": dB0.contiguous()}
    got.update(("d" + k, g) for k, g in zip(names, dparams.split([t[k].numel() for k in names])))
    return got


@pytest.mark.parametrize("shape,pad", [(s, 0) for s in SHAPES] + [((7, 5, 6, 3, 3), 2)],
                         ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else "pad%d" % v)
def test_stack_and_gradients_within_the_fp32_yardstick(shape, pad):
    if shape[0] == GRID:
        lim = ops.gin_limits()
        shape = (lim["workgroups"] * lim["tile_samples"] + 3,) + shape[1:]
    t = make_inputs(shape, seed=sum(shape))
    ref, f32 = (run_torch(t, shape[4], dt, bool(pad)) for dt in (torch.float64, torch.float32))
    worst = compare("gin %s pad=%d" % (shape, pad), ref, f32, run_hip(t, shape, pad))
    print("gin %s pad=%d largest err / bound %.3f" % (shape, pad, worst))
