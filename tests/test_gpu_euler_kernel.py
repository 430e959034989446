"""EulerNet's Euler interaction and polar kernels (csrc/fx_euler.hip) alone, through fuxictr_amd.ops, on a real MI355X
against the arithmetic in plain torch (tests/test_eulernet_host.py:euler_reference) under fp64 autograd: OP, dZ, the
explicit part of dRP, d inter_orders, d bias_lam, d bias_theta and the four LayerNorm gradients; for the polar pair RP,
dE and dmu.

Yardstick (that of tests/test_gpu_lognet_kernel.py): per compared tensor e32 = max |the same arithmetic in fp32 torch on
the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  Every case prints its observed err / bound.
Outputs and workspace are pre-filled with NaN and every element is compared.  Inputs are drawn in fp32 and widened, so
both sides see the same values; Z is an INPUT with |z| >= 1e-3, so both sides take the same side of the ReLU.
LayerNorm runs where D >= 4: at D = 1 the true gradients through the norm are ~1e-14 against ~1e-5 of fp32 rounding
residue and the yardstick would be noise (D = 2 is nearly as ill-conditioned)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_eulernet_host import euler_reference  # noqa: E402

GRID = "grid"        # B such that the tiles outnumber the workgroups / slabs / chunks of every pass: euler_limits
#        (B, Fi, D, O), extra
SHAPES = [((1, 1, 1, 1), None),
          ((2, 3, 1, 5), None),                      # D 1
          ((7, 5, 6, 8), None),                      # ragged
          ((33, 39, 10, 20), None),                  # the reference's D 10 and shape 20
          ((9, 64, 4, 17), None), ((5, 3, 64, 16), None), ((3, 4, 4, 64), None),      # each limit in turn
          ((GRID, 4, 4, 5), None),
          ((33, 39, 10, 20), "wide"),                # orders = randn / 2: ut far outside [-pi, pi], exp(ul) over decades
          ((7, 5, 6, 8), "planted")]                 # (r, p) in {(0, 0), (-1, +0), (-1, -0)}
CASES = [(s, e, ln) for s, e in SHAPES for ln in (False, True) if not ln or s[2] >= 4]
PLANTED = [(0.0, 0.0), (-1.0, 0.0), (-1.0, -0.0)]
LEAVES = ["r", "p", "Z", "orders", "blam", "bth", "wr", "br", "wp", "bp"]


def make_inputs(shape, extra, seed):
    B, Fi, D, O = shape
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)    # noqa: E731
    z = rnd(2 * B, O * D)
    t = {"r": rnd(B, Fi, D), "p": rnd(B, Fi, D), "Z": torch.where(z < 0, -1.0, 1.0) * z.abs().clamp(min=1e-3),
         "orders": rnd(Fi, O) / 2 if extra == "wide" else torch.softmax(rnd(Fi, O), dim=0),
         "blam": 0.1 * rnd(D, O), "bth": 0.1 * rnd(D, O), "wr": 1 + 0.1 * rnd(D), "br": 0.1 * rnd(D),
         "wp": 1 + 0.1 * rnd(D), "bp": 0.1 * rnd(D), "dOP": rnd(2, B, O, D)}
    if extra == "planted":
        for k, (r, p) in enumerate(PLANTED):
            t["r"].view(-1)[7 * k], t["p"].view(-1)[7 * k] = r, p
    return {k: v.double() for k, v in t.items()}


def compare(tag, ref, f32, got):
    """every tensor of `ref` against `got` under the yardstick -> the largest err / bound"""
    assert sorted(got) == sorted(ref)
    worst, failures = 0.0, []
    for name, r in ref.items():
        g = got[name].double().cpu().reshape(r.shape)
        assert bool(torch.isfinite(g).all()), (tag, name)
        e32 = float((f32[name] - r).abs().max())
        bound = 4.0 * e32 + 1e-6 * float(r.abs().max())
        err = float((g - r).abs().max())
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print("%s %-8s err %.3e  e32 %.3e  bound %.3e  err/bound %.3f" % (tag, name, err, e32, bound, ratio))
        if not err <= bound:
            failures.append((name, err, bound))
    assert not failures, (tag, failures)
    return worst


def run_torch(t, ln, dtype):
    leaves = [t[k].to(dtype).clone().requires_grad_(True) for k in LEAVES[:6 + 4 * ln]]
    OP = torch.stack(euler_reference(*leaves[:6], leaves[6:] if ln else None))
    grads = torch.autograd.grad(OP, leaves, t["dOP"].to(dtype))
    out = {"OP": OP.detach(), "dRP": torch.stack(grads[:2])}
    out.update(("d" + k, g) for k, g in zip(LEAVES[2:], grads[2:]))
    return {k: v.double() for k, v in out.items()}


def run_hip(t, ln):
    dev = torch.device("cuda:0")
    B, Fi, D = t["r"].shape
    O = t["orders"].shape[1]
    p = {k: t[k].float().to(dev).contiguous() for k in LEAVES[2:] + ["dOP"]}
    RP = torch.stack((t["r"], t["p"])).float().to(dev)
    full = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)    # noqa: E731
    OP, stats, ws = full(2, B, O, D), full(4, B, O), full(ops.euler_workspace_floats(B, Fi, D, O))
    ops.euler_fwd(RP, p["Z"], p["orders"], p["blam"], p["bth"], (p["wr"], p["br"], p["wp"], p["bp"]) if ln else None,
                  1e-5, stats, OP)
    dZ, dRP, d_orders, d_bias, d_norm = full(2 * B, O * D), full(2, B, Fi, D), full(Fi, O), full(2, D, O), full(2, 2, D)
    ops.euler_bwd(RP, p["Z"], p["orders"], p["blam"], p["bth"], (p["wr"], p["wp"]) if ln else None, 1e-5, stats,
                  p["dOP"], dZ, dRP, d_orders, d_bias, d_norm, ws)
    torch.cuda.synchronize()
    out = {"OP": OP, "dRP": dRP, "dZ": dZ, "dorders": d_orders, "dblam": d_bias[0], "dbth": d_bias[1]}
    if ln:
        out.update(dwr=d_norm[0, 0], dbr=d_norm[0, 1], dwp=d_norm[1, 0], dbp=d_norm[1, 1])
    return out


def grid_batch(D):
    lim = ops.euler_limits()
    return lim["workgroups"] * min(lim["tile_samples"], lim["tile_columns"] // D) + 3


@pytest.mark.parametrize("shape,extra,ln", CASES,
                         ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_layer_forward_and_gradients_within_the_fp32_yardstick(shape, extra, ln):
    if shape[0] == GRID:
        shape = (grid_batch(shape[2]),) + shape[1:]
    t = make_inputs(shape, extra, seed=sum(shape))
    ref, f32, got = run_torch(t, ln, torch.float64), run_torch(t, ln, torch.float32), run_hip(t, ln)
    compare("euler %s %s ln=%d" % (shape, extra, ln), ref, f32, got)
    if extra == "planted":                   # torch masks atan2's 0 / 0: exactly 0 on both sides
        at = torch.arange(1) * 7
        for side in (got["dRP"].cpu().double(), ref["dRP"]):
            assert bool((side.reshape(2, -1)[:, at] == 0).all())


@pytest.mark.parametrize("shape,pad", [((1, 1, 1), 0), ((7, 5, 6), 0), ((33, 39, 10), 0), ((5, 64, 64), 0),
                                       ((GRID, 4, 4), 0), ((7, 5, 6), 1)],
                         ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else "pad%d" % v)
def test_polar_front_end_within_the_fp32_yardstick(shape, pad):
    if shape[0] == GRID:
        shape = (grid_batch(shape[2]),) + shape[1:]
    B, F, D = shape
    dev, gen = torch.device("cuda:0"), torch.Generator().manual_seed(sum(shape))
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)    # noqa: E731
    t = {"E": 2 * rnd(B, F, D), "mu": 1 + 0.1 * rnd(1, F, 1), "dRP": rnd(2, B, F, D)}

    def run_torch_polar(dtype):
        E, mu = (t[k].to(dtype).clone().requires_grad_(True) for k in ("E", "mu"))
        RP = torch.stack((mu * torch.cos(E), mu * torch.sin(E)))
        dE, dmu = torch.autograd.grad(RP, (E, mu), t["dRP"].to(dtype))
        return {"RP": RP.detach().double(), "dE": dE.double(), "dmu": dmu.double()}
    full = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)    # noqa: E731
    rec, drec = torch.full((B, F + pad, D), 7.0, dtype=torch.float32, device=dev), full(B, F + pad, D)
    E, dE = rec[:, :F, :], drec[:, :F, :]
    E.copy_(t["E"])
    mu, RP, dmu, ws = t["mu"].to(dev), full(2, B, F, D), full(1, F, 1), full(ops.euler_workspace_floats(B, F, D, 1))
    ops.euler_polar_fwd(E, mu, RP)
    ops.euler_polar_bwd(E, mu, t["dRP"].to(dev), dE, dmu, ws)
    torch.cuda.synchronize()
    if pad:                                  # the slots behind the fields are nobody's to write
        assert bool((rec[:, F:, :] == 7.0).all()) and bool(torch.isnan(drec[:, F:, :]).all())
    compare("euler polar %s pad=%d" % (shape, pad), run_torch_polar(torch.float64), run_torch_polar(torch.float32),
            {"RP": RP, "dE": dE.contiguous(), "dmu": dmu})
