"""AFN's logarithmic transformation kernels (csrc/fx_lognet.hip) alone, through fuxictr_amd.ops, on a real MI355X
against the layer in plain torch (tests/test_afn_host.py:lognet_reference, two training-mode batch norms around the
log / product over fields / exp) under fp64 autograd: Y, dX, dW, the four affine gradients, both pairs of running
statistics and both step counters.

Yardstick (that of tests/test_gpu_destine_kernel.py and tests/test_gpu_crossmix_kernel.py): per compared tensor e32 =
max |the same layer in fp32 torch on the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  The
factor 4 covers another summation order.  Every case prints its observed err / bound.  Outputs and workspace are
pre-filled with NaN and every element is compared.  Inputs are drawn in fp32 and widened, so both sides see the same x
and take the same side of the clamp; |x| is floored at 1e-3 * scale except where a case plants clamped elements.
"accumulate" adds dX to a buffer of 3.0 and takes the 3.0 off again: (3 + dX) - 3 in fp32 rounds once, at magnitude
<= 3 + max|dX|, so that case's dX bound grows by 2^-23 (3 + max|ref|)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_afn_host import lognet_reference  # noqa: E402

GRID = "grid"        # B such that the (sample, d) column tiles outnumber the workgroups of every pass: lognet_limits
#        (B, F, D, L), x scale, W scale, extra
CASES = [((1, 1, 2, 1), 1.0, 1.0, None),            # one field, one neuron, two values per statistic
         ((2, 3, 1, 5), 1.0, 1.0, None),            # D 1
         ((7, 5, 6, 8), 1.0, 1.0, None),            # ragged
         ((33, 39, 16, 24), 1.0, 1.0, None),        # L no multiple of the tile
         ((9, 64, 4, 17), 1.0, 1.0, None),          # F at its limit
         ((5, 3, 64, 16), 1.0, 1.0, None),          # D at its limit
         ((3, 4, 4, 2048), 1.0, 1.0, None),         # L at its limit
         ((GRID, 4, 4, 5), 1.0, 1.0, None),
         ((33, 39, 16, 24), 1e-4, 1.0, None),       # a = -9.5 +- 1: plain sums of a, a^2 lose BN_log's variance
         ((257, 8, 4, 5), 1e-4, 0.05, None),        # and c = 1 +- eps: the same for BN_exp
         ((7, 5, 6, 8), 1.0, 1.0, "planted"),       # x in {0, +-1e-7, 1e-6}: log 1e-5 forward, dX exactly 0
         ((7, 5, 6, 8), 1.0, 1.0, "pad"),           # X, dX with a padded sample stride
         ((9, 7, 4, 12), 1.0, 1.0, "accumulate"),
         ((7, 5, 6, 8), 1.0, 1.0, "eval")]          # one launch on the running statistics, which stay as they are
PLANTED = [0.0, 1e-7, -1e-7, 1e-6]
PARAMS = ["W", "g1", "b1", "g2", "b2"]
BUFS = ["rm1", "rv1", "rm2", "rv2"]


def make_inputs(shape, scale, wscale, extra, seed):
    B, F, D, L = shape
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)    # noqa: E731
    x = rnd(B, F, D) * scale
    x = torch.where(x < 0, -1.0, 1.0) * x.abs().clamp(min=1e-3 * scale)
    if extra == "planted":
        x.view(-1)[torch.arange(len(PLANTED)) * 7] = torch.tensor(PLANTED)
    t = {"x": x, "W": rnd(L, F) * (wscale / F ** 0.5), "g1": 1 + 0.1 * rnd(F), "b1": 0.1 * rnd(F),
         "g2": 1 + 0.1 * rnd(L), "b2": 0.1 * rnd(L), "rm1": rnd(F), "rv1": 0.5 + rnd(F).abs(), "rm2": 1 + rnd(L),
         "rv2": 0.5 + rnd(L).abs(), "dY": rnd(B, L * D)}
    return {k: v.double() for k, v in t.items()}


def run_torch(t, training, dtype):
    leaves = [t[k].to(dtype).clone().requires_grad_(True) for k in ["x"] + PARAMS]
    bufs = [t[k].to(dtype).clone() for k in BUFS]
    Y = lognet_reference(*leaves, *bufs, training)
    out = {"Y": Y.detach().double()}
    out.update((k, b.double()) for k, b in zip(BUFS, bufs))
    if training:
        grads = torch.autograd.grad(Y, leaves, t["dY"].to(dtype))
        out.update(("d" + k, g.double()) for k, g in zip(["X"] + PARAMS, grads))
    return out


def run_hip(t, training, extra):
    """-> the same dict from ops.lognet_fwd / lognet_bwd, and the two step counters (3 before the forward)."""
    dev = torch.device("cuda:0")
    B, F, D = t["x"].shape
    L = t["W"].shape[0]
    pad, acc, nan = (1 if extra in ("pad", "accumulate") else 0), extra == "accumulate", float("nan")
    rec = torch.full((B, F + pad, D), 7.0, dtype=torch.float32, device=dev)
    x = rec[:, :F, :]
    x.copy_(t["x"].float())
    p = {k: t[k].float().to(dev).contiguous() for k in PARAMS + BUFS + ["dY"]}
    nbt = [torch.full((), 3, dtype=torch.int64, device=dev) for _ in range(2)]
    full = lambda *s: torch.full(s, nan, dtype=torch.float32, device=dev)    # noqa: E731
    Y, stats, ws = full(B, L * D), full(ops.lognet_stats_floats(F, L)), full(ops.lognet_workspace_floats(B, F, D, L))
    ops.lognet_fwd(x, p["W"], p["g1"], p["b1"], p["g2"], p["b2"], 1e-5, 0.1, training, (p["rm1"], p["rv1"], nbt[0]),
                   (p["rm2"], p["rv2"], nbt[1]), stats, Y, ws)
    out = {"Y": Y}
    out.update((k, p[k]) for k in BUFS)
    if training:
        drec = torch.full((B, F + pad, D), 3.0 if acc else nan, dtype=torch.float32, device=dev)
        dX, g = drec[:, :F, :], {k: full(*p[k].shape) for k in PARAMS}
        ws.fill_(nan)
        ops.lognet_bwd(x, p["W"], p["g1"], p["b1"], p["g2"], 1e-5, stats, p["dY"], dX, g["W"], g["g1"], g["b1"],
                       g["g2"], g["b2"], ws, dx_accumulate=acc)
        torch.cuda.synchronize()
        if pad:                          # the slots behind the fields are nobody's to write
            tail = drec[:, F:, :]
            assert bool((tail == 3.0).all()) if acc else bool(torch.isnan(tail).all())
        out["dX"] = dX - 3.0 if acc else dX.contiguous()
        out.update(("d" + k, v) for k, v in g.items())
    return out, [int(n) for n in nbt]


@pytest.mark.parametrize("shape,scale,wscale,extra", CASES,
                         ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v)
                         if isinstance(v, tuple) else "plain" if v is None else "%g" % v)
def test_forward_and_gradients_within_the_fp32_yardstick(shape, scale, wscale, extra):
    lim = ops.lognet_limits()
    if shape[0] == GRID:
        shape = (lim["workgroups"] * lim["tile_columns"] // shape[2] + 3,) + shape[1:]
    training = extra != "eval"
    t = make_inputs(shape, scale, wscale, extra, seed=sum(shape))
    ref, f32 = run_torch(t, training, torch.float64), run_torch(t, training, torch.float32)
    got, counters = run_hip(t, training, extra)
    assert sorted(got) == sorted(ref) and counters == ([4, 4] if training else [3, 3])
    tag, failures = "lognet %s %g %g %s" % (shape, scale, wscale, extra), []
    for name, r in ref.items():
        g = got[name].double().cpu().reshape(r.shape)
        assert bool(torch.isfinite(g).all()), (tag, name)
        e32 = float((f32[name] - r).abs().max())
        bound = 4.0 * e32 + 1e-6 * float(r.abs().max())
        if extra == "accumulate" and name == "dX":
            bound += 2.0 ** -23 * (3.0 + float(r.abs().max()))
        err = float((g - r).abs().max())
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %-4s err %.3e  e32 %.3e  bound %.3e  err/bound %.3f" % (tag, name, err, e32, bound, ratio))
        if not err <= bound:
            failures.append((name, err, bound))
    if extra == "planted":
        planted = got["dX"].reshape(-1)[torch.arange(len(PLANTED)) * 7]
        assert bool((planted == 0).all()) and bool((ref["dX"].reshape(-1)[torch.arange(len(PLANTED)) * 7] == 0).all())
    if not training:
        assert all(bool((got[k].cpu() == t[k].float()).all()) for k in BUFS)
    assert not failures, (tag, failures)
