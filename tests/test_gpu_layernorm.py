"""MaskNet's kernels (csrc/fx_layernorm.hip) alone, through fuxictr_amd.ops, on a real MI355X against fp64
torch-autograd restatements written from the formulas (tests/test_masknet_host.py):
    grouped LayerNorm   mu = mean_n x;  rstd = 1 / sqrt(mean_n (x - mu)^2 + eps);  y = (x - mu) rstd gamma + beta (+ ReLU)
    mask gradient       out[r, h] = sum_k dM[r, k H + h] * Vmask[r, k H + h]

The tolerance is the yardstick of tests/test_gpu_bilinear.py: the same formulas in fp32 torch on the CPU have an
error e32 against the fp64 result, per output tensor (max |.|); the HIP result must lie within
    4 * e32 + 1e-6 * max|ref|.
Every case prints its observed ratio err / bound.  The inputs are fp32 numbers, so all three computations start from
the same values.

The fused ReLU's mask is an input of the backward (the kernel reads it from its own Y), so the fp64 reference
backward takes the mask from the kernel's Y and the forward test pins that mask: Y > 0 exactly where the fp64
pre-activation is > 0 for every element with |z64| >= 1e-4, and |Y| <= 1e-4 + bound for the rest.  No element is
left out of any comparison."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_masknet_host import layernorm_reference, mask_grad_reference  # noqa: E402

DEV = "cuda:0"
EPS = 1e-5
KINK = 1e-4

#          rows G  N
SHAPES = [(7, 1, 1),            # var = 0: y = beta exactly
          (33, 5, 10),          # the scalar path; dgamma / dbeta over 33 rows, a slab each
          (65, 39, 16),         # Criteo's record
          (5, 64, 4), (3, 3, 64),       # the grouped limits
          (1, 39, 16)]
# lane boundaries and elements per lane
SHAPES += [(257, 1, n) for n in (3, 63, 64, 65, 255, 256, 257, 1000, 1028)]
# the regime switch points of fx_layernorm.hip: 64 | 65 above; a wave per row up to 512 (scalar) / 2048 (16-byte),
# the chunk counts per lane inside it (128, 256 scalar; 256, 512, 1024 16-byte), a workgroup per row above
SHAPES += [(257, 1, n) for n in (127, 128, 129, 511, 512, 513, 516, 1023, 1024, 1025)]
SHAPES += [(9, 1, n) for n in (2044, 2047, 2048, 2049, 2052, 4096, 4100)]
SHAPES += [(3, 1, 8192)]        # the width limit
# dgamma | dbeta leave through a row sum over the slabs (one per row here), 64 columns per workgroup: two slabs (the
# shapes above have 1, 3, 4, 5, 7, 9 and more) and 2 G N = 62, 64 and 66 columns
SHAPES += [(2, 1, 31), (2, 1, 32), (2, 3, 11)]


def _ids(s):
    return "r%d-G%d-N%d" % s


def compare(tag, got, ref, f32, extra=None):
    """Every tensor of `ref` (fp64) against `got` within 4 e32 + 1e-6 max|ref| -> the worst err / bound."""
    worst, failures, bounds = 0.0, [], {}
    for name, r in ref.items():
        g = got[name].double().cpu()
        assert bool(torch.isfinite(g).all()), (tag, name)
        e32 = float((f32[name] - r).abs().max()) if r.numel() else 0.0
        bound = 4.0 * e32 + 1e-6 * (float(r.abs().max()) if r.numel() else 0.0) + (extra or {}).get(name, 0.0)
        err = float((g - r).abs().max()) if r.numel() else 0.0
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        bounds[name] = bound
        print("%s %-6s err %.3e  e32 %.3e  bound %.3e  err/bound %.3f" % (tag, name, err, e32, bound, ratio))
        if not err <= bound:
            failures.append((name, err, bound))
    print("%s worst err/bound %.3f" % (tag, worst))
    assert not failures, (tag, failures)
    return bounds


def f32_exact(t):
    return t.float().double()


def ln_inputs(shape, seed, mean=0.0, std=1.0):
    rows, G, N = shape
    gen = torch.Generator().manual_seed(seed)
    X = f32_exact(mean + std * torch.randn(rows, G * N, generator=gen, dtype=torch.float64))
    gamma = f32_exact(1.0 + 0.5 * torch.randn(G, N, generator=gen, dtype=torch.float64))
    beta = f32_exact(0.3 * torch.randn(G, N, generator=gen, dtype=torch.float64))
    dY = f32_exact(torch.randn(rows, G * N, generator=gen, dtype=torch.float64))
    return X, gamma, beta, dY


def ln_torch(X, gamma, beta, dY, shape, relu, y_kernel, dtype):
    """Forward and autograd backward in `dtype` on the CPU; with the ReLU the backward's mask is the sign of the
    kernel's own Y.  -> tensors as fp64, `z` the pre-activation."""
    rows, G, N = shape
    x, ga, be = (t.to(dtype).clone().requires_grad_(True) for t in (X, gamma, beta))
    z, mu, rstd = layernorm_reference(x, G, N, ga, be, EPS, False)
    g = dY.to(dtype)
    if relu:
        g = g * (y_kernel > 0).to(dtype)
    gx, gg, gb = torch.autograd.grad(z, [x, ga, be], g)
    y = torch.relu(z) if relu else z
    return {"Y": y.detach().double(), "mu": mu.detach().double(), "rstd": rstd.detach().double(),
            "dX": gx.double(), "dgamma": gg.double(), "dbeta": gb.double()}, z.detach().double()


def ln_hip(X, gamma, beta, dY, shape, relu, xpad=0, col=0, tail=0, accumulate=False):
    """X / dX as [:, :G N] views of rows with `xpad` more floats (7.0 / 3.0 behind), Y / dY as the columns
    [col, col + G N) of rows with `col + G N + tail` floats (5.0 / 9.0 elsewhere).  accumulate: dX is ADDED to the
    buffer's 3.0, taken off again here."""
    rows, G, N = shape
    C = G * N
    rec = torch.full((rows, C + xpad), 7.0, dtype=torch.float32, device=DEV)
    x = rec[:, :C]
    x.copy_(X.float())
    ga, be = gamma.float().to(DEV).contiguous(), beta.float().to(DEV).contiguous()
    ybuf = torch.full((rows, col + C + tail), 5.0, dtype=torch.float32, device=DEV)
    stats = torch.empty(rows * G * 2, dtype=torch.float32, device=DEV)
    ops.layernorm_fwd(x, G, N, ga, be, EPS, relu, ybuf, stats, y_col=col)
    torch.cuda.synchronize()
    assert bool((ybuf[:, :col] == 5.0).all()) and bool((ybuf[:, col + C:] == 5.0).all())       # nobody's columns
    assert bool((rec[:, C:] == 7.0).all())
    gbuf = torch.full((rows, col + C + tail), 9.0, dtype=torch.float32, device=DEV)
    gbuf[:, col:col + C] = dY.float().to(DEV)
    drec = torch.full((rows, C + xpad), 3.0, dtype=torch.float32, device=DEV)
    dX = drec[:, :C]
    dgamma, dbeta = torch.empty_like(ga), torch.empty_like(be)
    ws = torch.empty(ops.layernorm_workspace_floats(rows, G, N), dtype=torch.float32, device=DEV)
    ops.layernorm_bwd(x, G, N, ga, relu, ybuf if relu else None, stats, gbuf, dX, dgamma, dbeta, ws, y_col=col,
                      dy_col=col, dx_accumulate=accumulate)
    torch.cuda.synchronize()
    assert bool((drec[:, C:] == 3.0).all()) and bool((ybuf[:, :col] == 5.0).all())
    st = stats.view(rows, G, 2)
    return {"Y": ybuf[:, col:col + C].clone(), "mu": st[:, :, 0].clone(), "rstd": st[:, :, 1].clone(),
            "dX": dX - 3.0 if accumulate else dX.contiguous(), "dgamma": dgamma, "dbeta": dbeta}


def ln_check(tag, X, gamma, beta, dY, shape, relu, **layout):
    got = ln_hip(X, gamma, beta, dY, shape, relu, **layout)
    y_kernel = got["Y"].cpu()
    ref, z64 = ln_torch(X, gamma, beta, dY, shape, relu, y_kernel, torch.float64)
    f32, _ = ln_torch(X, gamma, beta, dY, shape, relu, y_kernel, torch.float32)
    extra = None
    if layout.get("accumulate"):        # (3 + dX) - 3 in fp32: one rounding at magnitude <= 4 max(1, |dX|)
        extra = {"dX": 2.0 ** -22 * max(1.0, float(ref["dX"].abs().max()))}
    bounds = compare(tag, got, ref, f32, extra=extra)
    if relu:                            # the mask the backward used is the right one
        steady = z64.abs() >= KINK
        assert torch.equal((y_kernel > 0)[steady], (z64 > 0)[steady]), tag
        assert bool((y_kernel.double()[~steady].abs() <= KINK + bounds["Y"]).all()), tag
    return got


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_layernorm_forward_and_gradients_within_the_fp32_yardstick(shape, relu):
    rows, G, N = shape
    X, gamma, beta, dY = ln_inputs(shape, seed=17 + rows + 3 * G + 5 * N + relu)
    tag = "layernorm %s %s" % (shape, "relu" if relu else "plain")
    first = ln_check(tag, X, gamma, beta, dY, shape, relu)
    again = ln_hip(X, gamma, beta, dY, shape, relu)                     # the same inputs: the same bits
    for name in first:
        assert torch.equal(first[name], again[name]), name
    if N == 1:                          # var = 0: the centred value is an exact 0, y = beta
        want = beta.float().reshape(1, G * N).expand(rows, G * N)
        assert torch.equal(first["Y"].cpu(), torch.relu(want) if relu else want)
    # X / dX inside a wider record, Y / dY inside wider rows: at an aligned column with dX added to the buffer,
    # and at an unaligned one (the scalar path whatever N is)
    ln_check(tag + " in place", X, gamma, beta, dY, shape, relu, xpad=4, col=8, tail=4, accumulate=True)
    ln_check(tag + " unaligned", X, gamma, beta, dY, shape, relu, xpad=3, col=3, tail=2, accumulate=True)


@pytest.mark.parametrize("shape", [(9, 1, 10), (9, 1, 64), (9, 4, 16), (5, 1, 1000)], ids=_ids)
def test_a_row_of_one_repeated_value_gives_finite_output(shape):
    """var = 0 (to rounding): rstd = 1 / sqrt(eps), y = beta to within rstd times the rounding of the mean."""
    rows, G, N = shape
    _, gamma, beta, dY = ln_inputs(shape, seed=3)
    X = torch.full((rows, G * N), 3.7, dtype=torch.float64).float().double()
    got = ln_hip(X, gamma, beta, dY, shape, False)
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), name
    rstd = got["rstd"].double().cpu()
    assert float((rstd - EPS ** -0.5).abs().max()) <= 1e-5 * EPS ** -0.5
    slack = EPS ** -0.5 * 2.0 ** -22 * 3.7 * float(gamma.abs().max())     # a mean one ulp of 3.7 off
    assert float((got["Y"].double().cpu() - beta.reshape(1, -1)).abs().max()) <= slack


@pytest.mark.parametrize("shape", [(64, 1, 256), (64, 4, 16), (16, 1, 1000), (4, 1, 4096)], ids=_ids)
def test_the_cancellation_row_passes_the_yardstick(shape):
    """Rows with mean 1e4 and standard deviation 1e-2: E[x^2] - mu^2 in fp32 would be the difference of two numbers
    near 1e8 (spacing 8) for a variance of 1e-4: a variance of +-8, rstd = 316 or 0.35 instead of 100, outputs wrong
    by their own magnitude (6 .. 9 here) or NaN.  The spacing of fp32 at 1e4 is 9.8e-4, a tenth of the rows' spread,
    so the fp32 yardstick itself (torch on the CPU, the formulas of test_masknet_host.layernorm_reference, its mean
    one fp32 number) is coarse.  Measured on the CPU at these shapes: e32 of Y 0.06 (N = 4096), 0.12 (1000), 0.21
    (256), 0.55 (16) against max |Y| 6 .. 9, so the bound 4 e32 is 0.24 .. 2.2: meaningful, a lost variance misses
    it; e32 of dX 0.15 .. 24 against max |dX| 500 .. 700.  The kernel's arithmetic restated in fp32 on the CPU (the
    mean refined by the mean of the residuals) is within 1e-6 of fp64 in Y and within 0.3 of the bound in dX and
    dgamma, whose x-hat is recomputed from the one fp32 number that stats keeps for mu."""
    X, gamma, beta, dY = ln_inputs(shape, seed=23 + shape[2], mean=1e4, std=1e-2)
    for relu in (False, True):
        ln_check("layernorm cancellation %s relu %d" % (shape, relu), X, gamma, beta, dY, shape, relu)


# ---- fx_mask_grad ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("shape", [(33, 10, 1), (65, 624, 3), (1, 4, 2)], ids=lambda s: "r%d-H%d-nb%d" % s)
def test_mask_grad_within_the_fp32_yardstick(shape, accumulate):
    rows, H, nb = shape
    gen = torch.Generator().manual_seed(41 + rows + H + nb)
    dM = f32_exact(torch.randn(rows, nb * H, generator=gen, dtype=torch.float64))
    Vm = f32_exact(torch.randn(rows, nb * H, generator=gen, dtype=torch.float64))
    ref = {"out": mask_grad_reference(dM, Vm, H, nb)}
    f32 = {"out": mask_grad_reference(dM.float(), Vm.float(), H, nb).double()}
    results = []
    for _ in range(2):
        buf = torch.full((rows, H + 3), 3.0, dtype=torch.float32, device=DEV)      # out: a prefix of wider rows
        out = buf[:, :H]
        ops.mask_grad(dM.float().to(DEV), Vm.float().to(DEV), H, nb, out, accumulate=accumulate)
        torch.cuda.synchronize()
        assert bool((buf[:, H:] == 3.0).all())
        results.append(out - 3.0 if accumulate else out.contiguous())
    assert torch.equal(results[0], results[1])
    extra = {"out": 2.0 ** -22 * max(1.0, float(ref["out"].abs().max()))} if accumulate else None
    compare("mask_grad %s acc %d" % (shape, accumulate), {"out": results[0]}, ref, f32, extra=extra)
    # contiguous 16-byte aligned operands (H % 4 == 0: the 16-byte path)
    out = torch.empty(rows, H, dtype=torch.float32, device=DEV)
    ops.mask_grad(dM.float().to(DEV), Vm.float().to(DEV), H, nb, out)
    compare("mask_grad %s contiguous" % (shape,), {"out": out}, ref, f32)


def test_shapes_beyond_the_limits_are_rejected_before_the_launch():
    def run(rows, G, N):
        x = torch.zeros(rows, G * N, device=DEV)
        ops.layernorm_fwd(x, G, N, torch.ones(G * N, device=DEV), torch.zeros(G * N, device=DEV), EPS, False,
                          torch.empty_like(x), torch.empty(rows * G * 2, device=DEV))
    with pytest.raises(NotImplementedError, match="N=8193"):
        run(2, 1, 8193)
    with pytest.raises(NotImplementedError, match="G=65"):
        run(2, 65, 4)
    run(2, 64, 64)                      # the limits themselves run
    run(2, 1, 8192)
    torch.cuda.synchronize()
