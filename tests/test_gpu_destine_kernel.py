"""The fused disentangled self-attention kernels (csrc/fx_dsa.hip) alone, through fuxictr_amd.ops, on a real MI355X
against the layer as the reference writes it (tests/test_destine_host.py:dsa_reference, with the flat
view(B H, -1, hd)) under fp64 autograd: Y, dX, every weight and every bias gradient.

Yardstick (that of tests/test_gpu_mhsa.py and tests/test_gpu_crossmix_kernel.py): per compared tensor e32 = max |the
same layer in fp32 torch on the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  The factor 4
covers another summation order over the <= 64-term dot products and the B-term weight-gradient sums.  Every case
prints its observed err / bound.  Outputs and workspace are pre-filled with NaN and every element is compared.

relu_before_att has kinks at q, k, v = 0, where the derivative is decided by the last bit of whoever computes it and
which no mask of the upstream gradient hides: the relu cases run at the shapes with F * A <= 96, and every sample whose
fp64 |q|, |k| or |v| has an element below 1e-5 is taken out of the batch before either side runs — at most 5 % of the
samples (with unit-scale pre-activations ~2e-3 of them are expected)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_destine_host import dsa_reference  # noqa: E402

GRID = "grid"        # B = the forward's most workgroups + 3 (the backward's grid is smaller): read from dsa_limits
#        (B, F, D_in, A, H), (use_scale, relu_before_att, residual), extra
CASES = [((1, 1, 4, 4, 1), (False, True, True), None),          # one field: both soft-maxes are 1, Q~ = 0
         ((7, 5, 6, 8, 2), (True, True, False), None),          # groups straddle fields
         ((9, 7, 4, 12, 3), (False, True, True), None),         # hd 4, ragged
         ((5, 3, 64, 64, 16), (True, False, True), None),       # the head limit, hd 4; 16 gradient entries a thread
         ((3, 64, 10, 16, 2), (False, False, False), None),     # F at its limit: one head per pass
         ((33, 39, 16, 16, 2), (True, False, True), None),      # Criteo
         ((33, 24, 40, 40, 2), (False, False, False), None),    # the reference's default config
         ((GRID, 4, 4, 4, 2), (True, True, True), None),        # more samples than workgroups
         ((3, 64, 64, 64, 2), (True, False, True), None),       # the backward's weights and Wu stay in HBM
         ((3, 64, 16, 64, 16), (False, False, True), None),     # the same at 4 gradient entries a thread
         ((7, 5, 6, 8, 2), (False, False, True), "pad"),        # X, dX with a padded sample stride
         ((9, 7, 4, 12, 3), (True, False, False), "accumulate"),
         ((7, 5, 6, 8, 2), (True, False, True), "peak80")]      # the largest |score| is 80
NAMES = ["dWq", "dWk", "dWv", "dWres", "dWu", "dbq", "dbk", "dbv", "dbres", "dbu"]


def make_inputs(shape, flags, extra, seed):
    B, F, D, A, H = shape
    use_scale, relu, residual = flags
    hd = A // H
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(B, F, D, generator=gen, dtype=torch.float64)
    params = [torch.randn(H if m == 4 else A, D, generator=gen, dtype=torch.float64) / D ** 0.5 for m in range(5)]
    params += [torch.randn(H if m == 4 else A, generator=gen, dtype=torch.float64) for m in range(5)]
    if not residual:
        params[3] = params[8] = None
    if extra == "peak80":                # stretch Wq and bq (the scores are linear in the pair) until max |score| = 80
        def whitened(W, b):
            t = (X @ W.t() + b).view(B * H, -1, hd)
            return t - t.mean(dim=1, keepdim=True)
        scores = torch.bmm(whitened(params[0], params[5]), whitened(params[1], params[6]).transpose(1, 2))
        stretch = 80.0 * (hd ** 0.5 if use_scale else 1.0) / float(scores.abs().max())
        params[0], params[5] = params[0] * stretch, params[5] * stretch
    if relu:                             # away from the kinks: see the module docstring
        assert F * A <= 96
        pre = [(X @ params[m].t() + params[5 + m]).abs().flatten(1).min(dim=1).values for m in range(3)]
        keep = torch.stack(pre).min(dim=0).values >= 1e-5
        assert int((~keep).sum()) <= 0.05 * B and bool(keep.any()), (shape, int((~keep).sum()))
        X = X[keep]
    dY = torch.randn(X.shape[0], F, A, generator=gen, dtype=torch.float64)
    return X, params, dY


def run_torch(X, params, dY, H, flags, dtype):
    leaves = [None if t is None else t.to(dtype).clone().requires_grad_(True) for t in [X] + params]
    Y = dsa_reference(leaves[0], leaves[1:], H, flags[0], flags[1])
    live = [(n, t) for n, t in zip(["dX"] + NAMES, leaves) if t is not None]
    grads = torch.autograd.grad(Y, [t for _, t in live], dY.to(dtype))
    out = {"Y": Y.detach().double()}
    out.update((n, g.double()) for (n, _), g in zip(live, grads))
    return out


def run_hip(X, params, dY, H, flags, extra):
    """-> the same dict from ops.dsa_fwd / dsa_bwd.  "pad", "accumulate": X and dX are views of [B, F + 1, D] records;
    "accumulate": dX is ADDED to the buffer's 3.0 (dx_accumulate), and the 3.0 taken off again here."""
    dev = torch.device("cuda:0")
    B, F, D = X.shape
    pad = 1 if extra in ("pad", "accumulate") else 0
    acc = extra == "accumulate"
    nan = float("nan")
    rec = torch.full((B, F + pad, D), 7.0, dtype=torch.float32, device=dev)
    x = rec[:, :F, :]
    x.copy_(X.float())
    p = [None if t is None else t.float().to(dev).contiguous() for t in params]
    W, bias = p[:5], p[5:]
    A, has_res = W[0].shape[0], W[3] is not None
    Y = torch.full((B, F, A), nan, dtype=torch.float32, device=dev)
    ops.dsa_fwd(x, W, bias, H, flags[0], flags[1], Y)
    drec = torch.full((B, F + pad, D), 3.0 if acc else nan, dtype=torch.float32, device=dev)
    dX = drec[:, :F, :]
    dW = torch.full((ops.dsa_grad_floats(D, A, H, has_res),), nan, dtype=torch.float32, device=dev)
    ws = torch.full((ops.dsa_workspace_floats(B, D, A, H, has_res),), nan, dtype=torch.float32, device=dev)
    ops.dsa_bwd(x, W, bias, H, flags[0], flags[1], dY.float().to(dev).contiguous(), dX, dW, ws, dx_accumulate=acc)
    torch.cuda.synchronize()
    if pad:                              # the slots behind the fields are nobody's to write
        tail = drec[:, F:, :]
        assert bool((tail == 3.0).all()) if acc else bool(torch.isnan(tail).all())
    out = {"Y": Y, "dX": dX - 3.0 if acc else dX.contiguous()}
    sizes = [(n, t.numel()) for n, t in zip(NAMES, [W[0], W[1], W[2], W[3], W[4]] + bias[:4] + [bias[4]])
             if t is not None]
    # fx_dsa_bwd's order: the [A, D] matrices, Wu, the [A] biases, bu
    order = [s for s in sizes if s[0] in NAMES[:4]] + [s for s in sizes if s[0] == "dWu"] + \
        [s for s in sizes if s[0] in NAMES[5:9]] + [s for s in sizes if s[0] == "dbu"]
    assert sum(n for _, n in order) == dW.numel()
    out.update(zip((n for n, _ in order), dW.split([n for _, n in order])))
    return out


@pytest.mark.parametrize("shape,flags,extra", CASES,
                         ids=lambda v: v if isinstance(v, str) else "-".join(str(x if x == GRID else int(x)) for x in v)
                         if v is not None else "plain")
def test_forward_and_gradients_within_the_fp32_yardstick(shape, flags, extra):
    lim = ops.dsa_limits()
    if shape[0] == GRID:
        shape = (max(lim["fwd_workgroups"], lim["bwd_workgroups"]) + 3,) + shape[1:]
    X, params, dY = make_inputs(shape, flags, extra, seed=sum(shape) + 4 * flags[0] + 2 * flags[1] + flags[2])
    H = shape[4]
    ref = run_torch(X, params, dY, H, flags, torch.float64)
    f32 = run_torch(X, params, dY, H, flags, torch.float32)
    got = run_hip(X, params, dY, H, flags, extra)
    assert sorted(got) == sorted(ref)
    tag, failures = "dsa %s %s %s" % (shape, flags, extra), []
    for name, r in ref.items():
        g = got[name].double().cpu().reshape(r.shape)
        assert bool(torch.isfinite(g).all()), (tag, name)
        e32 = float((f32[name] - r).abs().max())
        bound = 4.0 * e32 + 1e-6 * float(r.abs().max())
        if extra == "accumulate" and name == "dX":
            bound += 2.0 ** -22          # (3 + dX) - 3 in fp32: one rounding at magnitude <= 4
        err = float((g - r).abs().max())
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %-6s err %.3e  e32 %.3e  bound %.3e  err/bound %.3f" % (tag, name, err, e32, bound, ratio))
        if not err <= bound:
            failures.append((name, err, bound))
    assert not failures, (tag, failures)
