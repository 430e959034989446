"""FiBiNET's kernels (csrc/fx_bilinear.hip) alone, through fuxictr_amd.ops, on a real MI355X against fp64
torch-autograd restatements written from the layers' formulas (tests/test_fibinet_host.py):
    squeeze-excitation   Z = mean_d X;  A = act(W2 relu(W1 Z));  V = X * A[:, :, None]
    bilinear interaction out[b, p, :] = ((a_i x_i) W_w(p)) * (a_j x_j),  pairs in triu order, w(p) = 0 | i | p

The tolerance is the yardstick of tests/test_gpu_mhsa.py: the same formulas in fp32 torch on the CPU have an error
e32 against the fp64 result, per output tensor (max |.|); the HIP result must lie within
    4 * e32 + 1e-6 * max|ref|.
Every case prints its observed ratio err / bound.

The excitation's two ReLUs sit inside the kernel: a sample with an fp64 pre-activation within 1e-4 of zero is
decided by the last bit of whoever computes it.  Such samples are left out of the comparison of A, V and dX
(at most 5 % of a case's samples, asserted), and dW1 / dW2 are compared only when no sample had to be left out.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import _lib, ops  # noqa: E402
from test_fibinet_host import bilinear_reference, senet_reference  # noqa: E402

#          B   F   D
SHAPES = [(7, 2, 8),          # one pair
          (33, 5, 10),        # D not a multiple of 4: the scalar path
          (65, 39, 16),       # Criteo's fields, more than one sample tile
          (50, 24, 40),       # FiBiNET_default's dims
          (5, 64, 4), (3, 3, 64),     # the limits
          (1, 39, 16)]
KINDS = ["field_all", "field_each", "field_interaction"]
KINK = 1e-4
SENET_SEED = 901      # (chosen on the CPU: with it no case loses more than 5 % of its samples to the kink band)
DEV = "cuda:0"


def _ids(s):
    return "B%d-F%d-D%d" % s


def compare(tag, got, ref, f32, extra=None):
    """Every tensor of `ref` (fp64) against `got` within 4 e32 + 1e-6 max|ref| -> the worst err / bound."""
    worst, failures = 0.0, []
    for name, r in ref.items():
        g = got[name].double().cpu()
        assert bool(torch.isfinite(g).all()), (tag, name)
        e32 = float((f32[name] - r).abs().max()) if r.numel() else 0.0
        bound = 4.0 * e32 + 1e-6 * (float(r.abs().max()) if r.numel() else 0.0) + (extra or {}).get(name, 0.0)
        err = float((g - r).abs().max()) if r.numel() else 0.0
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print("%s %-4s err %.3e  e32 %.3e  bound %.3e  err/bound %.3f" % (tag, name, err, e32, bound, ratio))
        if not err <= bound:
            failures.append((name, err, bound))
    print("%s worst err/bound %.3f" % (tag, worst))
    assert not failures, (tag, failures)
    return worst


# ---- bilinear interaction -------------------------------------------------------------------------------
def bilinear_inputs(shape, kind, scaled, seed):
    B, F, D = shape
    P = F * (F - 1) // 2
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(B, F, D, generator=gen, dtype=torch.float64)
    lead = {"field_all": (), "field_each": (F,), "field_interaction": (P,)}[kind]
    W = torch.randn(*lead, D, D, generator=gen, dtype=torch.float64) / D ** 0.5
    A = torch.rand(B, F, generator=gen, dtype=torch.float64) * 1.5 if scaled else None
    if scaled:
        A[torch.rand(B, F, generator=gen) < 0.3] = 0.0          # gates a ReLU closed
    dOut = torch.randn(B, P, D, generator=gen, dtype=torch.float64)
    return X, W, A, dOut


def bilinear_torch(X, W, A, dOut, kind, dtype):
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (X, W) + ((A,) if A is not None else ())]
    y = bilinear_reference(leaves[0], leaves[1], ops.BILINEAR_TYPES[kind], leaves[2] if A is not None else None)
    grads = torch.autograd.grad(y, leaves, dOut.to(dtype))
    out = {"out": y.detach().double(), "dX": grads[0].double(), "dW": grads[1].double()}
    if A is not None:
        out["dA"] = grads[2].double()
    return out


def bilinear_hip(X, W, A, dOut, kind, record_pad=0, col=0, tail=0, accumulate=False):
    """X / dX as [:, :F, :] views of [B, F + record_pad, D] records (7.0 / 3.0 in the slots behind), out / dOut as
    the columns [col, col + P D) of rows with `col + P D + tail` floats (5.0 elsewhere).  accumulate: dX is ADDED
    to the buffer's 3.0, taken off again here."""
    B, F, D = X.shape
    PD = (F * (F - 1) // 2) * D
    k = ops.BILINEAR_TYPES[kind]
    rec = torch.full((B, F + record_pad, D), 7.0, dtype=torch.float32, device=DEV)
    x = rec[:, :F, :]
    x.copy_(X.float())
    w = W.float().to(DEV).contiguous()
    a = None if A is None else A.float().to(DEV).contiguous()
    buf = torch.full((B, col + PD + tail), 5.0, dtype=torch.float32, device=DEV)
    ops.bilinear_fwd(x, w, k, a, buf, out_col=col)
    torch.cuda.synchronize()
    assert bool((buf[:, :col] == 5.0).all()) and bool((buf[:, col + PD:] == 5.0).all())      # nobody's columns
    assert bool((rec[:, F:, :] == 7.0).all())
    gbuf = torch.full((B, col + PD + tail), 9.0, dtype=torch.float32, device=DEV)
    gbuf[:, col:col + PD] = dOut.float().reshape(B, PD).to(DEV)
    drec = torch.full((B, F + record_pad, D), 3.0, dtype=torch.float32, device=DEV)
    dX = drec[:, :F, :]
    dA = torch.empty(B, F, dtype=torch.float32, device=DEV) if a is not None else None
    dW = torch.empty_like(w)
    ws = torch.empty(ops.bilinear_workspace_floats(B, F, D), dtype=torch.float32, device=DEV)
    ops.bilinear_bwd(x, w, k, a, gbuf, dX, dA, dW, ws, dout_col=col, dx_accumulate=accumulate)
    torch.cuda.synchronize()
    assert bool((drec[:, F:, :] == 3.0).all())
    got = {"out": buf[:, col:col + PD].reshape(B, -1, D).clone(),
           "dX": dX - 3.0 if accumulate else dX.contiguous(), "dW": dW}
    if a is not None:
        got["dA"] = dA
    return got


# dW's sum over the sample slabs (16 samples each at these sizes) has P D D columns, 64 per workgroup of four waves:
# two and five slabs (SHAPES has 1, 3, 4 and 9), one column, one workgroup's 64 missed by four and passed by two
ROWSUM_SHAPES = [(17, 2, 1), (65, 6, 2), (17, 12, 1)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES + ROWSUM_SHAPES, ids=_ids)
def test_bilinear_forward_and_gradients_within_the_fp32_yardstick(shape, kind, scaled):
    X, W, A, dOut = bilinear_inputs(shape, kind, scaled, seed=sum(shape) + 7 * KINDS.index(kind) + scaled)
    ref = bilinear_torch(X, W, A, dOut, kind, torch.float64)
    f32 = bilinear_torch(X, W, A, dOut, kind, torch.float32)
    tag = "bilinear %s %s %s" % (shape, kind, "scaled" if scaled else "plain")
    first = bilinear_hip(X, W, A, dOut, kind)
    compare(tag, first, ref, f32)
    again = bilinear_hip(X, W, A, dOut, kind)                   # the same inputs: the same bits
    for name in first:
        assert torch.equal(first[name], again[name]), name
    # X / dX inside a wider record, out / dOut inside wider rows at an aligned column, dX added to the buffer
    laid = bilinear_hip(X, W, A, dOut, kind, record_pad=1, col=8, tail=4, accumulate=True)
    compare(tag + " in place", laid, ref, f32, extra={"dX": 2.0 ** -22 * max(1.0, float(ref["dX"].abs().max()))})
    # (3 + dX) - 3 in fp32: one rounding at magnitude <= 4 max(1, |dX|)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=_ids)
def test_bilinear_at_an_unaligned_column_takes_the_scalar_path(shape):
    X, W, A, dOut = bilinear_inputs(shape, "field_interaction", True, seed=500 + sum(shape))
    ref = bilinear_torch(X, W, A, dOut, "field_interaction", torch.float64)
    f32 = bilinear_torch(X, W, A, dOut, "field_interaction", torch.float32)
    got = bilinear_hip(X, W, A, dOut, "field_interaction", record_pad=2, col=3, tail=2)
    compare("bilinear unaligned %s" % (shape,), got, ref, f32)


# ---- squeeze-excitation ---------------------------------------------------------------------------------
def senet_inputs(shape, R, seed):
    """Unit-variance pre-activations: Z = mean_d X has variance 1 for X ~ N(0, D)."""
    B, F, D = shape
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(B, F, D, generator=gen, dtype=torch.float64) * D ** 0.5
    W1 = torch.randn(R, F, generator=gen, dtype=torch.float64) / F ** 0.5
    W2 = torch.randn(F, R, generator=gen, dtype=torch.float64) * (2.0 / R) ** 0.5
    dA = torch.randn(B, F, generator=gen, dtype=torch.float64)
    dV = torch.randn(B, F, D, generator=gen, dtype=torch.float64)
    return X, W1, W2, dA, dV


def senet_steady_samples(X, W1, W2, act):
    """Samples none of whose fp64 pre-activations lies within KINK of a ReLU's kink."""
    h = X.mean(dim=-1) @ W1.t()
    near = (h.abs() < KINK).any(dim=1)
    if act == 0:
        # (with every hidden unit closed the outer pre-activation is an exact 0 in any arithmetic: relu(0) = 0 with
        # slope 0 for everybody, nothing is decided by a last bit)
        near |= ((torch.relu(h) @ W2.t()).abs() < KINK).any(dim=1) & (h > 0).any(dim=1)
    return ~near


def senet_torch(X, W1, W2, dA, dV, act, dtype):
    x, w1, w2 = (t.to(dtype).clone().requires_grad_(True) for t in (X, W1, W2))
    a, v = senet_reference(x, w1, w2, act)
    outs, gs = [], []
    if dA is not None:
        outs.append(a), gs.append(dA.to(dtype))
    if dV is not None:
        outs.append(v), gs.append(dV.to(dtype))
    gx, g1, g2 = torch.autograd.grad(outs, [x, w1, w2], gs)
    return {"A": a.detach().double(), "V": v.detach().double(), "dX": gx.double(), "dW1": g1.double(),
            "dW2": g2.double()}


def senet_hip(X, W1, W2, dA, dV, act, record_pad=0, accumulate=False):
    B, F, D = X.shape
    rec = torch.full((B, F + record_pad, D), 7.0, dtype=torch.float32, device=DEV)
    x = rec[:, :F, :]
    x.copy_(X.float())
    w1, w2 = W1.float().to(DEV).contiguous(), W2.float().to(DEV).contiguous()
    A = torch.empty(B, F, dtype=torch.float32, device=DEV)
    V = torch.empty(B, F, D, dtype=torch.float32, device=DEV)
    ops.senet_fwd(x, w1, w2, act, A, V)
    A_only = torch.empty_like(A)
    ops.senet_fwd(x, w1, w2, act, A_only)                       # no V asked for: the same gates
    drec = torch.full((B, F + record_pad, D), 3.0, dtype=torch.float32, device=DEV)
    dX = drec[:, :F, :]
    dW1, dW2 = torch.empty_like(w1), torch.empty_like(w2)
    ws = torch.empty(ops.senet_workspace_floats(B, F, w1.shape[0]), dtype=torch.float32, device=DEV)
    ops.senet_bwd(x, w1, w2, act, A, None if dA is None else dA.float().to(DEV).contiguous(),
                  None if dV is None else dV.float().to(DEV).contiguous(), dX, dW1, dW2, ws,
                  dx_accumulate=accumulate)
    torch.cuda.synchronize()
    assert torch.equal(A, A_only)
    assert bool((rec[:, F:, :] == 7.0).all()) and bool((drec[:, F:, :] == 3.0).all())
    return {"A": A, "V": V, "dX": dX - 3.0 if accumulate else dX.contiguous(), "dW1": dW1, "dW2": dW2}


def senet_case(shape, act, R, seed):
    B, F, D = shape
    X, W1, W2, dA, dV = senet_inputs(shape, R, seed)
    keep = senet_steady_samples(X, W1, W2, act)
    dropped = int((~keep).sum())
    print("senet %s act %d R %d: %d of %d samples within %.0e of a kink" % (shape, act, R, dropped, B, KINK))
    assert dropped <= 0.05 * B, (shape, act, R, dropped)
    return X, W1, W2, dA, dV, keep, dropped


def senet_check(tag, X, W1, W2, dA, dV, act, keep, dropped, **layout):
    got = senet_hip(X, W1, W2, dA, dV, act, **layout)
    # the samples are independent of each other: the reference of the kept ones is the reference ON the kept ones
    sub = lambda t: None if t is None else t[keep]
    ref = senet_torch(X[keep], W1, W2, sub(dA), sub(dV), act, torch.float64)
    f32 = senet_torch(X[keep], W1, W2, sub(dA), sub(dV), act, torch.float32)
    got = {k: (v if k in ("dW1", "dW2") else v[keep.to(v.device)]) for k, v in got.items()}
    if dropped:                                                 # the kernel's sums hold the dropped samples too
        for k in ("dW1", "dW2"):
            ref.pop(k), f32.pop(k)
    extra = {"dX": 2.0 ** -22 * max(1.0, float(ref["dX"].abs().max()))} if layout.get("accumulate") else None
    return compare(tag, got, ref, f32, extra=extra)


@pytest.mark.parametrize("act", [0, 1], ids=["relu", "sigmoid"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_senet_forward_and_gradients_within_the_fp32_yardstick(shape, act):
    B, F, D = shape
    for R in sorted({max(1, F // 3), 1}):
        X, W1, W2, dA, dV, keep, dropped = senet_case(shape, act, R, seed=SENET_SEED + sum(shape) + act + 31 * R)
        tag = "senet %s act %d R %d" % (shape, act, R)
        senet_check(tag + " dV", X, W1, W2, None, dV, act, keep, dropped)              # the layer alone
        senet_check(tag + " dA", X, W1, W2, dA, None, act, keep, dropped)              # the fused model's call
        senet_check(tag + " both in place", X, W1, W2, dA, dV, act, keep, dropped, record_pad=1,
                    accumulate=True)
        a = senet_hip(X, W1, W2, dA, dV, act)
        b = senet_hip(X, W1, W2, dA, dV, act)
        for name in a:
            assert torch.equal(a[name], b[name]), name


#                B  F  D  R    dW1 / dW2: a row sum over ceil(B / 4) partials of F R columns, 64 per workgroup
SENET_ROWSUM = [(9, 1, 4, 1),       # 3 rows, 1 column
                (13, 9, 4, 7),      # 4 rows, 63 columns
                (17, 13, 4, 5)]     # 5 rows, 65 columns     (the shapes above: 1, 2, 9, 13, 17 rows; 64 and 507 columns)


@pytest.mark.parametrize("case", SENET_ROWSUM, ids=lambda c: "B%d-F%d-D%d-R%d" % c)
def test_senet_weight_gradients_over_few_partial_rows_and_columns(case):
    B, F, D, R = case
    assert ops.senet_workspace_floats(B, F, R) == -(-B // 4) * 2 * F * R
    X, W1, W2, dA, dV, keep, dropped = senet_case((B, F, D), 1, R, seed=SENET_SEED + sum(case))
    assert dropped == 0                                         # so that dW1 and dW2 are compared
    senet_check("senet rowsum %s" % (case,), X, W1, W2, dA, dV, 1, keep, dropped)


def test_shapes_beyond_the_limits_are_rejected_with_a_message():
    def bilinear(B, F, D):
        x = torch.zeros(B, F, D, device=DEV)
        P = F * (F - 1) // 2
        ops.bilinear_fwd(x, torch.zeros(P, D, D, device=DEV), 2, None, torch.zeros(B, P * D, device=DEV))
    with pytest.raises(_lib.FxError, match="F=65"):
        bilinear(2, 65, 4)
    with pytest.raises(_lib.FxError, match="D=65"):
        bilinear(2, 3, 65)
    with pytest.raises(_lib.FxError, match="R=65"):
        ops.senet_fwd(torch.zeros(2, 4, 4, device=DEV), torch.zeros(65, 4, device=DEV),
                      torch.zeros(4, 65, device=DEV), 0, torch.zeros(2, 4, device=DEV))
    bilinear(2, 64, 64)                 # the largest shape itself runs
    torch.cuda.synchronize()
