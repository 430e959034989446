"""The fused self-attention kernels (csrc/fx_mhsa.hip) alone, through fuxictr_amd.ops, on a real MI355X against
an fp64 torch-autograd restatement of the layer (forward, dX and every dW), written here from the layer's
formulas:
    Q = X Wq^T, K = X Wk^T, V = X Wv^T;  per head: P = softmax_rows(Q_h K_h^T [/ sqrt(head_dim)]);  O_h = P V_h
    Y = concat_h(O_h) (+ X Wres^T | + X);  Y = relu(Y)

The tolerance is a yardstick, not a constant: the same layer in fp32 torch on the CPU (the reference's
arithmetic) has an error e32 against the fp64 result, per output tensor (max |.|); the HIP result must lie within
    4 * e32 + 1e-6 * max|ref|.
The factor 4 covers a different summation order over the <= 64-term dot products and the B-term weight-gradient
sums; anything beyond it is a bug, not rounding.  Every case prints its observed ratio err / bound.

The upstream gradient dY is an input of the test: it is zero wherever the fp64 pre-activation lies within 1e-4
of the ReLU's kink, where the derivative is decided by the last bit of whoever computes it.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import _lib, ops  # noqa: E402

#         B     F   D_in  A   H
SHAPES = [(4096, 39, 16, 16, 2),       # Criteo-shaped
          (4096, 39, 16, 32, 2),       # with W_res
          (1000, 24, 40, 40, 2),       # AutoInt_default
          (7, 1, 8, 8, 1),             # one field
          (33, 64, 10, 12, 3),         # ragged dims, head_dim 4
          (5, 3, 64, 64, 64)]          # head_dim 1
FLAGS = [(s, r, a) for s in (False, True) for r in (False, True) for a in (False, True)]


def mhsa_reference(X, Wq, Wk, Wv, Wres, H, use_scale, residual, relu):
    """The layer from its formulas in plain torch ops, in the dtype and on the device of its arguments."""
    B, F, _ = X.shape
    A = Wq.shape[0]
    hd = A // H

    def heads(W):
        return torch.matmul(X, W.t()).view(B, F, H, hd).transpose(1, 2)
    Q, K, V = heads(Wq), heads(Wk), heads(Wv)
    S = torch.matmul(Q, K.transpose(-1, -2))
    if use_scale:
        S = S / hd ** 0.5
    P = S.softmax(dim=-1)
    Y = torch.matmul(P, V).transpose(1, 2).reshape(B, F, A)
    if residual:
        Y = Y + (torch.matmul(X, Wres.t()) if Wres is not None else X)
    return Y.relu() if relu else Y


def make_inputs(shape, residual, seed, score_peak=None):
    B, F, D, A, H = shape
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(B, F, D, generator=gen, dtype=torch.float64)
    W = [torch.randn(A, D, generator=gen, dtype=torch.float64) / D ** 0.5 for _ in range(4)]
    if not (residual and D != A):
        W[3] = None
    dY = torch.randn(B, F, A, generator=gen, dtype=torch.float64)
    if score_peak is not None:          # stretch Wq until the largest |score| is score_peak
        hd = A // H
        Q = (X @ W[0].t()).view(B, F, H, hd).transpose(1, 2)
        K = (X @ W[1].t()).view(B, F, H, hd).transpose(1, 2)
        W[0] = W[0] * (score_peak / float((Q @ K.transpose(-1, -2)).abs().max()))
    return X, W, dY


def run_torch(X, W, dY, H, flags, dtype):
    use_scale, residual, relu = flags
    leaves = [None if t is None else t.to(dtype).clone().requires_grad_(True) for t in [X] + W]
    Y = mhsa_reference(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], H, use_scale, residual, relu)
    live = [t for t in leaves if t is not None]
    grads = torch.autograd.grad(Y, live, dY.to(dtype))
    names = ["dX", "dWq", "dWk", "dWv", "dWres"][:len(live)]
    out = {"Y": Y.detach().double()}
    out.update((n, g.double()) for n, g in zip(names, grads))
    return out


def run_hip(X, W, dY, H, flags, record_pad=0, accumulate=False):
    """-> the same dict from ops.mhsa_fwd / mhsa_bwd.  record_pad: X is a view of a [B, F + pad, D] record.
    accumulate: dX is ADDED to the buffer's 3.0 (dx_accumulate), and the 3.0 taken off again here."""
    use_scale, residual, relu = flags
    dev = torch.device("cuda:0")
    B, F, D = X.shape
    rec = torch.full((B, F + record_pad, D), 7.0, dtype=torch.float32, device=dev)
    x = rec[:, :F, :]
    x.copy_(X.float())
    w = [None if t is None else t.float().to(dev).contiguous() for t in W]
    A = w[0].shape[0]
    Y = torch.empty(B, F, A, dtype=torch.float32, device=dev)
    ops.mhsa_fwd(x, w[0], w[1], w[2], w[3], H, use_scale, residual, relu, Y)
    drec = torch.full((B, F + record_pad, D), 3.0, dtype=torch.float32, device=dev)
    dX = drec[:, :F, :]
    n_w = 4 if w[3] is not None else 3
    dW = torch.empty(n_w, A, D, dtype=torch.float32, device=dev)
    ws = torch.empty(ops.mhsa_workspace_floats(B, D, A, w[3] is not None), dtype=torch.float32, device=dev)
    ops.mhsa_bwd(x, w[0], w[1], w[2], w[3], H, use_scale, residual, relu, Y if relu else None,
                 dY.float().to(dev).contiguous(), dX, dW, ws, dx_accumulate=accumulate)
    torch.cuda.synchronize()
    if record_pad:                      # the slots behind the fields are nobody's to write
        assert bool((drec[:, F:, :] == 3.0).all())
    out = {"Y": Y, "dX": dX - 3.0 if accumulate else dX.contiguous(), "dWq": dW[0], "dWk": dW[1], "dWv": dW[2]}
    if n_w == 4:
        out["dWres"] = dW[3]
    return out


def steady_dY(X, W, dY, H, flags):
    """dY with zeros where the fp64 pre-activation is within 1e-4 of the ReLU's kink (see the module docstring)."""
    use_scale, residual, relu = flags
    if not relu:
        return dY
    pre = mhsa_reference(X, W[0], W[1], W[2], W[3], H, use_scale, residual, False)
    return dY * (pre.abs() >= 1e-4)


def check_against_fp64(tag, X, W, dY, H, flags, record_pad=0, accumulate=False):
    dY = steady_dY(X, W, dY, H, flags)
    ref = run_torch(X, W, dY, H, flags, torch.float64)
    f32 = run_torch(X, W, dY, H, flags, torch.float32)
    got = run_hip(X, W, dY, H, flags, record_pad, accumulate)
    worst = 0.0
    failures = []
    for name, r in ref.items():
        g = got[name].double().cpu()
        assert bool(torch.isfinite(g).all()), (tag, name)
        e32 = float((f32[name] - r).abs().max())
        bound = 4.0 * e32 + 1e-6 * float(r.abs().max())
        if accumulate and name == "dX":
            bound += 2.0 ** -22          # (3 + dX) - 3 in fp32: one rounding at magnitude <= 4
        err = float((g - r).abs().max())
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print("%s %-6s err %.3e  e32 %.3e  bound %.3e  err/bound %.3f" % (tag, name, err, e32, bound, ratio))
        if not err <= bound:
            failures.append((name, err, bound))
    print("%s worst err/bound %.3f" % (tag, worst))
    assert not failures, (tag, failures)
    return worst


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "scale%d-res%d-relu%d" % tuple(int(v) for v in f))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-F%d-D%d-A%d-H%d" % s)
def test_forward_and_gradients_within_the_fp32_yardstick(shape, flags):
    X, W, dY = make_inputs(shape, flags[1], seed=sum(shape) + 4 * flags[0] + 2 * flags[1] + flags[2])
    check_against_fp64("mhsa %s %s" % (shape, flags), X, W, dY, shape[4], flags)


# The arms of the in-LDS core that SHAPES does not reach (the host's arithmetic, csrc/fx_attn_lds.h: heads per pass
# = min(H, 4160 // (F * (F | 1))); the backward's weights stay in HBM when six [F, A] arrays, X, two score buffers
# and the weights exceed 160 KiB; 16 gradient entries per thread when A * D > 1024):
#   F = 40, H = 3: two heads per pass, so a ragged last group (2 + 1), without and with a W_res;
#   F = D = A = 64: weights in HBM, 16 entries per thread, three matrices; D = 32 with a W_res: four matrices
ARM_CASES = [((5, 40, 6, 12, 3), (True, False, True)), ((5, 40, 6, 12, 3), (True, True, True)),
             ((3, 64, 64, 64, 2), (True, True, True)), ((3, 64, 32, 64, 2), (True, True, True))]


#            (heads per pass, weights in LDS, gradient entries per thread) of the backward
ARM_OF = {(5, 40, 6, 12, 3): (2, True, 1), (3, 64, 64, 64, 2): (1, False, 16), (3, 64, 32, 64, 2): (1, False, 16)}


def backward_arm(shape, n_w):
    """The host's choice for the backward, restated from csrc/fx_attn_lds.h and fx_mhsa.hip: if a limit there moves,
    the cases below stop being the arms they are named for and this says so."""
    B, F, D, A, H = shape
    hg = min(H, (64 * 65) // (F * (F | 1)))
    floats = F * (D | 1) + 6 * F * (A | 1) + 2 * hg * F * (F | 1)
    wlds = 4 * (floats + n_w * A * (D | 1)) <= 160 * 1024
    return hg, wlds, 1 if A * D <= 256 else 4 if A * D <= 1024 else 16


@pytest.mark.parametrize("shape,flags", ARM_CASES, ids=lambda v: "-".join(str(int(x)) for x in v))
def test_ragged_head_groups_and_weights_left_in_hbm(shape, flags):
    X, W, dY = make_inputs(shape, flags[1], seed=6000 + sum(shape) + flags[1])
    assert (W[3] is not None) == (flags[1] and shape[2] != shape[3])
    assert backward_arm(shape, 3 if W[3] is None else 4) == ARM_OF[shape]
    assert shape[4] % ARM_OF[shape][0] != 0 or ARM_OF[shape][1] is False      # a ragged group, or weights in HBM
    check_against_fp64("mhsa arm %s %s" % (shape, flags), X, W, dY, shape[4], flags)


# The weight gradients leave through a row sum over min(B, 512) per-workgroup partials of 3 (4 with W_res) * A * D
# columns, 64 columns per workgroup of four waves: fewer rows than waves, as many, one and five more; the fewest
# columns the layer has, one short of a workgroup's, exactly its 64 (W_res: 4 * 8 * 2), and more than one workgroup
ROWSUM_CASES = [((1, 2, 1, 1, 1), (True, False, False)),        # 1 row, 3 columns
                ((2, 3, 1, 21, 3), (True, False, True)),        # 2 rows, 63 columns
                ((3, 2, 2, 8, 2), (False, True, False)),        # 3 rows, 64 columns
                ((4, 3, 2, 11, 1), (True, False, True)),        # 4 rows, 66 columns
                ((9, 2, 2, 22, 2), (True, False, False))]       # 9 rows, 132 columns


@pytest.mark.parametrize("shape,flags", ROWSUM_CASES, ids=lambda v: "-".join(str(int(x)) for x in v))
def test_weight_gradients_over_few_partial_rows_and_columns(shape, flags):
    X, W, dY = make_inputs(shape, flags[1], seed=5000 + sum(shape))
    n_w = 3 if W[3] is None else 4
    assert ops.mhsa_workspace_floats(shape[0], shape[2], shape[3], n_w == 4) == shape[0] * n_w * shape[3] * shape[2]
    check_against_fp64("mhsa rowsum %s %s" % (shape, flags), X, W, dY, shape[4], flags)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-F%d-D%d-A%d-H%d" % s)
@pytest.mark.parametrize("flags", [(False, True, True), (True, False, False)],
                         ids=lambda f: "scale%d-res%d-relu%d" % tuple(int(v) for v in f))
def test_input_read_in_place_from_a_wider_record(shape, flags):
    """X and dX as [:, :F, :] views of [B, F + 1, D] records: the sample stride is taken as it lies."""
    X, W, dY = make_inputs(shape, flags[1], seed=1000 + sum(shape))
    check_against_fp64("mhsa record %s %s" % (shape, flags), X, W, dY, shape[4], flags, record_pad=1)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[4]], ids=lambda s: "B%d-F%d-D%d-A%d-H%d" % s)
def test_dx_is_added_to_the_buffer_when_asked(shape):
    """dx_accumulate: dX lands on top of what the record-shaped gradient buffer holds (3.0 everywhere)."""
    flags = (False, True, True)
    X, W, dY = make_inputs(shape, True, seed=4000 + sum(shape))
    check_against_fp64("mhsa accumulate %s" % (shape,), X, W, dY, shape[4], flags, record_pad=1, accumulate=True)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=lambda s: "B%d-F%d-D%d-A%d-H%d" % s)
@pytest.mark.parametrize("use_scale", [False, True])
def test_scores_of_plus_minus_80_stay_finite_and_within_the_bound(shape, use_scale):
    flags = (use_scale, True, True)
    peak = 80.0 * ((shape[3] // shape[4]) ** 0.5 if use_scale else 1.0)     # +-80 after the division
    X, W, dY = make_inputs(shape, True, seed=2000 + sum(shape), score_peak=peak)
    check_against_fp64("mhsa peak80 %s scale%d" % (shape, use_scale), X, W, dY, shape[4], flags)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-F%d-D%d-A%d-H%d" % s)
def test_two_launches_give_the_same_bits(shape):
    flags = (True, True, True)
    X, W, dY = make_inputs(shape, True, seed=3000 + sum(shape))
    a = run_hip(X, W, dY, shape[4], flags)
    b = run_hip(X, W, dY, shape[4], flags)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_shapes_beyond_the_limits_are_rejected_with_a_message():
    dev = torch.device("cuda:0")

    def call(B, F, D, A, H):
        x = torch.zeros(B, F, D, device=dev)
        w = torch.zeros(A, D, device=dev)
        ops.mhsa_fwd(x, w, w, w, None, H, False, False, True, torch.zeros(B, F, A, device=dev))
    with pytest.raises(_lib.FxError, match="F=65"):
        call(2, 65, 8, 8, 1)
    with pytest.raises(_lib.FxError, match="A=65"):
        call(2, 10, 8, 65, 1)
    with pytest.raises(_lib.FxError, match="does not divide"):
        call(2, 10, 8, 8, 3)
    call(2, 64, 64, 64, 1)              # the largest shape itself runs
    torch.cuda.synchronize()
