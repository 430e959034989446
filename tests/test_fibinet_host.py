"""FiBiNET on the native layers, host side (no GPU): zoo.FiBiNET + layers.SqueezeExcitation / BilinearInteractionV2
wired end to end with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the
fx_senet_* / fx_bilinear_* wrappers emulated here from their formulas — against fixtures recorded from the REAL
reference's model_zoo.FiBiNET (tests/golden/make_golden_fibinet.py).  Checks the parameter names (the frozen
`triu_index` included), the fused composition (gates only, two branches into one padded buffer, the linear part in
the tower's epilogue), the unfused one, the autograd nodes' plumbing and the optimizer protocol; the HIP kernels
themselves are held to an fp64 restatement in tests/test_gpu_bilinear.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, losses 1e-4 per step, trained weights
through conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden, assert_weights_close
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

FIBINET_CASES = ["fibinet_adam", "fibinet_zoo_test", "fibinet_each_sigmoid_sgd", "fibinet_all_nodnn"]


def senet_reference(X, W1, W2, act):
    """-> (A, V) from the layer's formulas, in the dtype and on the device of the arguments."""
    Z = X.mean(dim=-1)
    A = torch.relu(Z @ W1.t()) @ W2.t()
    A = torch.relu(A) if act == 0 else torch.sigmoid(A)
    return A, X * A.unsqueeze(-1)


def bilinear_reference(X, W, kind, A=None):
    """-> [B, P, D]: ((a_i x_i) W_w) * (a_j x_j) over the pairs i < j in triu order."""
    F = X.shape[1]
    V = X if A is None else X * A.unsqueeze(-1)
    iu = torch.triu_indices(F, F, 1)
    left, right = V[:, iu[0]], V[:, iu[1]]
    if kind == 0:
        y = left @ W
    elif kind == 1:
        y = torch.einsum("bpd,pde->bpe", left, W[iu[0]])
    else:
        y = torch.einsum("bpd,pde->bpe", left, W)
    return y * right


def _emul_senet_fwd(X, W1, W2, act, A, V=None):
    with torch.no_grad():
        a, v = senet_reference(X, W1, W2, act)
        A.copy_(a)
        if V is not None:
            V.copy_(v)
    return A


def _emul_senet_bwd(X, W1, W2, act, A, dA, dV, dX, dW1, dW2, workspace, dx_accumulate=False):
    with torch.enable_grad():
        x, w1, w2 = (t.detach().clone().requires_grad_(True) for t in (X, W1, W2))
        a, v = senet_reference(x, w1, w2, act)
        outs, gs = [], []
        if dA is not None:
            outs.append(a), gs.append(dA)
        if dV is not None:
            outs.append(v), gs.append(dV)
        gx, g1, g2 = torch.autograd.grad(outs, [x, w1, w2], gs)
    with torch.no_grad():
        dX.add_(gx) if dx_accumulate else dX.copy_(gx)
        dW1.copy_(g1)
        dW2.copy_(g2)
    return dX, dW1, dW2


def _emul_bilinear_fwd(X, W, kind, A, out, out_col=0):
    with torch.no_grad():
        y = bilinear_reference(X, W, kind, A).flatten(start_dim=1)
        out[:, out_col:out_col + y.shape[1]].copy_(y)
    return out


def _emul_bilinear_bwd(X, W, kind, A, dOut, dX, dA, dW, workspace, dout_col=0, dx_accumulate=False):
    with torch.enable_grad():
        leaves = [t.detach().clone().requires_grad_(True) for t in (X, W) + ((A,) if A is not None else ())]
        y = bilinear_reference(leaves[0], leaves[1], kind, leaves[2] if A is not None else None)
        n = y.shape[1] * y.shape[2]
        grads = torch.autograd.grad(y, leaves, dOut[:, dout_col:dout_col + n].reshape(y.shape))
    with torch.no_grad():
        dX.add_(grads[0]) if dx_accumulate else dX.copy_(grads[0])
        dW.copy_(grads[1])
        if A is not None:
            dA.copy_(grads[2])
    return dX, dA, dW


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "senet_fwd", _emul_senet_fwd)
    monkeypatch.setattr(ops, "senet_bwd", _emul_senet_bwd)
    monkeypatch.setattr(ops, "bilinear_fwd", _emul_bilinear_fwd)
    monkeypatch.setattr(ops, "bilinear_bwd", _emul_bilinear_bwd)
    monkeypatch.setattr(ops, "senet_workspace_floats", lambda B, F, R: 1)
    monkeypatch.setattr(ops, "bilinear_workspace_floats", lambda B, F, D: 1)


def build_fibinet(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.FiBiNET with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_fibinet.py)."""
    m = g.meta
    return build_from_golden(zoo.FiBiNET, g, tmp_path, gpu=gpu, hidden_units=m["hidden"],
                             excitation_activation=m["excitation"], reduction_ratio=m["ratio"],
                             bilinear_type=m["bilinear_type"], **extra)


def _build(g, tmp_path, monkeypatch, **extra):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_fibinet(zoo, g, tmp_path, **extra)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", FIBINET_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts keys, shapes, dtypes)
    for k in ("senet_layer.excitation.0.weight", "senet_layer.excitation.2.weight",
              "bilinear_interaction1.bilinear_W", "bilinear_interaction2.triu_index"):
        assert k in g.state0, k
    tri = model.bilinear_interaction1.triu_index
    assert tri.dtype == torch.int64 and not tri.requires_grad
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", FIBINET_CASES)
def test_training_trajectory_and_trained_weights(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)
    check_trajectory(model, g)


@pytest.mark.parametrize("case", FIBINET_CASES)
def test_fused_and_unfused_routes_agree(case, tmp_path, monkeypatch):
    g = Golden(case)
    a = _build(g, tmp_path, monkeypatch, fused=True)
    b = _build(g, tmp_path, monkeypatch, fused=False)
    assert a._fused and not b._fused
    a.train(), b.train()
    for i in range(g.meta["steps"]):
        la, lb = float(a.train_step(tb(g.batches[i])).item()), float(b.train_step(tb(g.batches[i])).item())
        assert abs(la - lb) <= 1e-5, (i, la, lb)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert_weights_close(sa[k].numpy(), sb[k].numpy(), g.meta["lr"], g.meta["steps"], k)


def test_fixtures_exercise_both_relus_and_the_senet_branch():
    """What make_golden_fibinet.py asserted when it wrote the fixtures, re-read from their meta."""
    for case in FIBINET_CASES:
        m = Golden(case).meta
        if m["excitation"] == "ReLU":
            assert 0.1 <= m["gate_zero_share"] <= 0.9, (case, m["gate_zero_share"])
        assert 0.1 <= m["hidden_zero_share"] <= 0.9, (case, m["hidden_zero_share"])
        assert m["senet_branch_share"] >= 0.05, (case, m["senet_branch_share"])


def test_layers_alone_match_their_formulas_and_both_bilinear_classes_agree(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    torch.manual_seed(3)
    x = torch.randn(5, 6, 4, requires_grad=True)
    for kind, lead in (("field_all", ()), ("field_each", (6,)), ("field_interaction", (15,))):
        v2 = layers.BilinearInteractionV2(6, 4, kind)
        v1 = layers.BilinearInteraction(6, 4, kind)
        assert tuple(v2.bilinear_W.shape) == lead + (4, 4) and v2.interact_dim == 15
        assert "triu_index" in v2.state_dict() and "triu_index" not in v1.state_dict()
        v1.load_state_dict({"bilinear_W": v2.bilinear_W.detach()})
        assert torch.equal(v1(x), v2(x)) and tuple(v2(x).shape) == (5, 15, 4)
    se = layers.SqueezeExcitation(6, reduction_ratio=3, excitation_activation="Sigmoid")
    assert sorted(se.state_dict()) == ["excitation.0.weight", "excitation.2.weight"]
    assert tuple(se.excitation[0].weight.shape) == (2, 6)
    v = se(x)
    v.sum().backward()
    assert x.grad is not None and se.excitation[0].weight.grad is not None
    assert torch.allclose(v, senet_reference(x, se.excitation[0].weight, se.excitation[2].weight, 1)[1])
    assert layers.SqueezeExcitation(2, reduction_ratio=3).excitation[0].out_features == 1      # R = max(1, .)


def test_limits_and_unknown_options_raise(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    with pytest.raises(NotImplementedError, match="excitation_activation"):
        layers.SqueezeExcitation(10, excitation_activation="Tanh")
    with pytest.raises(NotImplementedError, match="num_fields=65"):
        layers.SqueezeExcitation(65)
    with pytest.raises(NotImplementedError, match="reduced size=65"):
        layers.SqueezeExcitation(26, reduction_ratio=0.4)
    with pytest.raises(NotImplementedError, match="num_fields=65"):
        layers.BilinearInteractionV2(65, 8)
    with pytest.raises(NotImplementedError, match="embedding_dim=65"):
        layers.BilinearInteraction(10, 65)
    with pytest.raises(NotImplementedError, match="bilinear_type"):
        layers.BilinearInteractionV2(10, 8, "field_none")
    with pytest.raises(NotImplementedError, match="built for"):
        layers.BilinearInteractionV2(10, 8)(torch.zeros(2, 9, 8))
    with pytest.raises(NotImplementedError, match="dim <= 64"):
        layers.SqueezeExcitation(4)(torch.zeros(2, 4, 65))


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib, patch
    names = ("fx_senet_fwd", "fx_senet_bwd", "fx_senet_workspace_floats", "fx_bilinear_fwd", "fx_bilinear_bwd",
             "fx_bilinear_workspace_floats")
    for name in names:
        assert name in _lib.SIGNATURES
    for name in ("SqueezeExcitation", "BilinearInteraction", "BilinearInteractionV2"):
        assert name in patch.LAYER_NAMES
    lib = _lib.load()
    st = lib.fx_bilinear_fwd(None, 65 * 8, 4, 65, 8, None, 2, None, None, 0, 0, None)
    assert st == 1 and b"F <= 64" in lib.fx_last_error()
    st = lib.fx_bilinear_fwd(None, 10 * 65, 4, 10, 65, None, 2, None, None, 0, 0, None)
    assert st == 1 and b"D <= 64" in lib.fx_last_error()
    st = lib.fx_bilinear_fwd(None, 80, 4, 10, 8, None, 3, None, None, 0, 0, None)
    assert st == 1 and b"bilinear type 3" in lib.fx_last_error()
    st = lib.fx_senet_fwd(None, 80, 4, 10, 8, None, None, 65, 0, None, None, None)
    assert st == 1 and b"R <= 64" in lib.fx_last_error()
    st = lib.fx_senet_bwd(None, 80, 4, 10, 8, None, None, 3, 2, None, None, None, None, 80, 0, None, None, None,
                          None)
    assert st == 1 and b"activation 2" in lib.fx_last_error()
    # one partial per (sample slab, pair); per workgroup for the excitation
    assert lib.fx_bilinear_workspace_floats(4096, 39, 16) % (741 * 256) == 0
    assert lib.fx_bilinear_workspace_floats(1, 2, 8) == 64
    assert lib.fx_senet_workspace_floats(4096, 39, 13) == 256 * 2 * 39 * 13
    assert lib.fx_senet_workspace_floats(5, 10, 3) == 2 * 2 * 30
