"""AutoInt on the native layers, host side (no GPU): zoo.AutoInt + layers.MultiHeadSelfAttention wired end to end
with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the two fx_mhsa_*
wrappers emulated here — against fixtures recorded from the REAL reference's model_zoo.AutoInt
(tests/golden/make_golden_autoint.py).  Checks the parameter names, the forward composition (wide + attention
head + deep tower in the GEMM epilogues), the autograd node's plumbing and the optimizer protocol; the HIP
kernels themselves are held to an fp64 restatement in tests/test_gpu_mhsa.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, losses 1e-4 per step, trained weights
through conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

AUTOINT_CASES = ["autoint_adam", "autoint_zoo_test", "autoint_scale_wide_sgd", "autoint_nores_nodnn",
                 "autoint_layernorm"]


def _attend(X, Wq, Wk, Wv, Wres, H, use_scale, residual, relu):
    """The layer in plain torch ops, from its formulas: -> Y [B, F, A]."""
    B, F, _ = X.shape
    A = Wq.shape[0]
    hd = A // H

    def heads(W):
        return (X @ W.t()).view(B, F, H, hd).permute(0, 2, 1, 3)          # [B, H, F, hd]
    Q, K, V = heads(Wq), heads(Wk), heads(Wv)
    S = Q @ K.transpose(-1, -2)
    if use_scale:
        S = S / hd ** 0.5
    P = torch.softmax(S, dim=-1)
    Y = (P @ V).permute(0, 2, 1, 3).reshape(B, F, A)
    if residual:
        Y = Y + (X @ Wres.t() if Wres is not None else X)
    if relu:
        Y = torch.relu(Y)
    return Y


def _emul_mhsa_fwd(X, Wq, Wk, Wv, Wres, H, use_scale, residual, relu, Y):
    with torch.no_grad():
        Y.copy_(_attend(X, Wq, Wk, Wv, Wres, H, use_scale, residual, relu))
    return Y


def _emul_mhsa_bwd(X, Wq, Wk, Wv, Wres, H, use_scale, residual, relu, Y, dY, dX, dW, workspace,
                   dx_accumulate=False):
    with torch.enable_grad():
        leaves = [t.detach().clone().requires_grad_(True)
                  for t in (X, Wq, Wk, Wv) + ((Wres,) if Wres is not None else ())]
        y = _attend(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4] if Wres is not None else None,
                       H, use_scale, residual, relu)
        grads = torch.autograd.grad(y, leaves, dY)
    with torch.no_grad():
        if dx_accumulate:
            dX.add_(grads[0])
        else:
            dX.copy_(grads[0])
        for i, g in enumerate(grads[1:]):
            dW[i].copy_(g)
    return dX, dW


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "mhsa_fwd", _emul_mhsa_fwd)
    monkeypatch.setattr(ops, "mhsa_bwd", _emul_mhsa_bwd)
    monkeypatch.setattr(ops, "mhsa_workspace_floats", lambda B, D, A, has_wres: 1)


def build_autoint(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.AutoInt with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_autoint.py)."""
    m = g.meta
    return build_from_golden(zoo.AutoInt, g, tmp_path, gpu=gpu, dnn_hidden_units=m["hidden"],
                             attention_layers=m["layers"], num_heads=m["heads"], attention_dim=m["attention_dim"],
                             layer_norm=m["layer_norm"], use_scale=m["use_scale"], use_wide=m["use_wide"],
                             use_residual=m["use_residual"], **extra)


def _build(g, tmp_path, monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_autoint(zoo, g, tmp_path)


@pytest.mark.parametrize("case", AUTOINT_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    assert any(k.startswith("self_attention.0.W_q.") for k in g.state0)
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", AUTOINT_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)
    check_trajectory(model, g)


def test_fixtures_exercise_softmax_and_relu():
    """What make_golden_autoint.py asserted when it wrote the fixtures, re-read from their meta."""
    for case in AUTOINT_CASES:
        m = Golden(case).meta
        peaks, zeros = m["attention_peak_median"], m["relu_zero_share"]
        assert 0.05 <= peaks[0] <= 0.5 and all(p >= 0.01 for p in peaks[1:]), (case, peaks)
        assert all(0.1 <= z <= 0.9 for z in zeros), (case, zeros)


def test_limits_and_unsupported_options_raise(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    with pytest.raises(NotImplementedError, match="input_dim <= 64"):
        layers.MultiHeadSelfAttention(65, attention_dim=16)
    with pytest.raises(NotImplementedError, match="attention_dim <= 64"):
        layers.MultiHeadSelfAttention(16, attention_dim=65, num_heads=5)
    with pytest.raises(NotImplementedError, match="dropout_rate"):
        layers.MultiHeadSelfAttention(16, dropout_rate=0.1)
    with pytest.raises(ValueError, match="3 heads"):
        layers.MultiHeadSelfAttention(16, attention_dim=16, num_heads=3)
    layer = layers.MultiHeadSelfAttention(8, attention_dim=8)
    with pytest.raises(NotImplementedError, match="fields <= 64"):
        layer(torch.zeros(2, 65, 8))
    assert layer.W_res is None and layers.MultiHeadSelfAttention(8, attention_dim=16).W_res is not None


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib
    for name in ("fx_mhsa_fwd", "fx_mhsa_bwd", "fx_mhsa_workspace_floats"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    none = (None,) * 4
    st = lib.fx_mhsa_fwd(None, 65 * 8, 4, 65, 8, *none, 8, 1, 0, 1, 1, None, None)
    assert st == 1 and b"F <= 64" in lib.fx_last_error()
    st = lib.fx_mhsa_fwd(None, 80, 4, 10, 8, *none, 65, 1, 0, 1, 1, None, None)
    assert st == 1 and b"A <= 64" in lib.fx_last_error()
    st = lib.fx_mhsa_bwd(None, 80, 4, 10, 65, *none, 8, 1, 0, 1, 1, None, None, None, 80, 0, None, None, None)
    assert st == 1 and b"D_in <= 64" in lib.fx_last_error()
    st = lib.fx_mhsa_fwd(None, 80, 4, 10, 8, *none, 8, 3, 0, 1, 1, None, None)
    assert st == 1 and b"does not divide" in lib.fx_last_error()
    assert lib.fx_mhsa_workspace_floats(4096, 16, 16, 0) == 512 * 3 * 256
    assert lib.fx_mhsa_workspace_floats(7, 8, 16, 1) == 7 * 4 * 128
