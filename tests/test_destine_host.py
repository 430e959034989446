"""DESTINE on the native layers, host side (no GPU): zoo.DESTINE + layers.DisentangledSelfAttention wired end to end
with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the fx_dsa_* wrappers
emulated here on `dsa_reference`, the layer as the reference writes it — against fixtures recorded from the REAL
reference's model_zoo.DESTINE (tests/golden/make_golden_destine.py).  Checks the parameter names, the forward
composition, the autograd node's plumbing (the order of the ten gradients in dW) and the optimizer protocol; the
HIP kernels themselves are held to fp64 in tests/test_gpu_destine_kernel.py.

Stated tolerances (those of tests/zoo_cases.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

DESTINE_CASES = ["destine_zoo_test", "destine_adam", "destine_last_layer_sgd", "destine_nores_relu", "destine_h3"]


def dsa_reference(X, params, H, use_scale, relu_before_att, dtype=None):
    """DisentangledSelfAttention.forward (DESTINE.py:190-227) in plain torch, with its flat view(B H, -1, hd).
    params = (Wq, Wk, Wv, Wres | None, Wu, bq, bk, bv, bres | None, bu); dtype converts X and params first."""
    if dtype is not None:
        X, params = X.to(dtype), [None if t is None else t.to(dtype) for t in params]
    (Wq, Wk, Wv, Wres, Wu), (bq, bk, bv, bres, bu) = params[:5], params[5:]
    B, A = X.shape[0], Wq.shape[0]
    hd = A // H
    unary = X @ Wu.t() + bu
    query, key, value = X @ Wq.t() + bq, X @ Wk.t() + bk, X @ Wv.t() + bv
    if relu_before_att:
        query, key, value = query.relu(), key.relu(), value.relu()
    query, key, value = (t.reshape(B * H, -1, hd) for t in (query, key, value))
    mu_query = query - query.mean(dim=1, keepdim=True)
    mu_key = key - key.mean(dim=1, keepdim=True)
    pair = torch.bmm(mu_query, mu_key.transpose(1, 2))
    if use_scale:
        pair = pair / hd ** 0.5
    pair = pair.softmax(dim=2)
    un = unary.softmax(dim=1).reshape(B * H, -1, 1).transpose(1, 2)
    out = torch.bmm(pair + un, value).reshape(B, -1, A)
    return out + (X @ Wres.t() + bres) if Wres is not None else out


def _emul_dsa_fwd(X, W, bias, H, use_scale, relu_before_att, Y):
    with torch.no_grad():
        Y.copy_(dsa_reference(X, list(W) + list(bias), H, use_scale, relu_before_att))
    return Y


def _emul_dsa_bwd(X, W, bias, H, use_scale, relu_before_att, dY, dX, dW, workspace, dx_accumulate=False):
    with torch.enable_grad():
        leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in [X] + list(W) + list(bias)]
        y = dsa_reference(leaves[0], leaves[1:], H, use_scale, relu_before_att)
        live = [t for t in leaves if t is not None]
        grads = dict(zip((id(t) for t in live), torch.autograd.grad(y, live, dY)))
    with torch.no_grad():
        if dx_accumulate:
            dX.add_(grads[id(leaves[0])])
        else:
            dX.copy_(grads[id(leaves[0])])
        # fx_dsa_bwd's order: dWq | dWk | dWv (| dWres) | dWu | dbq | dbk | dbv (| dbres) | dbu
        order = [leaves[i] for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10) if leaves[i] is not None]
        dW.copy_(torch.cat([grads[id(t)].reshape(-1) for t in order]))
    return dX, dW


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "dsa_fwd", _emul_dsa_fwd)
    monkeypatch.setattr(ops, "dsa_bwd", _emul_dsa_bwd)
    monkeypatch.setattr(ops, "dsa_workspace_floats", lambda B, D, A, H, has_wres: 1)


def build_destine(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.DESTINE with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_destine.py)."""
    m = g.meta
    return build_from_golden(zoo.DESTINE, g, tmp_path, gpu=gpu, attention_dim=m["attention_dim"],
                             num_heads=m["heads"], attention_layers=m["layers"], dnn_hidden_units=m["hidden"],
                             net_dropout=0, att_dropout=0, relu_before_att=m["relu_before_att"],
                             batch_norm=m["batch_norm"], use_scale=m["use_scale"], use_wide=m["use_wide"],
                             residual_mode=m["residual_mode"], **extra)


def _build(g, tmp_path, monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_destine(zoo, g, tmp_path)


@pytest.mark.parametrize("case", DESTINE_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    assert "self_attns.0.W_unary.bias" in g.state0 and "attn_fc.weight" in g.state0
    assert ("W_res.bias" in g.state0) == (g.meta["residual_mode"] == "last_layer")
    m = g.meta
    assert 0.05 <= m["pair_peak_median"] <= 0.5 and m["unary_peak_median"] >= 0.01      # the generator's asserts
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", DESTINE_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    check_trajectory(_build(g, tmp_path, monkeypatch), g)


def test_limits_and_unsupported_options_raise(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers, ops
    lim = ops.dsa_limits()
    assert (lim["F_max"], lim["D_max"], lim["A_max"], lim["H_max"]) == (64, 64, 64, 16)
    with pytest.raises(NotImplementedError, match="dropout_rate"):
        layers.DisentangledSelfAttention(16, 16)                              # the reference's default, 0.1
    with pytest.raises(NotImplementedError, match="embedding_dim <= 64"):
        layers.DisentangledSelfAttention(65, 16, dropout_rate=0)
    with pytest.raises(NotImplementedError, match="attention_dim <= 64"):
        layers.DisentangledSelfAttention(16, 65, num_heads=5, dropout_rate=0)
    with pytest.raises(NotImplementedError, match="num_heads <= 16"):
        layers.DisentangledSelfAttention(16, 34, num_heads=17, dropout_rate=0)
    with pytest.raises(ValueError, match="3 heads"):
        layers.DisentangledSelfAttention(16, 16, num_heads=3, dropout_rate=0)
    layer = layers.DisentangledSelfAttention(8, 8, dropout_rate=0)
    assert layer.W_res is not None and layer.W_res.bias is not None       # a Linear even at equal widths
    assert layers.DisentangledSelfAttention(8, 8, dropout_rate=0, use_residual=False).W_res is None
    x = torch.zeros(2, 5, 8)
    with pytest.raises(NotImplementedError, match="same tensor"):
        layer(x, x.clone(), x)
    with pytest.raises(NotImplementedError, match="same tensor"):
        layer(x, x, x.clone())
    with pytest.raises(NotImplementedError, match="fields <= 64"):
        big = torch.zeros(2, 65, 8)
        layer(big, big, big)
    assert tuple(layer(x, x, x).shape) == (2, 5, 8)


def test_entry_points_are_declared_and_validate_before_the_device():
    import ctypes
    from fuxictr_amd import _lib
    for name in ("fx_dsa_fwd", "fx_dsa_bwd", "fx_dsa_workspace_floats", "fx_dsa_limits"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    tab = (ctypes.c_void_p * 5)()

    def fwd(F, D, A, H, W=tab):
        return lib.fx_dsa_fwd(None, F * D, 4, F, D, W, tab, A, H, 0, 0, None, None)
    assert fwd(65, 8, 8, 1) == 1 and b"F <= 64" in lib.fx_last_error()
    assert fwd(10, 8, 65, 1) == 1 and b"A <= 64" in lib.fx_last_error()
    assert fwd(10, 8, 34, 17) == 1 and b"H <= 16" in lib.fx_last_error()
    assert fwd(10, 8, 8, 3) == 1 and b"does not divide" in lib.fx_last_error()
    assert fwd(10, 8, 8, 2, None) == 1 and b"pointer tables" in lib.fx_last_error()
    assert fwd(10, 8, 8, 2) == 1 and b"null X" in lib.fx_last_error()
    st = lib.fx_dsa_bwd(None, 80, 4, 10, 65, tab, tab, 8, 1, 0, 0, None, None, 80, 0, None, None, None)
    assert st == 1 and b"D_in <= 64" in lib.fx_last_error()
    # one partial row per workgroup: (3 | 4) [A, D] matrices and Wu [H, D], each with its bias
    assert lib.fx_dsa_workspace_floats(4096, 16, 16, 2, 1) == 512 * (4 * 16 + 2) * 17
    assert lib.fx_dsa_workspace_floats(7, 8, 16, 4, 0) == 7 * (3 * 16 + 4) * 9
