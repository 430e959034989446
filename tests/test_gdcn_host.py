"""GDCN and GDCNP on the native layers, host side (no GPU): zoo.GDCN / zoo.GDCNP + layers.GateCrossLayer wired end to
end with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the two
fx_gate_cross_* wrappers emulated here from their formulas in fp32 torch (checked against torch autograd below) —
against fixtures recorded from the REAL reference's model_zoo.GDCN (tests/golden/make_golden_gdcn.py).  Checks the
parameter names, the fused composition (one node for the whole stack: one GEMM + one gate_cross_fwd per layer
forward, one gate_cross_bwd + one gemm_dw_dx per layer backward), the module-by-module one, the packed weight
storage and the optimizer protocol; the HIP kernels themselves are held to an fp64 restatement in
tests/test_gpu_gatecross.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, losses 1e-4 per step, trained weights
through conftest.assert_weights_close."""
import numpy as np
import pytest
import torch

import _cpu_emul
from conftest import Golden, assert_weights_close
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

GDCN_CASES = ["gdcn_adam", "gdcnp_adam", "gdcn_d10_sgd", "gdcnp_one_layer", "gdcnp_zoo_test"]


# ---- the formulas, in the dtype of the arguments ----------------------------------------------------------
def gate_cross_reference(x0, ws, wgs, bs):
    """x_{i+1} = x_0 * (W_i x_i + b_i) * sigmoid(Wg_i x_i) + x_i over the layers -> x_n (GDCN.py:197-211)"""
    x = x0
    for W, Wg, b in zip(ws, wgs, bs):
        x = x0 * (x @ W.t() + b) * torch.sigmoid(x @ Wg.t()) + x
    return x


def gate_cross_fwd_reference(h, x0, xi, b):
    """one layer behind its GEMM: h = [W x_i | Wg x_i]"""
    cols = x0.shape[1]
    return x0 * (h[:, :cols] + b) * torch.sigmoid(h[:, cols:]) + xi


def gate_cross_bwd_reference(dxn, h, x0, b):
    """-> (dh, the layer's share of dx0 without the residual)"""
    cols = x0.shape[1]
    u, g = h[:, :cols] + b, torch.sigmoid(h[:, cols:])
    t = dxn * x0
    return torch.cat([t * g, t * u * g * (1.0 - g)], dim=1), dxn * u * g


# ---- emulations of the two ops ------------------------------------------------------------------------------
CALLS = {"gemm": 0, "gemm_dw_dx": 0, "gate_cross_fwd": 0, "gate_cross_bwd": 0}


def _emul_gate_cross_fwd(h, x0, xi, b, xn):
    CALLS["gate_cross_fwd"] += 1
    with torch.no_grad():
        xn.copy_(gate_cross_fwd_reference(h, x0, xi, b))
    return xn


def _emul_gate_cross_bwd(dxn, h, x0, b, dh, dx0, init, add_dxn):
    CALLS["gate_cross_bwd"] += 1
    with torch.no_grad():
        d, term = gate_cross_bwd_reference(dxn, h, x0, b)
        dh.copy_(d)
        if add_dxn:
            term = term + dxn
        dx0.copy_(term) if init else dx0.add_(term)
    return dh, dx0


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "gate_cross_fwd", _emul_gate_cross_fwd)
    monkeypatch.setattr(ops, "gate_cross_bwd", _emul_gate_cross_bwd)
    gemm, gemm_dw_dx = ops.gemm, ops.gemm_dw_dx

    def counted_gemm(*a, **kw):
        CALLS["gemm"] += 1
        return gemm(*a, **kw)

    def counted_gemm_dw_dx(*a, **kw):
        CALLS["gemm_dw_dx"] += 1
        return gemm_dw_dx(*a, **kw)
    monkeypatch.setattr(ops, "gemm", counted_gemm)
    monkeypatch.setattr(ops, "gemm_dw_dx", counted_gemm_dw_dx)


def build_gdcn(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.GDCN / zoo.GDCNP with a fixture's hyper-parameters and initial weights (shared with
    tests/test_gpu_gdcn.py)."""
    m = g.meta
    return build_from_golden(zoo.GDCNP if m["model"] == "GDCNP" else zoo.GDCN, g, tmp_path, gpu=gpu,
                             dnn_hidden_units=m["dnn"], dnn_activations="relu", num_cross_layers=m["n_cross"], **extra)


def _install_all(monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return zoo


def _build(g, tmp_path, monkeypatch, **extra):
    return build_gdcn(_install_all(monkeypatch), g, tmp_path, **extra)


def _aliases_packed(layer):
    for i, p in enumerate(layer._packed):
        D = p.shape[1]
        assert tuple(p.shape) == (2 * D, D)
        w, wg = layer.w[i].weight, layer.wg[i].weight
        assert w.data_ptr() == p.data_ptr() and wg.data_ptr() == p[D:].data_ptr()
        assert torch.equal(w.detach(), p[:D]) and torch.equal(wg.detach(), p[D:])
    return True


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", GDCN_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    m = g.meta
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts keys, shapes, dtypes)
    width = sum(v.shape[1] if v.shape[1] > 1 else v.shape[0] for k, v in g.state0.items()
                if k.startswith("embedding_layer.") and v.ndim == 2)
    assert width == model.feature_map.sum_emb_out_dim()
    for i in range(m["n_cross"]):
        assert g.state0["cross_net.w.%d.weight" % i].shape == (width, width)
        assert g.state0["cross_net.wg.%d.weight" % i].shape == (width, width)
        assert g.state0["cross_net.b.%d" % i].shape == (width,)
    assert not any(k.startswith("cross_net.") and k.endswith(".bias") for k in g.state0)     # neither Linear has one
    assert ("fc.weight" in g.state0) == (m["model"] == "GDCNP")
    if m["model"] == "GDCNP":
        assert g.state0["fc.weight"].shape == (1, width + m["dnn"][-1])
    assert _aliases_packed(model.cross_net)                          # still, after load_state_dict
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", GDCN_CASES)
def test_training_trajectory_and_trained_weights(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)
    check_trajectory(model, g)
    assert _aliases_packed(model.cross_net)                          # the optimizer updated the packed storage


@pytest.mark.parametrize("case", GDCN_CASES)
def test_fused_and_module_by_module_routes_agree(case, tmp_path, monkeypatch):
    g = Golden(case)
    a = _build(g, tmp_path, monkeypatch, fused=True)
    b = _build(g, tmp_path, monkeypatch, fused=False)
    assert a._fused and a.cross_net.fused and not b._fused and not b.cross_net.fused
    a.train(), b.train()
    for i in range(g.meta["steps"]):
        la, lb = float(a.train_step(tb(g.batches[i])).item()), float(b.train_step(tb(g.batches[i])).item())
        assert abs(la - lb) <= 1e-5, (i, la, lb)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert_weights_close(sa[k].numpy(), sb[k].numpy(), g.meta["lr"], g.meta["steps"], k)


def test_fused_switch_follows_the_environment(tmp_path, monkeypatch):
    for case in ("gdcn_adam", "gdcnp_adam"):
        g = Golden(case)
        monkeypatch.setenv("FX_GDCN_FUSED", "0")
        assert not _build(g, tmp_path, monkeypatch)._fused
        assert _build(g, tmp_path, monkeypatch, fused=True)._fused
        monkeypatch.delenv("FX_GDCN_FUSED")
        model = _build(g, tmp_path, monkeypatch)
        assert model._fused and model.cross_net.fused


def test_an_empty_tower_raises_and_the_defaults_are_the_references(tmp_path, monkeypatch):
    zoo = _install_all(monkeypatch)
    import inspect
    from fuxictr_amd import layers
    from fuxictr_amd.features import FeatureMap
    g = Golden("gdcn_adam")
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": 8})
    kw = dict(gpu=-1, embedding_dim=8, optimizer="adam", loss="binary_crossentropy", task="binary_classification",
              metrics=["AUC"], verbose=0, model_root=str(tmp_path))
    for cls in (zoo.GDCN, zoo.GDCNP):
        with pytest.raises(ValueError, match="dnn_hidden_units"):
            cls(fmap, **kw)                                              # the default is []
        with pytest.raises(ValueError, match="dnn_hidden_units"):
            cls(fmap, dnn_hidden_units=[], **kw)
        sig = inspect.signature(cls.__init__).parameters
        assert sig["embedding_dim"].default == 10 and sig["dnn_hidden_units"].default == []
        assert sig["num_cross_layers"].default == 3 and sig["dnn_activations"].default == "ReLU"
        assert sig["model_id"].default == cls.__name__ and sig["batch_norm"].default is False
    assert layers.GateCorssLayer is layers.GateCrossLayer               # the reference's spelling
    sig = inspect.signature(layers.GateCrossLayer.__init__).parameters
    assert list(sig)[1:] == ["input_dim", "cn_layers"] and sig["cn_layers"].default == 3
    model = zoo.GDCNP(fmap, dnn_hidden_units=[16, 8], **kw)
    for name in ("embedding_layer", "dnn", "cross_net", "fc"):
        assert hasattr(model, name)
    assert isinstance(model.cross_net, layers.GateCrossLayer) and model.cross_net.cn_layers == 3
    assert not hasattr(zoo.GDCN(fmap, dnn_hidden_units=[16, 8], **kw), "fc")


def test_emulated_ops_match_torch_autograd():
    """The emulations above (= the kernels' formulas) against autograd of the forward formula, all flag pairs."""
    gen = torch.Generator().manual_seed(3)
    B, D = 7, 5
    for init in (True, False):
        for add_dxn in (True, False):
            h = torch.randn(B, 2 * D, generator=gen).requires_grad_(True)
            x0 = torch.randn(B, D, generator=gen).requires_grad_(True)
            xi = torch.randn(B, D, generator=gen)
            b = torch.randn(D, generator=gen)
            dxn = torch.randn(B, D, generator=gen)
            xn = gate_cross_fwd_reference(h, x0, xi, b)
            want_dh, want_dx0 = torch.autograd.grad(xn, [h, x0], dxn)
            got = torch.empty(B, D)
            _emul_gate_cross_fwd(h.detach(), x0.detach(), xi, b, got)
            assert torch.allclose(got, xn.detach(), atol=1e-6)
            dh, dx0 = torch.empty(B, 2 * D), torch.full((B, D), 3.0)
            _emul_gate_cross_bwd(dxn, h.detach(), x0.detach(), b, dh, dx0, init, add_dxn)
            want = want_dx0 + (dxn if add_dxn else 0.0) + (0.0 if init else 3.0)
            assert torch.allclose(dh, want_dh, atol=1e-5) and torch.allclose(dx0, want, atol=1e-5)


def _layer(layers, D, n, seed):
    torch.manual_seed(seed)
    layer = layers.GateCrossLayer(D, n)
    with torch.no_grad():
        for lin in list(layer.w) + list(layer.wg):
            lin.weight.copy_(torch.randn(D, D) / D ** 0.5)
    return layer


@pytest.mark.parametrize("n", [1, 2, 3])
def test_gate_cross_layer_alone_matches_the_fp64_restatement_with_the_stated_launches(n, monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    B, D = 9, 6
    layer = _layer(layers, D, n, seed=10 + n)
    assert sorted(layer.state_dict()) == sorted(["w.%d.weight" % i for i in range(n)] +
                                                ["wg.%d.weight" % i for i in range(n)] + ["b.%d" % i for i in range(n)])
    for i in range(n):
        bi = layer.b[i].detach()                                        # uniform(0, 1), as the reference draws it
        assert bool(((bi >= 0) & (bi < 1)).all()) and float(bi.std()) > 0
    x = torch.randn(B, D)
    gy = torch.randn(B, D)
    params = [p for i in range(n) for p in (layer.w[i].weight, layer.wg[i].weight, layer.b[i])]
    x64 = x.double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    want = gate_cross_reference(x64, p64[0::3], p64[1::3], p64[2::3])
    want_g = torch.autograd.grad(want, [x64] + p64, gy.double())
    for fused in (True, False):
        layer.fused = fused
        xin = x.clone().requires_grad_(True)
        for k in CALLS:
            CALLS[k] = 0
        got = layer(xin)
        fwd = dict(CALLS)
        got_g = torch.autograd.grad(got, [xin] + params, gy)
        assert torch.allclose(got.detach().double(), want.detach(), atol=1e-5)
        for a, b in zip(got_g, want_g):
            assert a.shape == b.shape and torch.allclose(a.double(), b, atol=1e-4), (fused, (a - b).abs().max())
        if fused:
            # forward: one GEMM and one gate_cross_fwd per layer; backward: one gate_cross_bwd and one dW + dX pair
            assert fwd == {"gemm": n, "gemm_dw_dx": 0, "gate_cross_fwd": n, "gate_cross_bwd": 0}
            assert CALLS == {"gemm": n, "gemm_dw_dx": n, "gate_cross_fwd": n, "gate_cross_bwd": n}
        else:
            assert fwd["gemm"] == 2 * n and fwd["gate_cross_fwd"] == 0 and CALLS["gate_cross_bwd"] == 0


def test_out_into_receives_the_last_layer_and_nothing_else(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    B, D, H = 5, 6, 3
    for n in (1, 2):
        layer = _layer(layers, D, n, seed=20 + n)
        x = torch.randn(B, D)
        want = layer(x).detach()
        buf = torch.full((B, D + H), 7.0)
        got = layer(x, out_into=buf[:, :D])
        assert got.data_ptr() == buf.data_ptr() and torch.equal(got.detach(), want)
        assert torch.equal(buf[:, :D], want) and bool((buf[:, D:] == 7.0).all())


def test_weights_alias_the_packed_storage_after_to_and_load_state_dict(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    D, n = 6, 2
    layer = _layer(layers, D, n, seed=30)
    assert _aliases_packed(layer)
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    layer.to(torch.float64)
    assert layer._packed[0].dtype == torch.float64 and layer.b[0].dtype == torch.float64 and _aliases_packed(layer)
    layer.to(torch.float32)
    assert _aliases_packed(layer)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, before[k]), k
    sd = {k: torch.randn_like(v) for k, v in before.items()}
    layer.load_state_dict(sd)
    assert _aliases_packed(layer)
    for i in range(n):
        assert torch.equal(layer._packed[i][:D], sd["w.%d.weight" % i])
        assert torch.equal(layer._packed[i][D:], sd["wg.%d.weight" % i])
    # an in-place update of a Parameter (what the optimizer does) is an update of the storage the GEMM reads
    with torch.no_grad():
        layer.wg[1].weight.add_(1.0)
    assert torch.equal(layer._packed[1][D:], sd["wg.1.weight"] + 1.0)


def test_gdcnp_writes_both_towers_into_one_buffer_and_falls_back_to_cat(tmp_path, monkeypatch):
    """The plain Linear / ReLU tower takes `out_into`: fc reads [cross | deep] from one buffer and no torch.cat runs;
    with batch_norm the tower's result is its own tensor and the cat joins them: the same numbers."""
    g = Golden("gdcnp_adam")
    model = _build(g, tmp_path, monkeypatch, fused=True)
    cats = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **kw: (cats.append(1), real_cat(*a, **kw))[1])
    seen = []
    model.fc.register_forward_pre_hook(lambda m, inp: seen.append(inp[0]))
    model.eval()
    with torch.no_grad():
        model.forward(tb(g.batches[0]))
    n_fused = len(cats)
    D0, H = model.feature_map.sum_emb_out_dim(), g.meta["dnn"][-1]
    assert tuple(seen[-1].shape) == (g.meta["B"], D0 + H) and seen[-1].is_contiguous()
    model._fused = False
    model.cross_net.fused = False
    with torch.no_grad():
        model.forward(tb(g.batches[0]))
    assert len(cats) - n_fused == n_fused + 1                      # exactly one more: the join of the two towers
    assert torch.allclose(seen[-1], seen[-2], atol=1e-5)


def test_fixtures_exercise_the_gates_and_the_cross_weights():
    """What make_golden_gdcn.py asserted when it wrote the fixtures, re-checked from the committed files."""
    for case in GDCN_CASES:
        g = Golden(case)
        m = g.meta
        loss = list(g.expect["loss"])
        assert all(a != b for a, b in zip(loss, loss[1:])), (case, loss)
        assert len(m["gate_spread"]) == m["n_cross"] and all(s >= 0.2 for s in m["gate_spread"]), case
        assert m["gate_share"] >= 0.05 and m["w_share"] >= 0.05, case
        for i in range(m["n_cross"]):
            k = "cross_net.b.%d" % i
            assert not np.array_equal(g.state0[k], g.state1[k]), (case, k)
        assert m["B"] == 64 and m["steps"] == 3
    m = Golden("gdcn_d10_sgd").meta
    width = m["embedding_dim"] * (m["n_dense"] + len(m["cards"]))
    assert width % 4 != 0 and m["net_reg"] > 0 and m["optimizer"] == "SGD"          # the scalar arm
    assert Golden("gdcnp_one_layer").meta["n_cross"] == 1
    m = Golden("gdcnp_zoo_test").meta
    assert (m["embedding_dim"], m["dnn"], m["n_cross"], m["emb_reg"], m["lr"]) == (4, [64, 32], 3, 1e-8, 1e-3)
    import os
    from conftest import GOLDEN
    largest = os.path.getsize(os.path.join(GOLDEN, "masknet_parallel_adam.npz"))
    for case in GDCN_CASES:
        assert os.path.getsize(os.path.join(GOLDEN, case + ".npz")) <= largest, case


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib
    for name in ("fx_gate_cross_fwd", "fx_gate_cross_bwd", "fx_gate_cross_tile_rows"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.fx_gate_cross_tile_rows() >= 1
    one = 16        # (any non-null address: validation happens before anything is read)
    st = lib.fx_gate_cross_fwd(one, 16, one, 8, one, 8, one, one, 8, 4, 0, None)
    assert st == 1 and b"cols=0" in lib.fx_last_error()
    st = lib.fx_gate_cross_fwd(None, 16, one, 8, one, 8, one, one, 8, 4, 8, None)
    assert st == 1 and b"null h" in lib.fx_last_error()
    st = lib.fx_gate_cross_fwd(one, 15, one, 8, one, 8, one, one, 8, 4, 8, None)
    assert st == 1 and b"h row stride" in lib.fx_last_error()
    st = lib.fx_gate_cross_fwd(one, 16, one, 8, one, 7, one, one, 8, 4, 8, None)
    assert st == 1 and b"xi row stride" in lib.fx_last_error()
    st = lib.fx_gate_cross_fwd(one, 16, one, 8, one, 8, None, one, 8, 4, 8, None)
    assert st == 1 and b"null b" in lib.fx_last_error()
    st = lib.fx_gate_cross_fwd(one, 16, one, 8, one, 8, one, one, 8, -1, 8, None)
    assert st == 1 and b"rows=-1" in lib.fx_last_error()
    assert lib.fx_gate_cross_fwd(one, 16, one, 8, one, 8, one, one, 8, 0, 8, None) == 0          # no rows: no launch
    st = lib.fx_gate_cross_bwd(one, 7, one, 16, one, 8, one, one, 16, one, 8, 4, 8, 1, 0, None)
    assert st == 1 and b"dxn row stride" in lib.fx_last_error()
    st = lib.fx_gate_cross_bwd(one, 8, one, 16, one, 8, one, one, 12, one, 8, 4, 8, 1, 0, None)
    assert st == 1 and b"dh row stride" in lib.fx_last_error()
    st = lib.fx_gate_cross_bwd(one, 8, one, 16, one, 8, one, one, 16, None, 8, 4, 8, 1, 0, None)
    assert st == 1 and b"null dx0" in lib.fx_last_error()
    assert lib.fx_gate_cross_bwd(one, 8, one, 16, one, 8, one, one, 16, one, 8, 0, 8, 1, 0, None) == 0
