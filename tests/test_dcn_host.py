"""DCN on the native layers, host side (no GPU): zoo.DCN + layers.CrossNet wired end to end with the kernels replaced
by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the two fx_cross_net_* wrappers emulated here from
their formulas in fp32 torch (checked against torch autograd of the plain layer loop below) — against fixtures
recorded from the REAL reference's model_zoo.DCN (tests/golden/make_golden_dcn.py).  Checks the parameter names, the
fused composition (one node for the whole stack: one cross_net_fwd forward, one cross_net_bwd backward), the
module-by-module one and the fallback to it outside the kernels' limits, the packed weight storage, the side-by-side
buffer and the optimizer protocol; the HIP kernels themselves are held to an fp64 restatement in
tests/test_gpu_crossnet.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, predictions atol 2e-5, losses 1e-4 per step,
trained weights through conftest.assert_weights_close."""
import contextlib

import numpy as np
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import LOGIT_TOL, allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

DCN_CASES = ["dcn_adam", "dcn_d10_sgd", "dcn_cross_only", "dcn_one_layer", "dcn_zoo_test"]


# ---- the formulas, in the dtype of the arguments ----------------------------------------------------------
def cross_net_reference(x0, w, b):
    """x_{l+1} = x_l + ((w_l . x_l) * x_0 + b_l) over the rows of w, b [L, cols] -> x_L (cross_net.py:54, 89-92)"""
    x = x0
    for l in range(w.shape[0]):
        x = x + ((x @ w[l:l + 1].t()) * x0 + b[l])
    return x


def cross_net_fwd_reference(x0, w, b):
    """-> (x_L, s [rows, L]): the forward as the kernel states it"""
    x, s = x0, x0.new_empty(x0.shape[0], w.shape[0])
    for l in range(w.shape[0]):
        s[:, l] = (x * w[l]).sum(dim=1)
        x = x + ((s[:, l:l + 1] * x0) + b[l])
    return x, s


def cross_net_bwd_reference(dout, x0, w, b, s):
    """-> (dx0, dw, db) by the recurrences of the backward, x_l recomputed from x0, s and b"""
    L = w.shape[0]
    xs = [x0]
    for l in range(L - 1):
        xs.append(xs[-1] + ((s[:, l:l + 1] * x0) + b[l]))
    g = dout
    dx0 = torch.zeros_like(x0)
    dw, db = torch.zeros_like(w), torch.zeros_like(b)
    for l in range(L - 1, -1, -1):
        t = (g * x0).sum(dim=1, keepdim=True)
        dx0 = dx0 + s[:, l:l + 1] * g
        dw[l] = (t * xs[l]).sum(dim=0)
        db[l] = g.sum(dim=0)
        g = g + t * w[l]
    return dx0 + g, dw, db


# ---- emulations of the two ops ------------------------------------------------------------------------------
CALLS = {"cross_net_fwd": 0, "cross_net_bwd": 0}


def _emul_cross_net_fwd(x0, w, b, out, s=None):
    CALLS["cross_net_fwd"] += 1
    assert tuple(w.shape) == (w.shape[0], x0.shape[1]) and w.shape == b.shape and out.shape == x0.shape
    with torch.no_grad():
        x, dots = cross_net_fwd_reference(x0, w, b)
        out.copy_(x)
        if s is not None:
            s.copy_(dots)
    return out


def _emul_cross_net_bwd(dout, x0, w, b, s, dx0, dw, db, init, workspace):
    CALLS["cross_net_bwd"] += 1
    with torch.no_grad():
        d, gw, gb = cross_net_bwd_reference(dout, x0, w, b, s)
        dx0.copy_(d) if init else dx0.add_(d)
        dw.copy_(gw)
        db.copy_(gb)
    return dx0, dw, db


def _reset_calls():
    for k in CALLS:
        CALLS[k] = 0


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "cross_net_fwd", _emul_cross_net_fwd)
    monkeypatch.setattr(ops, "cross_net_bwd", _emul_cross_net_bwd)


def build_dcn(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.DCN with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_dcn.py)."""
    m = g.meta
    return build_from_golden(zoo.DCN, g, tmp_path, gpu=gpu, dnn_hidden_units=m["dnn"], dnn_activations="relu",
                             num_cross_layers=m["n_cross"], **extra)


def _install_all(monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return zoo


def _build(g, tmp_path, monkeypatch, **extra):
    return build_dcn(_install_all(monkeypatch), g, tmp_path, **extra)


@contextlib.contextmanager
def _counted(want):
    """the launch counters over the block: reset before, `want` after"""
    _reset_calls()
    yield
    assert CALLS == want


def _aliases_packed(layer):
    L = layer.num_layers
    assert tuple(layer._w.shape) == tuple(layer._b.shape) and layer._w.shape[0] == L
    for i, ci in enumerate(layer.cross_net):
        w, b = ci.weight.weight, ci.bias
        assert tuple(w.shape) == (1, layer._w.shape[1]) and tuple(b.shape) == (layer._w.shape[1],)
        assert w.data_ptr() == layer._w[i].data_ptr() and b.data_ptr() == layer._b[i].data_ptr()
        assert torch.equal(w.detach()[0], layer._w[i]) and torch.equal(b.detach(), layer._b[i])
    return True


# ---- the emulations are the formulas --------------------------------------------------------------------------
@pytest.mark.parametrize("init", [True, False], ids=["init", "add"])
@pytest.mark.parametrize("cols", [5, 8])
@pytest.mark.parametrize("L", [1, 3])
def test_emulated_ops_match_torch_autograd(L, cols, init):
    gen = torch.Generator().manual_seed(3 + 10 * L + cols)
    rows = 7
    x0 = torch.randn(rows, cols, generator=gen).requires_grad_(True)
    w = (torch.randn(L, cols, generator=gen) / cols ** 0.5).requires_grad_(True)
    b = torch.randn(L, cols, generator=gen).requires_grad_(True)
    dout = torch.randn(rows, cols, generator=gen)
    want = cross_net_reference(x0, w, b)
    want_dx0, want_dw, want_db = torch.autograd.grad(want, [x0, w, b], dout)
    _reset_calls()
    out, s = torch.empty(rows, cols), torch.empty(rows, L)
    _emul_cross_net_fwd(x0.detach(), w.detach(), b.detach(), out, s)
    assert torch.allclose(out, want.detach(), atol=1e-5)
    bare = torch.empty(rows, cols)
    _emul_cross_net_fwd(x0.detach(), w.detach(), b.detach(), bare, None)          # no stash: the same result
    assert torch.equal(bare, out)
    dx0, dw, db = torch.full((rows, cols), 3.0), torch.empty(L, cols), torch.empty(L, cols)
    _emul_cross_net_bwd(dout, x0.detach(), w.detach(), b.detach(), s, dx0, dw, db, init, None)
    assert torch.allclose(dx0, want_dx0 + (0.0 if init else 3.0), atol=1e-4)
    assert torch.allclose(dw, want_dw, atol=1e-4) and torch.allclose(db, want_db, atol=1e-4)
    assert CALLS == {"cross_net_fwd": 2, "cross_net_bwd": 1}


# ---- zoo.DCN against the reference's fixtures -------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", DCN_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    m = g.meta
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts keys, shapes, dtypes; strict load)
    width = model.feature_map.sum_emb_out_dim()
    assert width == m["embedding_dim"] * (m["n_dense"] + len(m["cards"]))
    for i in range(m["n_cross"]):
        assert g.state0["crossnet.cross_net.%d.weight.weight" % i].shape == (1, width)
        assert g.state0["crossnet.cross_net.%d.bias" % i].shape == (width,)
    assert g.state0["fc.weight"].shape == (1, width + (m["dnn"][-1] if m["dnn"] else 0))
    assert (model.dnn is None) == (not m["dnn"])
    assert any(k.startswith("dnn.") for k in g.state0) == bool(m["dnn"])
    assert _aliases_packed(model.crossnet)                           # still, after load_state_dict
    with _counted({"cross_net_fwd": 1 if fused else 0, "cross_net_bwd": 0}):
        check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", DCN_CASES)
def test_training_trajectory_and_trained_weights(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)
    n = 1 if fused else 0                  # the whole stack: exactly one launch-pair per step, or none of either
    check_trajectory(model, g, per_step=lambda i: _counted({"cross_net_fwd": n, "cross_net_bwd": n}))
    assert _aliases_packed(model.crossnet)                           # the optimizer updated the packed storage
    for i in range(g.meta["n_cross"]):                               # ... and it moved
        assert not np.array_equal(model.crossnet._w[i].numpy(), g.state0["crossnet.cross_net.%d.weight.weight" % i][0])
        assert not np.array_equal(model.crossnet._b[i].numpy(), g.state0["crossnet.cross_net.%d.bias" % i])


def test_fused_switch_follows_the_environment_and_the_defaults_are_the_references(tmp_path, monkeypatch):
    import inspect
    g = Golden("dcn_adam")
    monkeypatch.setenv("FX_DCN_FUSED", "0")
    assert not _build(g, tmp_path, monkeypatch)._fused
    assert _build(g, tmp_path, monkeypatch, fused=True)._fused
    monkeypatch.delenv("FX_DCN_FUSED")
    model = _build(g, tmp_path, monkeypatch)
    assert model._fused and model.crossnet.fused
    from fuxictr_amd import layers, patch, zoo
    sig = inspect.signature(zoo.DCN.__init__).parameters
    assert sig["model_id"].default == "DCN" and sig["embedding_dim"].default == 10 and sig["gpu"].default == -1
    assert sig["dnn_hidden_units"].default == [] and sig["dnn_activations"].default == "ReLU"
    assert sig["num_cross_layers"].default == 3 and sig["net_dropout"].default == 0
    assert sig["batch_norm"].default is False and sig["learning_rate"].default == 1e-3
    assert list(inspect.signature(layers.CrossNet.__init__).parameters)[1:] == ["input_dim", "num_layers"]
    for name in ("embedding_layer", "dnn", "crossnet", "fc"):
        assert hasattr(model, name)
    assert type(model.crossnet) is layers.CrossNet and model.crossnet.num_layers == 3
    assert isinstance(model.fc, layers.FxLinear)
    assert "CrossNet" in patch.LAYER_NAMES
    assert "DCN" in zoo.__doc__


def test_no_cross_layers_returns_the_input_without_a_launch(tmp_path, monkeypatch):
    g = Golden("dcn_adam")
    _install(monkeypatch)
    from fuxictr_amd import layers
    layer = layers.CrossNet(6, 0)
    x = torch.randn(4, 6)
    _reset_calls()
    assert layer(x) is x and not layer.native(x)
    assert list(layer.state_dict()) == [] and CALLS == {"cross_net_fwd": 0, "cross_net_bwd": 0}
    # the model: fc over [x_0 | tower], and it trains
    zoo = _install_all(monkeypatch)
    from fuxictr_amd.features import FeatureMap
    m = g.meta
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": m["embedding_dim"]})
    model = zoo.DCN(fmap, gpu=-1, embedding_dim=m["embedding_dim"], optimizer="adam", loss="binary_crossentropy",
                    task="binary_classification", metrics=["AUC"], verbose=0, model_root=str(tmp_path),
                    dnn_hidden_units=[16, 8], dnn_activations="relu", num_cross_layers=0)
    assert not any(k.startswith("crossnet.") for k in model.state_dict())
    model.train()
    loss = float(model.train_step(tb(g.batches[0])).item())
    assert np.isfinite(loss) and CALLS == {"cross_net_fwd": 0, "cross_net_bwd": 0}


@pytest.mark.parametrize("what", ["max_cols", "max_layers"])
def test_a_shape_above_the_limits_takes_the_module_by_module_route(what, tmp_path, monkeypatch):
    g = Golden("dcn_adam")
    model = _build(g, tmp_path, monkeypatch, fused=True)
    from fuxictr_amd import ops
    real = ops.cross_net_limits()
    assert sorted(real) == ["max_cols", "max_layers", "max_wg", "tile_rows"] and all(v >= 1 for v in real.values())
    width = model.feature_map.sum_emb_out_dim()
    assert width <= real["max_cols"] and g.meta["n_cross"] <= real["max_layers"]
    assert real["max_cols"] >= 1248                                  # both production widths are inside
    batch = tb(g.batches[-1])
    model.eval()
    _reset_calls()
    with torch.no_grad():
        inside = model.forward(batch)["y_pred"]._fx_logit.clone()
    assert CALLS["cross_net_fwd"] == 1
    small = dict(real)
    small[what] = (width if what == "max_cols" else g.meta["n_cross"]) - 1
    monkeypatch.setattr(ops, "cross_net_limits", lambda: small)
    assert model._fused and not model.crossnet.native(torch.empty(2, width))
    _reset_calls()
    with torch.no_grad():
        outside = model.forward(batch)["y_pred"]._fx_logit
    assert torch.allclose(inside, outside, atol=1e-5)
    assert np.abs(outside.reshape(-1).numpy() - g.expect["logit0"]).max() <= LOGIT_TOL
    model.train()
    losses = [float(model.train_step(tb(g.batches[i])).item()) for i in range(g.meta["steps"])]
    np.testing.assert_allclose(losses, g.expect["loss"], rtol=0, atol=1e-4)
    assert CALLS == {"cross_net_fwd": 0, "cross_net_bwd": 0}


def _layer(layers, D, n, seed):
    torch.manual_seed(seed)
    layer = layers.CrossNet(D, n)
    with torch.no_grad():
        for ci in layer.cross_net:
            ci.weight.weight.copy_(torch.randn(1, D) / D ** 0.5)
            ci.bias.copy_(torch.randn(D))
    return layer


@pytest.mark.parametrize("n", [1, 2, 3])
def test_cross_net_layer_alone_matches_the_fp64_restatement_with_the_stated_launches(n, monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    B, D = 9, 6
    layer = _layer(layers, D, n, seed=10 + n)
    assert sorted(layer.state_dict()) == sorted(["cross_net.%d.weight.weight" % i for i in range(n)] +
                                                ["cross_net.%d.bias" % i for i in range(n)])
    fresh = layers.CrossNet(D, n)
    assert all(bool((ci.bias == 0).all()) for ci in fresh.cross_net)          # zeros, as the reference starts them
    assert all(float(ci.weight.weight.detach().abs().max()) > 0 for ci in fresh.cross_net)
    x, gy = torch.randn(B, D), torch.randn(B, D)
    params = [p for ci in layer.cross_net for p in (ci.weight.weight, ci.bias)]
    x64 = x.double().requires_grad_(True)
    w64 = layer._w.detach().double().requires_grad_(True)
    b64 = layer._b.detach().double().requires_grad_(True)
    want = cross_net_reference(x64, w64, b64)
    want_dx, want_dw, want_db = torch.autograd.grad(want, [x64, w64, b64], gy.double())
    for fused in (True, False):
        layer.fused = fused
        xin = x.clone().requires_grad_(True)
        _reset_calls()
        got = layer(xin)
        fwd = dict(CALLS)
        got_g = torch.autograd.grad(got, [xin] + params, gy)
        assert torch.allclose(got.detach().double(), want.detach(), atol=1e-5)
        assert torch.allclose(got_g[0].double(), want_dx, atol=1e-4)
        for i in range(n):
            assert got_g[1 + 2 * i].shape == (1, D) and got_g[2 + 2 * i].shape == (D,)
            assert torch.allclose(got_g[1 + 2 * i].double()[0], want_dw[i], atol=1e-4), (fused, i)
            assert torch.allclose(got_g[2 + 2 * i].double(), want_db[i], atol=1e-4), (fused, i)
        if fused:       # ONE launch forward, one call (two launches) backward, whatever n is
            assert fwd == {"cross_net_fwd": 1, "cross_net_bwd": 0} and CALLS == {"cross_net_fwd": 1, "cross_net_bwd": 1}
        else:
            assert CALLS == {"cross_net_fwd": 0, "cross_net_bwd": 0}


def test_eval_forward_takes_no_stash(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers, ops
    seen = []
    emul = ops.cross_net_fwd
    monkeypatch.setattr(ops, "cross_net_fwd", lambda x0, w, b, out, s=None: (seen.append(s), emul(x0, w, b, out, s))[1])
    layer = _layer(layers, 6, 2, seed=5)
    x = torch.randn(4, 6)
    with torch.no_grad():
        a = layer(x)
    b = layer(x.clone().requires_grad_(True))
    assert seen[0] is None and tuple(seen[1].shape) == (4, 2) and torch.equal(a, b.detach())


def test_out_into_receives_the_result_and_nothing_else(monkeypatch):
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


def test_parameters_alias_the_packed_storage_after_to_load_state_dict_and_an_optimizer_step(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    D, n = 6, 3
    layer = _layer(layers, D, n, seed=30)
    assert _aliases_packed(layer)
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    layer.to(torch.float64)
    assert layer._w.dtype == torch.float64 and layer._b.dtype == torch.float64 and _aliases_packed(layer)
    layer.to(torch.float32)
    assert _aliases_packed(layer)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, before[k]), k
    sd = {k: torch.randn_like(v) for k, v in before.items()}
    layer.load_state_dict(sd)
    assert _aliases_packed(layer)
    for i in range(n):
        assert torch.equal(layer._w[i], sd["cross_net.%d.weight.weight" % i][0])
        assert torch.equal(layer._b[i], sd["cross_net.%d.bias" % i])
    # an optimizer step on the Parameters is a step of the storage the kernels read
    opt = torch.optim.SGD(layer.parameters(), lr=0.5)
    w0, b0 = layer._w.clone(), layer._b.clone()
    layer(torch.randn(4, D)).square().sum().backward()
    opt.step()
    assert _aliases_packed(layer)
    assert not torch.equal(layer._w, w0) and not torch.equal(layer._b, b0)
    for i, ci in enumerate(layer.cross_net):
        assert torch.allclose(layer._w[i], w0[i] - 0.5 * ci.weight.weight.grad[0])
        assert torch.allclose(layer._b[i], b0[i] - 0.5 * ci.bias.grad)


def test_dcn_writes_both_towers_into_one_buffer_and_falls_back_to_cat(tmp_path, monkeypatch):
    """The plain Linear / ReLU tower takes `out_into`: fc reads [cross | deep] from one buffer and no torch.cat joins
    them; with batch_norm the tower's result is its own tensor and the cat joins them: the same logits."""
    g = Golden("dcn_adam")
    model = _build(g, tmp_path, monkeypatch, fused=True)
    cats = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **kw: (cats.append(1), real_cat(*a, **kw))[1])
    seen = []
    model.fc.register_forward_pre_hook(lambda m, inp: seen.append(inp[0]))
    model.eval()
    with torch.no_grad():
        logit = model.forward(tb(g.batches[0]))["y_pred"]._fx_logit.clone()
    n_side = len(cats)
    D0, H = model.feature_map.sum_emb_out_dim(), g.meta["dnn"][-1]
    assert tuple(seen[-1].shape) == (g.meta["B"], D0 + H) and seen[-1].is_contiguous()
    # the tower with batch_norm (identity statistics and affine at its start: running mean 0, variance 1) does not
    # take out_into
    zoo = _install_all(monkeypatch)
    from fuxictr_amd.features import FeatureMap
    m = g.meta
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": m["embedding_dim"]})
    bn = zoo.DCN(fmap, gpu=-1, embedding_dim=m["embedding_dim"], optimizer="adam", loss="binary_crossentropy",
                 task="binary_classification", metrics=["AUC"], verbose=0, model_root=str(tmp_path),
                 dnn_hidden_units=m["dnn"], dnn_activations="relu", num_cross_layers=m["n_cross"], batch_norm=True,
                 fused=True)
    plain = zoo.DCN(fmap, gpu=-1, embedding_dim=m["embedding_dim"], optimizer="adam", loss="binary_crossentropy",
                    task="binary_classification", metrics=["AUC"], verbose=0, model_root=str(tmp_path),
                    dnn_hidden_units=m["dnn"], dnn_activations="relu", num_cross_layers=m["n_cross"], batch_norm=True,
                    fused=False)
    plain.load_state_dict(bn.state_dict())
    bn.eval(), plain.eval()
    _reset_calls()
    before = len(cats)
    with torch.no_grad():
        a = bn.forward(tb(g.batches[0]))["y_pred"]._fx_logit
    bn_cats = len(cats) - before
    assert CALLS["cross_net_fwd"] == 1                                # the fused cross stack, joined by the cat
    before = len(cats)
    with torch.no_grad():
        b = plain.forward(tb(g.batches[0]))["y_pred"]._fx_logit
    assert bn_cats == len(cats) - before == n_side + 1               # exactly one more: the join of the two towers
    assert torch.allclose(a, b, atol=1e-5)
    # ... and on the fixture's own model the two routes give the same logits
    model._fused = False
    model.crossnet.fused = False
    before = len(cats)
    with torch.no_grad():
        logit2 = model.forward(tb(g.batches[0]))["y_pred"]._fx_logit
    assert len(cats) - before == n_side + 1
    assert torch.allclose(logit, logit2, atol=1e-5) and torch.allclose(seen[-1], seen[0], atol=1e-5)


def test_fixtures_exercise_the_cross_weights():
    """What make_golden_dcn.py asserted when it wrote the fixtures, re-checked from the committed files."""
    import os
    from conftest import GOLDEN
    largest = os.path.getsize(os.path.join(GOLDEN, "masknet_parallel_adam.npz"))
    for case in DCN_CASES:
        g = Golden(case)
        m = g.meta
        loss = list(g.expect["loss"])
        assert all(a != b for a, b in zip(loss, loss[1:])), (case, loss)
        assert m["w_share"] >= 0.05 and m["model"] == "DCN", case
        for i in range(m["n_cross"]):
            for k in ("crossnet.cross_net.%d.bias" % i, "crossnet.cross_net.%d.weight.weight" % i):
                assert not np.array_equal(g.state0[k], g.state1[k]), (case, k)
        assert m["B"] == 64 and m["steps"] == 3
        assert os.path.getsize(os.path.join(GOLDEN, case + ".npz")) <= largest, case
    m = Golden("dcn_adam").meta
    assert (m["embedding_dim"], m["n_dense"], len(m["cards"]), m["n_cross"], m["dnn"]) == (8, 3, 7, 3, [32, 16])
    m = Golden("dcn_d10_sgd").meta
    width = m["embedding_dim"] * (m["n_dense"] + len(m["cards"]))
    assert width == 90 and width % 4 != 0 and m["net_reg"] == 1e-4 and m["optimizer"] == "SGD"       # the scalar arm
    assert Golden("dcn_cross_only").meta["dnn"] == [] and Golden("dcn_one_layer").meta["n_cross"] == 1
    m = Golden("dcn_zoo_test").meta
    assert (m["embedding_dim"], m["dnn"], m["n_cross"], m["emb_reg"], m["lr"]) == (4, [64, 32], 3, 1e-8, 1e-3)


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib, ops
    for name in ("fx_cross_net_fwd", "fx_cross_net_bwd", "fx_cross_net_limits", "fx_cross_net_workspace_floats"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    lim = ops.cross_net_limits()
    one = 16        # (any non-null address: validation happens before anything is read)
    st = lib.fx_cross_net_fwd(one, 8, one, one, one, 8, None, 4, 0, 2, None)
    assert st == 1 and b"cols=0" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(one, 1 << 20, one, one, one, 1 << 20, None, 4, lim["max_cols"] + 1, 2, None)
    assert st == 1 and b"cols=" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(one, 8, one, one, one, 8, None, 4, 8, lim["max_layers"] + 1, None)
    assert st == 1 and b"L=" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(one, 8, one, one, one, 8, None, 4, 8, 0, None)
    assert st == 1 and b"L=0" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(None, 8, one, one, one, 8, None, 4, 8, 2, None)
    assert st == 1 and b"null x0" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(one, 7, one, one, one, 8, None, 4, 8, 2, None)
    assert st == 1 and b"x0 row stride" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(one, 8, one, one, one, 7, None, 4, 8, 2, None)
    assert st == 1 and b"out row stride" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(one, 8, one, None, one, 8, None, 4, 8, 2, None)
    assert st == 1 and b"null w / b" in lib.fx_last_error()
    st = lib.fx_cross_net_fwd(one, 8, one, one, one, 8, None, -1, 8, 2, None)
    assert st == 1 and b"rows=-1" in lib.fx_last_error()
    assert lib.fx_cross_net_fwd(one, 8, one, one, one, 8, None, 0, 8, 2, None) == 0             # no rows: no launch
    st = lib.fx_cross_net_bwd(one, 7, one, 8, one, one, one, one, 8, one, one, one, 4, 8, 2, 1, None)
    assert st == 1 and b"dout row stride" in lib.fx_last_error()
    st = lib.fx_cross_net_bwd(one, 8, one, 8, one, one, one, None, 8, one, one, one, 4, 8, 2, 1, None)
    assert st == 1 and b"null dx0" in lib.fx_last_error()
    st = lib.fx_cross_net_bwd(one, 8, one, 8, one, one, None, one, 8, one, one, one, 4, 8, 2, 1, None)
    assert st == 1 and b"null w / b / s" in lib.fx_last_error()
    st = lib.fx_cross_net_bwd(one, 8, one, 8, one, one, one, one, 8, one, one, None, 4, 8, 2, 1, None)
    assert st == 1 and b"workspace" in lib.fx_last_error()
    st = lib.fx_cross_net_bwd(one, 8, one, 8, one, one, one, one, 8, one, one, one, 4, 8, lim["max_layers"] + 1, 1, None)
    assert st == 1 and b"L=" in lib.fx_last_error()
    # the workspace: one row of (L + 1) column sums and L scalars per workgroup, at most max_wg of them
    tile, cap = lim["tile_rows"], lim["max_wg"]
    per = ops.cross_net_workspace_floats(1, 8, 3)
    assert per >= 4 * 8 + 3 and per % 4 == 0
    assert ops.cross_net_workspace_floats(tile + 1, 8, 3) == 2 * per
    assert ops.cross_net_workspace_floats(10 ** 9, 8, 3) == cap * per
    from fuxictr_amd._lib import FxError
    x = torch.zeros(4, 8)
    with pytest.raises(FxError, match="GPU"):
        ops.cross_net_fwd(x, torch.zeros(2, 8), torch.zeros(2, 8), torch.empty(4, 8))
    with pytest.raises(FxError, match="GPU"):
        ops.cross_net_bwd(x, x, torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(4, 2), torch.empty(4, 8),
                          torch.empty(2, 8), torch.empty(2, 8), True, torch.empty(per))
