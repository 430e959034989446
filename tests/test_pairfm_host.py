"""FwFM and FmFM on the native layers, host side (no GPU): zoo.FwFM / zoo.FmFM + layers._PairFMFn wired end to end
with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the two fx_pairfm_*
wrappers emulated here from their formulas in torch (the backward as include/fxctr.h states it, checked against torch
autograd of the reference's composition in fp64) — against fixtures recorded from the REAL reference's model_zoo.FwFM
and model_zoo.FmFM (tests/golden/make_golden_pairfm.py).  Checks the parameter names, the fused node (one pairfm_fwd
per forward, one pairfm_bwd per backward), the module-by-module composition, the route outside the envelope and the
messages for the unsupported options; the HIP kernels themselves are held to the fp64 restatement in
tests/test_gpu_pairfm_kernel.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, pred atol 2e-5, losses 1e-4 per step, trained
weights through conftest.assert_weights_close."""
import os

import contextlib

import numpy as np
import pytest
import torch

import _cpu_emul
from conftest import GOLDEN, Golden, assert_weights_close
from zoo_cases import OMIT, allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

FMFM_CASES = ["fmfm_matrixed_adam", "fmfm_matrixed_d10_sgd", "fmfm_vectorized", "fmfm_two_fields", "fmfm_zoo_test"]
FWFM_CASES = ["fwfm_filv_adam", "fwfm_felv_sgd", "fwfm_lw", "fwfm_zoo_test"]
PAIRFM_CASES = FMFM_CASES + FWFM_CASES


# ---- the formulas, in the dtype of the arguments ----------------------------------------------------------
def pairfm_composition(x, W, mode, wlin=None, bias=None, addend=None):
    """The reference's composition tensor by tensor (FmFM.py:84-91; FwFM.py:78-88 with the inner products written
    as the sum over d of the same two gathers): x [B, F, D] -> out [B, 1]"""
    F = x.shape[1]
    i, j = torch.triu_indices(F, F, offset=1)
    left, right = torch.index_select(x, 1, i), torch.index_select(x, 1, j)
    if mode == "matrix":
        left = torch.matmul(left.unsqueeze(2), W).squeeze(2)
    elif mode == "vector":
        left = left * W
    else:
        left = left * W.reshape(1, -1, 1)
    out = (left * right).sum(dim=-1).sum(dim=-1, keepdim=True)
    if wlin is not None:
        out = out + x.flatten(start_dim=1) @ wlin.reshape(-1, 1)
    if bias is not None:
        out = out + bias.reshape(1, 1)
    if addend is not None:
        out = out + addend.reshape(-1, 1)
    return out


def pairfm_bwd_restated(g, x, W, mode, wlin=None, has_bias=False):
    """The backward as the header states it -> dx [B, F, D], grads = [dW | dwlin | dbias] (flat)"""
    B, F, D = x.shape
    i, j = torch.triu_indices(F, F, offset=1)
    xi, xj = x[:, i, :], x[:, j, :]
    gg = g.reshape(B, 1, 1)
    if mode == "matrix":
        di = torch.einsum("pde,bpe->bpd", W, xj)            # M_ij x_j
        dj = torch.einsum("pde,bpd->bpe", W, xi)            # M_ij^T x_i
        dW = torch.einsum("b,bpd,bpe->pde", g.reshape(-1), xi, xj)
    elif mode == "vector":
        di, dj = W * xj, W * xi
        dW = (gg * xi * xj).sum(dim=0)
    else:
        r = W.reshape(1, -1, 1)
        di, dj = r * xj, r * xi
        dW = (gg * xi * xj).sum(dim=(0, 2))
    dx = torch.zeros_like(x)
    dx.index_add_(1, i, gg * di)
    dx.index_add_(1, j, gg * dj)
    parts = [dW.reshape(-1)]
    if wlin is not None:
        dx = dx + gg * wlin.reshape(1, F, D)
        parts.append((gg * x).sum(dim=0).reshape(-1))
    if has_bias:
        parts.append(g.sum().reshape(1))
    return dx, torch.cat(parts)


def _shaped(W, mode, F, D):
    P = F * (F - 1) // 2
    return W.reshape((P, D, D) if mode == "matrix" else (P, D) if mode == "vector" else (P,))


# ---- emulations of the two ops ------------------------------------------------------------------------------
CALLS = {"pairfm_fwd": 0, "pairfm_bwd": 0}


def _emul_pairfm_fwd(rec, F, D, mode, W, wlin, bias, addend, out):
    CALLS["pairfm_fwd"] += 1
    with torch.no_grad():
        x = rec.reshape(rec.shape[0], F, D)
        out.copy_(pairfm_composition(x, _shaped(W, mode, F, D), mode, wlin, bias, addend))
    return out


def _emul_pairfm_bwd(g, rec, F, D, mode, W, wlin, has_bias, drec, grads, workspace):
    CALLS["pairfm_bwd"] += 1
    with torch.no_grad():
        B = rec.shape[0]
        dx, gr = pairfm_bwd_restated(g, rec.reshape(B, F, D), _shaped(W, mode, F, D), mode, wlin, has_bias)
        drec.copy_(dx.reshape(B, F * D))
        grads.copy_(gr)
    return drec, grads


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "pairfm_fwd", _emul_pairfm_fwd)
    monkeypatch.setattr(ops, "pairfm_bwd", _emul_pairfm_bwd)
    monkeypatch.setattr(ops, "pairfm_workspace_floats", lambda mode, B, F, D: 4)
    for k in CALLS:
        CALLS[k] = 0


def build_pairfm(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.FwFM / zoo.FmFM with a fixture's hyper-parameters and initial weights (shared with
    tests/test_gpu_pairfm.py).  Both take one `regularizer`, which feeds the embedding and the net regularizer."""
    m = g.meta
    own = {"field_interaction_type": m["field_interaction_type"]} if m["model"] == "FmFM" else \
        {"linear_type": m["linear_type"]}
    return build_from_golden(getattr(zoo, m["model"]), g, tmp_path, gpu=gpu, regularizer=m["regularizer"],
                             embedding_regularizer=OMIT, net_regularizer=OMIT, **own, **extra)


def _install_all(monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return zoo


def _build(g, tmp_path, monkeypatch, **extra):
    return build_pairfm(_install_all(monkeypatch), g, tmp_path, **extra)


@contextlib.contextmanager
def _launches(fwd, bwd):
    """the launch counters over the block move by exactly (fwd, bwd)"""
    before = dict(CALLS)
    yield
    assert [CALLS[k] - before[k] for k in ("pairfm_fwd", "pairfm_bwd")] == [fwd, bwd]


@pytest.mark.parametrize("mode", ["scalar", "vector", "matrix"])
def test_backward_restatement_matches_torch_autograd_of_the_composition_in_fp64(mode):
    gen = torch.Generator().manual_seed(7)
    for B, F, D in ((3, 2, 4), (5, 4, 5), (4, 7, 6), (2, 3, 1)):
        P = F * (F - 1) // 2
        x = torch.randn(B, F, D, generator=gen, dtype=torch.float64).requires_grad_(True)
        shape = (P, D, D) if mode == "matrix" else (P, D) if mode == "vector" else (1, P)
        W = torch.randn(*shape, generator=gen, dtype=torch.float64).requires_grad_(True)
        wlin = torch.randn(1, F * D, generator=gen, dtype=torch.float64).requires_grad_(True)
        bias = torch.randn(1, generator=gen, dtype=torch.float64).requires_grad_(True)
        add = torch.randn(B, 1, generator=gen, dtype=torch.float64).requires_grad_(True)
        g = torch.randn(B, 1, generator=gen, dtype=torch.float64)
        for use_lin, use_bias in ((True, True), (False, False), (True, False), (False, True)):
            args = [x, W] + ([wlin] if use_lin else []) + ([bias] if use_bias else []) + [add]
            want = pairfm_composition(x, W if mode != "scalar" else W.reshape(-1), mode, wlin if use_lin else None,
                                      bias if use_bias else None, add)
            wants = torch.autograd.grad(want, args, g)
            d = dict(x=x.detach(), W=W.detach().reshape(-1))
            out = torch.empty(B, 1, dtype=torch.float64)
            _emul_pairfm_fwd(d["x"].reshape(B, F * D), F, D, mode, d["W"], wlin.detach() if use_lin else None,
                             bias.detach() if use_bias else None, add.detach(), out)
            assert torch.allclose(out, want.detach(), atol=1e-12)
            drec = torch.empty(B, F * D, dtype=torch.float64)
            n = W.numel() + (F * D if use_lin else 0) + (1 if use_bias else 0)
            grads = torch.empty(n, dtype=torch.float64)
            _emul_pairfm_bwd(g, d["x"].reshape(B, F * D), F, D, mode, d["W"], wlin.detach() if use_lin else None,
                             use_bias, drec, grads, None)
            got = [drec.reshape(B, F, D), grads[:W.numel()].reshape(W.shape)]
            o = W.numel()
            if use_lin:
                got.append(grads[o:o + F * D].reshape(1, F * D))
                o += F * D
            if use_bias:
                got.append(grads[o:o + 1])
            got.append(g)
            for a, b in zip(got, wants):
                assert a.shape == b.shape and torch.allclose(a, b, atol=1e-11), (mode, (a - b).abs().max())


def test_fwfm_composition_is_the_inner_product_layer_and_its_linear():
    """FwFM.py:78-79 as the reference composes it (masked select of the Gram matrix, then nn.Linear) equals the scalar
    mode of the formula above: the pair order of triu_mask is that of triu_indices."""
    gen = torch.Generator().manual_seed(3)
    B, F, D = 4, 5, 3
    x = torch.randn(B, F, D, generator=gen, dtype=torch.float64)
    lin = torch.nn.Linear(F * (F - 1) // 2, 1).double()
    gram = torch.bmm(x, x.transpose(1, 2))
    mask = torch.ones(F, F).triu(1).bool()
    want = lin(gram.masked_select(mask).view(B, -1))
    got = pairfm_composition(x, lin.weight.detach().reshape(-1), "scalar", bias=lin.bias.detach())
    assert torch.allclose(got, want.detach(), atol=1e-12)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", PAIRFM_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    m = g.meta
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts keys, shapes, dtypes)
    D, F = m["embedding_dim"], m["n_dense"] + len(m["cards"])
    P = F * (F - 1) // 2
    if m["model"] == "FmFM":
        shape = (P, D, D) if m["field_interaction_type"] == "matrixed" else (P, D)
        assert g.state0["interaction_weight"].shape == shape and g.state0["lr_layer.bias"].shape == (1,)
        assert isinstance(model.interaction_weight, torch.nn.Parameter) and model.interaction_weight.requires_grad
        assert "triu_index" not in g.state0                          # a plain attribute in the reference
    else:
        assert g.state0["interaction_weight.weight"].shape == (1, P)
        assert g.state0["interaction_weight.bias"].shape == (1,)
        assert g.state0["inner_product_layer.triu_mask"].shape == (F, F)
        if m["linear_type"] == "FiLV":
            assert g.state0["linear_weight_layer.weight"].shape == (1, F * D)
    with _launches(1 if fused else 0, 0):
        check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", PAIRFM_CASES)
def test_training_trajectory_and_trained_weights(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)
    n = 1 if fused else 0                                            # one launch forward, one backward, per step
    check_trajectory(model, g, per_step=lambda i: _launches(n, n))


def test_fused_switch_follows_the_environment_and_the_defaults_are_the_references(tmp_path, monkeypatch):
    import inspect
    for case, attrs in (("fmfm_matrixed_adam", ("embedding_layer", "interaction_weight", "lr_layer", "triu_index")),
                        ("fwfm_filv_adam", ("embedding_layer", "interaction_weight", "inner_product_layer",
                                            "linear_weight_layer"))):
        g = Golden(case)
        monkeypatch.setenv("FX_PAIRFM_FUSED", "0")
        assert not _build(g, tmp_path, monkeypatch)._fused
        assert _build(g, tmp_path, monkeypatch, fused=True)._fused
        monkeypatch.delenv("FX_PAIRFM_FUSED")
        model = _build(g, tmp_path, monkeypatch)
        assert model._fused and model._native
        sig = inspect.signature(type(model).__init__).parameters
        assert sig["embedding_dim"].default == 10 and sig["regularizer"].default is None
        assert sig["model_id"].default == g.meta["model"] and sig["learning_rate"].default == 1e-3
        assert "embedding_regularizer" not in sig and "net_regularizer" not in sig
        for name in attrs:
            assert hasattr(model, name)
    assert sig["linear_type"].default == "FiLV"
    g = Golden("fmfm_matrixed_d10_sgd")
    model = _build(g, tmp_path, monkeypatch)
    assert model._embedding_regularizer == 1e-4 and model._net_regularizer == 1e-4     # one keyword feeds both
    assert inspect.signature(type(model).__init__).parameters["field_interaction_type"].default == "matrixed"


def test_the_bare_parameter_is_initialised_regularised_and_optimised(tmp_path, monkeypatch):
    g = Golden("fmfm_matrixed_d10_sgd")
    zoo = _install_all(monkeypatch)
    from fuxictr_amd.features import FeatureMap
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": 10})
    kw = dict(gpu=-1, optimizer="SGD", loss="binary_crossentropy", task="binary_classification", metrics=["AUC"],
              verbose=0, model_root=str(tmp_path))
    model = zoo.FmFM(fmap, regularizer=1e-4, **kw)
    w = model.interaction_weight.detach()
    P = w.shape[0]
    assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0             # xavier_normal_ in the constructor
    fan_in, fan_out = torch.nn.init._calculate_fan_in_and_fan_out(w)
    assert abs(float(w.std()) - (2.0 / (fan_in + fan_out)) ** 0.5) < 0.2 * (2.0 / (fan_in + fan_out)) ** 0.5
    assert P == 9 * 8 // 2
    reg = model.regularization_loss().detach()
    with torch.no_grad():
        model.interaction_weight.mul_(2.0)
    assert float(model.regularization_loss().detach()) > float(reg)                       # counted as a net parameter
    with torch.no_grad():
        model.interaction_weight.mul_(0.5)
    before = model.interaction_weight.detach().clone()
    model.train()
    model.train_step(tb(g.batches[0]))
    assert not torch.equal(before, model.interaction_weight.detach())            # it reached the dense optimizer


def test_unsupported_options_raise_the_references_messages(tmp_path, monkeypatch):
    zoo = _install_all(monkeypatch)
    from fuxictr_amd.features import FeatureMap
    g = Golden("fwfm_filv_adam")
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": 8})
    kw = dict(gpu=-1, embedding_dim=8, optimizer="adam", loss="binary_crossentropy", task="binary_classification",
              metrics=["AUC"], verbose=0, model_root=str(tmp_path))
    with pytest.raises(NotImplementedError, match="linear_type=XX is not supported."):
        zoo.FwFM(fmap, linear_type="XX", **kw)
    with pytest.raises(ValueError, match="field_interaction_type=full is not supported."):
        zoo.FmFM(fmap, field_interaction_type="full", **kw)


def test_outside_the_envelope_the_models_compose_the_modules(tmp_path, monkeypatch):
    """An embedding wider than the kernel takes: neither op is called and the step is the composition's."""
    zoo = _install_all(monkeypatch)
    from fuxictr_amd import ops
    from fuxictr_amd.features import FeatureMap
    lim = ops.pairfm_limits()
    assert lim["F_min"] == 2 and lim["D_max"] >= 64 and lim["FD_max"] >= 4096
    assert ops.pairfm_in_envelope(39, 16) and ops.pairfm_in_envelope(9, 10) and ops.pairfm_in_envelope(2, 8)
    assert ops.pairfm_in_envelope(64, 64) and ops.pairfm_in_envelope(7, 1)
    assert not ops.pairfm_in_envelope(1, 8) and not ops.pairfm_in_envelope(3, lim["D_max"] + 1)
    assert not ops.pairfm_in_envelope(lim["FD_max"] // 8 + 1, 8)
    D = lim["D_max"] + 1
    kw = dict(gpu=-1, embedding_dim=D, optimizer="adam", loss="binary_crossentropy", task="binary_classification",
              metrics=["AUC"], verbose=0, model_root=str(tmp_path))
    cards = [37, 5, 11]
    spec = {"dataset_id": "pairfm_env", "num_fields": 3, "total_features": 0, "input_length": 3,
            "labels": ["label"],
            "features": [{"C%d" % (k + 1): {"source": "", "type": "categorical", "padding_idx": 0,
                                            "vocab_size": c + 1}} for k, c in enumerate(cards)]}
    for build in (lambda f: zoo.FmFM(f, **kw), lambda f: zoo.FmFM(f, field_interaction_type="vectorized", **kw),
                  lambda f: zoo.FwFM(f, **kw)):
        fmap = FeatureMap("pairfm_env", str(tmp_path))
        fmap.load_dict(spec, {"embedding_dim": D})
        model = build(fmap)
        assert model._fused and not model._native
        batch = {"label": torch.zeros(6)}
        for k, c in enumerate(cards):
            batch["C%d" % (k + 1)] = torch.randint(1, c + 1, (6,))
        model.train()
        loss = model.train_step(batch)
        assert bool(torch.isfinite(loss)) and CALLS == {"pairfm_fwd": 0, "pairfm_bwd": 0}


def test_fixtures_exercise_the_interaction_weight():
    """What make_golden_pairfm.py asserted when it wrote the fixtures, re-checked from the committed files."""
    for case in PAIRFM_CASES:
        g = Golden(case)
        m = g.meta
        loss = list(g.expect["loss"])
        assert all(a != b for a, b in zip(loss, loss[1:])), (case, loss)
        assert m["B"] == 64 and m["steps"] == 3 and m["emb_scale_used"] <= m["emb_scale_max"]
        assert os.path.getsize(os.path.join(GOLDEN, case + ".npz")) <= 1 << 19, case
        assert m["pair_share"] >= 0.05, case
        keys = ["interaction_weight"] if m["model"] == "FmFM" else \
            ["interaction_weight.weight", "interaction_weight.bias"] + \
            [k for k in g.state0 if k.startswith("linear_weight_layer.")]
        assert len(keys) >= (1 if m["model"] == "FmFM" else 3)
        for k in keys:
            assert not np.array_equal(g.state0[k], g.state1[k]), (case, k)
    m = Golden("fmfm_matrixed_d10_sgd").meta
    assert (m["embedding_dim"], m["regularizer"], m["optimizer"], m["n_dense"]) == (10, 1e-4, "SGD", 2)
    assert Golden("fmfm_two_fields").meta["n_pairs"] == 1
    assert Golden("fmfm_vectorized").meta["field_interaction_type"] == "vectorized"
    assert Golden("fwfm_felv_sgd").meta["linear_type"] == "FeLV" and Golden("fwfm_lw").meta["linear_type"] == "LW"
    m = Golden("fmfm_zoo_test").meta
    assert (m["embedding_dim"], m["regularizer"], m["lr"], m["field_interaction_type"]) == (4, 0, 1e-3, "matrixed")
    m = Golden("fwfm_zoo_test").meta
    assert (m["embedding_dim"], m["regularizer"], m["lr"], m["linear_type"]) == (4, 1e-8, 1e-3, "FiLV")


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib, ops
    for name in ("fx_pairfm_fwd", "fx_pairfm_bwd", "fx_pairfm_tile_rows", "fx_pairfm_limits",
                 "fx_pairfm_workspace_floats"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    T = ops.pairfm_tile_rows("matrix", 39, 16)
    assert T >= 16 and ops.pairfm_tile_rows("matrix", 9, 10) >= 16             # W re-read once per >= 16 samples
    assert ops.pairfm_grad_floats("matrix", 5, 6) == 10 * 36
    assert ops.pairfm_grad_floats("scalar", 5, 6, wlin=True, bias=True) == 10 + 30 + 1
    assert ops.pairfm_grad_floats("vector", 5, 6) == 60
    # more than one slab of samples at 2 T + 3: the partial rows and the reduce's own
    assert ops.pairfm_workspace_floats("matrix", 2 * T + 3, 5, 6) >= 2 * ops.pairfm_grad_floats("matrix", 5, 6)
    # nothing of size B * P: the workspace does not grow with the batch beyond the slab count
    assert ops.pairfm_workspace_floats("matrix", 1 << 20, 39, 16) == ops.pairfm_workspace_floats("matrix", 1 << 14, 39, 16)
    one = 16        # (any non-null address: validation happens before anything is read)
    st = lib.fx_pairfm_fwd(one, 8, 4, 1, 8, 2, one, None, None, None, one, None)
    assert st == 1 and b"F=1" in lib.fx_last_error()
    st = lib.fx_pairfm_fwd(one, 195, 4, 3, 65, 2, one, None, None, None, one, None)
    assert st == 1 and b"D=65" in lib.fx_last_error()
    st = lib.fx_pairfm_fwd(one, 24, 4, 3, 8, 3, one, None, None, None, one, None)
    assert st == 1 and b"mode=3" in lib.fx_last_error()
    st = lib.fx_pairfm_fwd(one, 23, 4, 3, 8, 2, one, None, None, None, one, None)
    assert st == 1 and b"X row stride" in lib.fx_last_error()
    st = lib.fx_pairfm_fwd(one, 24, 4, 3, 8, 2, None, None, None, None, one, None)
    assert st == 1 and b"null W" in lib.fx_last_error()
    st = lib.fx_pairfm_fwd(one, 24, -1, 3, 8, 2, one, None, None, None, one, None)
    assert st == 1 and b"B=-1" in lib.fx_last_error()
    st = lib.fx_pairfm_fwd(one, 5000, 4, 100, 50, 2, one, None, None, None, one, None)
    assert st == 1 and b"F*D=5000" in lib.fx_last_error()
    assert lib.fx_pairfm_fwd(one, 24, 0, 3, 8, 2, one, None, None, None, one, None) == 0          # no rows
    st = lib.fx_pairfm_bwd(one, one, 24, 4, 3, 8, 2, one, None, 0, one, 23, one, one, None)
    assert st == 1 and b"dX row stride" in lib.fx_last_error()
    st = lib.fx_pairfm_bwd(one, one, 24, 4, 3, 8, 2, one, None, 0, one, 24, None, one, None)
    assert st == 1 and b"null grads" in lib.fx_last_error()
