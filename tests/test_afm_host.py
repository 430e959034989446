"""AFM on the native layers, host side (no GPU): zoo.AFM + layers._AFMAttnFn wired end to end with the kernels
replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the two fx_afm_attn_* wrappers emulated
here from their formulas in fp32 torch (checked against torch autograd of the module-by-module composition below) —
against fixtures recorded from the REAL reference's model_zoo.AFM (tests/golden/make_golden_afm.py).  Checks the
parameter names, the fused node (one afm_attn_fwd per forward, one afm_attn_bwd per backward), the module-by-module
composition, the routes around the kernel (no attention, dropout in training, outside the envelope) and the
optimizer protocol; the HIP kernels themselves are held to an fp64 restatement in tests/test_gpu_afm_attn.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, pred atol 2e-5, losses 1e-4 per step, trained
weights through conftest.assert_weights_close."""
import os

import contextlib

import numpy as np
import pytest
import torch

import _cpu_emul
from conftest import GOLDEN, Golden, assert_weights_close
from zoo_cases import LOGIT_TOL, allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

AFM_CASES = ["afm_adam", "afm_d10_sgd", "afm_noatt", "afm_two_fields", "afm_zoo_test"]
ATT_KEYS = ["attention.0.weight", "attention.0.bias", "attention.2.weight", "weight_p.weight"]


# ---- the formulas, in the dtype of the arguments ----------------------------------------------------------
def afm_pairs(x):
    """x [B, F, D] -> e [B, P, D], the pairs i < j in torch.triu_indices order"""
    F = x.shape[1]
    i, j = torch.triu_indices(F, F, offset=1)
    return x[:, i, :] * x[:, j, :]


def afm_reference(x, W1, b1, w2, wp, addend=None, parts=False):
    """AFM.py:84-93 composed tensor by tensor: -> out [B, 1] (parts: also z, s, t, a)"""
    e = afm_pairs(x)
    z = e @ W1.t() + b1
    s = torch.relu(z) @ w2.reshape(-1)
    a = torch.softmax(s, dim=1)
    out = ((a.unsqueeze(-1) * e).sum(dim=1) @ wp.reshape(-1)).unsqueeze(-1)
    if addend is not None:
        out = out + addend.reshape(-1, 1)
    if parts:
        return out, z, s, e @ wp.reshape(-1), a
    return out


def afm_stats_reference(x, W1, b1, w2, wp):
    """-> [B, 3]: the softmax's max, its denominator, y without the addend"""
    out, z, s, t, a = afm_reference(x, W1, b1, w2, wp, parts=True)
    m = s.max(dim=1).values
    return torch.stack([m, torch.exp(s - m.unsqueeze(1)).sum(dim=1), out.reshape(-1)], dim=1)


def afm_bwd_reference(g, x, W1, b1, w2, wp, stats):
    """The backward as the kernel states it (include/fxctr.h) -> dx [B, F, D], dW1, db1, dw2, dwp"""
    B, F, D = x.shape
    i, j = torch.triu_indices(F, F, offset=1)
    e = x[:, i, :] * x[:, j, :]
    z = e @ W1.t() + b1
    h = torch.relu(z)
    s, t = h @ w2.reshape(-1), e @ wp.reshape(-1)
    a = torch.exp(s - stats[:, 0:1]) / stats[:, 1:2]
    dt = g.reshape(-1, 1) * a
    ds = dt * (t - stats[:, 2:3])
    dz = ds.unsqueeze(-1) * w2.reshape(-1) * (z > 0).to(x.dtype)
    de = dt.unsqueeze(-1) * wp.reshape(-1) + dz @ W1
    dx = torch.zeros_like(x)
    dx.index_add_(1, i, de * x[:, j, :])
    dx.index_add_(1, j, de * x[:, i, :])
    dW1 = torch.einsum("bpa,bpd->ad", dz, e)
    return dx, dW1, dz.sum(dim=(0, 1)), (ds.unsqueeze(-1) * h).sum(dim=(0, 1)), (dt.unsqueeze(-1) * e).sum(dim=(0, 1))


# ---- emulations of the two ops ------------------------------------------------------------------------------
CALLS = {"afm_attn_fwd": 0, "afm_attn_bwd": 0}


def _emul_afm_attn_fwd(rec, F, D, W1, b1, w2, wp, addend, out, stats):
    CALLS["afm_attn_fwd"] += 1
    with torch.no_grad():
        x = rec.reshape(rec.shape[0], F, D)
        st = afm_stats_reference(x, W1, b1, w2, wp)
        stats.copy_(st)
        y = st[:, 2:3]
        out.copy_(y if addend is None else y + addend.reshape(-1, 1))
    return out, stats


def _emul_afm_attn_bwd(g, rec, F, D, W1, b1, w2, wp, stats, drec, grads, workspace):
    CALLS["afm_attn_bwd"] += 1
    with torch.no_grad():
        B = rec.shape[0]
        dx, dW1, db1, dw2, dwp = afm_bwd_reference(g, rec.reshape(B, F, D), W1, b1, w2, wp, stats)
        drec.copy_(dx.reshape(B, F * D))
        grads.copy_(torch.cat([dW1.reshape(-1), db1, dw2, dwp]))
    return drec, grads


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "afm_attn_fwd", _emul_afm_attn_fwd)
    monkeypatch.setattr(ops, "afm_attn_bwd", _emul_afm_attn_bwd)
    monkeypatch.setattr(ops, "afm_attn_workspace_floats", lambda B, F, D, A: 4)
    for k in CALLS:
        CALLS[k] = 0


def build_afm(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.AFM with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_afm.py)."""
    m = g.meta
    return build_from_golden(zoo.AFM, g, tmp_path, gpu=gpu, attention_dim=m["attention_dim"],
                             use_attention=m["use_attention"], **extra)


def _install_all(monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return zoo


def _build(g, tmp_path, monkeypatch, **extra):
    return build_afm(_install_all(monkeypatch), g, tmp_path, **extra)


@contextlib.contextmanager
def _launches(fwd, bwd):
    """the launch counters over the block move by exactly (fwd, bwd)"""
    before = dict(CALLS)
    yield
    assert [CALLS[k] - before[k] for k in ("afm_attn_fwd", "afm_attn_bwd")] == [fwd, bwd]


def _expected_calls(g, fused):
    return 1 if (fused and g.meta["use_attention"]) else 0


def test_emulated_ops_match_torch_autograd_of_the_module_composition():
    gen = torch.Generator().manual_seed(5)
    for B, F, D, A in ((3, 2, 4, 3), (5, 4, 5, 3), (4, 7, 6, 9)):
        x = torch.randn(B, F, D, generator=gen).requires_grad_(True)
        W1 = (torch.randn(A, D, generator=gen) / D ** 0.5).requires_grad_(True)
        b1 = (0.3 * torch.randn(A, generator=gen)).requires_grad_(True)
        w2 = torch.randn(1, A, generator=gen).requires_grad_(True)
        wp = torch.randn(1, D, generator=gen).requires_grad_(True)
        add = torch.randn(B, 1, generator=gen).requires_grad_(True)
        g = torch.randn(B, 1, generator=gen)
        # module by module, as AFM.forward composes them
        att = torch.nn.Sequential(torch.nn.Linear(D, A), torch.nn.ReLU(), torch.nn.Linear(A, 1, bias=False),
                                  torch.nn.Softmax(dim=1))
        proj = torch.nn.Linear(D, 1, bias=False)
        with torch.no_grad():
            att[0].weight.copy_(W1), att[0].bias.copy_(b1), att[2].weight.copy_(w2), proj.weight.copy_(wp)
        e = afm_pairs(x)
        want = proj(torch.sum(att(e) * e, dim=1)) + add
        wants = torch.autograd.grad(want, [x, att[0].weight, att[0].bias, att[2].weight, proj.weight, add], g)
        out, stats = torch.empty(B, 1), torch.empty(B, 3)
        d = [t.detach() for t in (x, W1, b1, w2, wp, add)]
        _emul_afm_attn_fwd(d[0].reshape(B, F * D), F, D, d[1], d[2], d[3].reshape(-1), d[4].reshape(-1), d[5], out,
                           stats)
        assert torch.allclose(out, want.detach(), atol=1e-5)
        drec, grads = torch.empty(B, F * D), torch.empty(A * D + 2 * A + D)
        _emul_afm_attn_bwd(g, d[0].reshape(B, F * D), F, D, d[1], d[2], d[3].reshape(-1), d[4].reshape(-1), stats,
                           drec, grads, None)
        AD = A * D
        got = [drec.reshape(B, F, D), grads[:AD].reshape(A, D), grads[AD:AD + A], grads[AD + A:AD + 2 * A].reshape(1, A),
               grads[AD + 2 * A:].reshape(1, D), g]
        for a, b in zip(got, wants):
            assert a.shape == b.shape and torch.allclose(a, b, atol=2e-5), (a - b).abs().max()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", AFM_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    m = g.meta
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts keys, shapes, dtypes)
    D, A, F = m["embedding_dim"], m["attention_dim"], m["n_dense"] + len(m["cards"])
    assert g.state0["attention.0.weight"].shape == (A, D) and g.state0["attention.0.bias"].shape == (A,)
    assert g.state0["attention.2.weight"].shape == (1, A) and g.state0["weight_p.weight"].shape == (1, D)
    assert g.state0["product_layer.triu_index"].shape == (2, F * (F - 1) // 2)
    assert g.state0["lr_layer.bias"].shape == (1,)
    assert not model.product_layer.triu_index.requires_grad
    with _launches(_expected_calls(g, fused), 0):
        check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", AFM_CASES)
def test_training_trajectory_and_trained_weights(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)
    n = _expected_calls(g, fused)                                    # one launch forward, one backward, per step
    check_trajectory(model, g, per_step=lambda i: _launches(n, n))


def test_fused_switch_follows_the_environment_and_the_defaults_are_the_references(tmp_path, monkeypatch):
    import inspect
    g = Golden("afm_adam")
    monkeypatch.setenv("FX_AFM_FUSED", "0")
    assert not _build(g, tmp_path, monkeypatch)._fused
    assert _build(g, tmp_path, monkeypatch, fused=True)._fused
    monkeypatch.delenv("FX_AFM_FUSED")
    model = _build(g, tmp_path, monkeypatch)
    assert model._fused and model._native
    sig = inspect.signature(type(model).__init__).parameters
    assert sig["embedding_dim"].default == 10 and sig["attention_dim"].default == 10
    assert sig["attention_dropout"].default == [0, 0] and sig["use_attention"].default is True
    assert sig["model_id"].default == "AFM" and sig["learning_rate"].default == 1e-3
    for name in ("embedding_layer", "product_layer", "lr_layer", "attention", "weight_p", "dropout1", "dropout2"):
        assert hasattr(model, name)
    assert isinstance(model.attention, torch.nn.Sequential) and len(model.attention) == 4
    assert isinstance(model.attention[3], torch.nn.Softmax) and model.attention[3].dim == 1


def test_attention_dropout_takes_the_modules_in_training_and_the_fused_op_in_eval(tmp_path, monkeypatch):
    g = Golden("afm_adam")
    model = _build(g, tmp_path, monkeypatch, attention_dropout=[0.3, 0.2])
    assert model.dropout1.p == 0.3 and model.dropout2.p == 0.2
    model.eval()
    with torch.no_grad():
        p = model.forward(tb(g.batches[-1]))["y_pred"]
    assert CALLS == {"afm_attn_fwd": 1, "afm_attn_bwd": 0}
    assert np.abs(p._fx_logit.reshape(-1).numpy() - g.expect["logit0"]).max() <= LOGIT_TOL
    model.train()
    torch.manual_seed(0)
    loss = model.train_step(tb(g.batches[0]))
    assert bool(torch.isfinite(loss)) and CALLS == {"afm_attn_fwd": 1, "afm_attn_bwd": 0}


def test_outside_the_envelope_the_model_composes_the_modules(tmp_path, monkeypatch):
    """A single field (no pair) and an attention wider than the kernel takes: neither op is called and the result is
    the composition's."""
    zoo = _install_all(monkeypatch)
    from fuxictr_amd import ops
    from fuxictr_amd.features import FeatureMap
    lim = ops.afm_attn_limits()
    assert lim["F_min"] == 2 and lim["A_max"] >= 64 and lim["FD_max"] >= 39 * 40 and lim["P_max"] >= 741
    assert ops.afm_attn_in_envelope(39, 16, 16) and ops.afm_attn_in_envelope(39, 40, 40)
    assert not ops.afm_attn_in_envelope(1, 8, 8) and not ops.afm_attn_in_envelope(4, 8, lim["A_max"] + 1)
    kw = dict(gpu=-1, optimizer="adam", loss="binary_crossentropy", task="binary_classification", metrics=["AUC"],
              verbose=0, model_root=str(tmp_path))
    for n_dense, cards, A in ((0, [37], 8), (1, [37, 5], lim["A_max"] + 1)):
        spec = {"dataset_id": "afm_env", "num_fields": n_dense + len(cards), "total_features": 0,
                "input_length": n_dense + len(cards), "labels": ["label"],
                "features": [{"I%d" % (k + 1): {"source": "", "type": "numeric"}} for k in range(n_dense)] +
                            [{"C%d" % (k + 1): {"source": "", "type": "categorical", "padding_idx": 0,
                                                "vocab_size": c + 1}} for k, c in enumerate(cards)]}
        fmap = FeatureMap("afm_env", str(tmp_path))
        fmap.load_dict(spec, {"embedding_dim": 8})
        model = zoo.AFM(fmap, embedding_dim=8, attention_dim=A, **kw)
        assert model._fused and not model._native
        batch = {"label": torch.zeros(6)}
        for k in range(n_dense):
            batch["I%d" % (k + 1)] = torch.rand(6)
        for k, c in enumerate(cards):
            batch["C%d" % (k + 1)] = torch.randint(1, c + 1, (6,))
        model.train()
        loss = model.train_step(batch)
        assert bool(torch.isfinite(loss)) and CALLS == {"afm_attn_fwd": 0, "afm_attn_bwd": 0}


def test_fixtures_exercise_the_attention():
    """What make_golden_afm.py asserted when it wrote the fixtures, re-checked from the committed files."""
    largest = os.path.getsize(os.path.join(GOLDEN, "gdcn_adam.npz"))
    for case in AFM_CASES:
        g = Golden(case)
        m = g.meta
        loss = list(g.expect["loss"])
        assert all(a != b for a, b in zip(loss, loss[1:])), (case, loss)
        assert m["B"] == 64 and m["steps"] == 3 and m["emb_scale_used"] <= m["emb_scale_max"]
        assert os.path.getsize(os.path.join(GOLDEN, case + ".npz")) <= largest, case
        moved = [k for k in ATT_KEYS if not np.array_equal(g.state0[k], g.state1[k])]
        if m["use_attention"] and m["n_pairs"] > 1:
            assert m["att_ratio_share"] >= 0.5 and m["att_share"] >= 0.05 and m["wp_share"] >= 0.05, case
            assert moved == ATT_KEYS, (case, moved)
    m = Golden("afm_d10_sgd").meta
    assert (m["embedding_dim"], m["attention_dim"]) == (10, 10) and m["net_reg"] == 1e-4 and m["optimizer"] == "SGD"
    assert (m["embedding_dim"] * (m["n_dense"] + len(m["cards"]))) % 4 != 0                    # the scalar arm
    m = Golden("afm_two_fields").meta
    assert m["n_pairs"] == 1 and m["wp_share"] >= 0.05 and m["moved"] == ["weight_p.weight"]
    m = Golden("afm_noatt").meta
    assert not m["use_attention"] and m["pair_share"] >= 0.05
    m = Golden("afm_zoo_test").meta
    assert (m["embedding_dim"], m["attention_dim"], m["emb_reg"], m["lr"]) == (4, 8, 1e-8, 1e-3)


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib, ops
    for name in ("fx_afm_attn_fwd", "fx_afm_attn_bwd", "fx_afm_attn_tile_rows", "fx_afm_attn_limits",
                 "fx_afm_attn_workspace_floats"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert ops.afm_attn_tile_rows() >= 1 and ops.afm_attn_tile_rows(5, 6, 3) == ops.afm_attn_tile_rows()
    n = ops.afm_attn_grad_floats(6, 3)
    assert n == 3 * 6 + 2 * 3 + 6 and ops.afm_attn_workspace_floats(9, 5, 6, 3) >= 3 * n
    one = 16        # (any non-null address: validation happens before anything is read)
    st = lib.fx_afm_attn_fwd(one, 8, 4, 1, 8, one, one, one, one, 4, None, one, one, None)
    assert st == 1 and b"F=1" in lib.fx_last_error()
    st = lib.fx_afm_attn_fwd(one, 8, 4, 3, 8, one, one, one, one, 65, None, one, one, None)
    assert st == 1 and b"A=65" in lib.fx_last_error()
    st = lib.fx_afm_attn_fwd(one, 23, 4, 3, 8, one, one, one, one, 4, None, one, one, None)
    assert st == 1 and b"X row stride" in lib.fx_last_error()
    st = lib.fx_afm_attn_fwd(one, 24, 4, 3, 8, None, one, one, one, 4, None, one, one, None)
    assert st == 1 and b"null W1" in lib.fx_last_error()
    st = lib.fx_afm_attn_fwd(one, 24, -1, 3, 8, one, one, one, one, 4, None, one, one, None)
    assert st == 1 and b"B=-1" in lib.fx_last_error()
    st = lib.fx_afm_attn_fwd(one, 5000, 4, 100, 50, one, one, one, one, 4, None, one, one, None)
    assert st == 1 and b"F*D=5000" in lib.fx_last_error()
    assert lib.fx_afm_attn_fwd(one, 24, 0, 3, 8, one, one, one, one, 4, None, one, one, None) == 0   # no rows
    st = lib.fx_afm_attn_bwd(one, one, 24, 4, 3, 8, one, one, one, one, 4, one, one, 23, one, one, None)
    assert st == 1 and b"dX row stride" in lib.fx_last_error()
    st = lib.fx_afm_attn_bwd(one, one, 24, 4, 3, 8, one, one, one, one, 4, one, one, 24, None, one, None)
    assert st == 1 and b"null grads" in lib.fx_last_error()
