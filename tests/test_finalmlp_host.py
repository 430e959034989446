"""FinalMLP and DualMLP on the native layers, host side (no GPU): zoo.FinalMLP / zoo.DualMLP +
layers.FeatureSelection / InteractionAggregation wired end to end with the kernels replaced by torch-CPU emulations —
tests/_cpu_emul.py for the existing ops, the fx_gate2_* / fx_biagg_* wrappers emulated here from their formulas in
fp32 torch (checked against torch autograd below) — against fixtures recorded from the REAL reference's
model_zoo.FinalMLP / DualMLP (tests/golden/make_golden_finalmlp.py).  Checks the parameter names, the fused
composition (one node for both gates, one for the head, the per-head products through gemm_batch on column slices),
the module-by-module one, the autograd nodes' plumbing and the optimizer protocol; the HIP kernels themselves are
held to an fp64 restatement in tests/test_gpu_finalmlp_kernels.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, losses 1e-4 per step, trained weights
through conftest.assert_weights_close."""
import numpy as np
import pytest
import torch

import _cpu_emul
from conftest import Golden, assert_weights_close
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

FINALMLP_CASES = ["finalmlp_adam", "finalmlp_ctx_sgd", "finalmlp_mixed", "finalmlp_nofs_heads4",
                  "finalmlp_zoo_test", "dualmlp_adam"]


# ---- the formulas, in the dtype of the arguments ----------------------------------------------------------
def gate_reference(E, Z):
    """F = E * 2 sigmoid(Z); Z [B, W] or [1, W]"""
    return E * (2.0 * torch.sigmoid(Z))


def gate_grads_reference(dF, E, Z):
    """-> (dF's share of dE, dZ in the shape of Z)"""
    s = torch.sigmoid(Z)
    dz = dF * E * (2.0 * s * (1.0 - s))
    if Z.shape[0] == 1 and E.shape[0] > 1:
        dz = dz.sum(dim=0, keepdim=True)
    return dF * (2.0 * s), dz


def head_t_reference(X, w_xy, H):
    """T[:, h dyh : (h + 1) dyh] = X[:, h dxh : (h + 1) dxh] W_h"""
    B, dx = X.shape
    Wv = w_xy.reshape(H, dx // H, -1)
    return torch.einsum("bhi,hij->bhj", X.reshape(B, H, dx // H), Wv).reshape(B, -1)


def head_reference(X, Y, w_x, b_x, w_y, b_y, w_xy, H, out_add=None):
    """out[b] = b_x + b_y + X[b] . w_x + Y[b] . (w_y + T[b]) (+ out_add[b]) -> [B, 1]"""
    T = head_t_reference(X, w_xy, H)
    out = b_x + b_y + X @ w_x.reshape(-1, 1) + (Y * (w_y.reshape(1, -1) + T)).sum(dim=1, keepdim=True)
    return out if out_add is None else out + out_add.reshape(-1, 1)


# ---- emulations of the four ops -----------------------------------------------------------------------------
def _emul_gate2_fwd(E, Z1, Z2, F1, F2):
    with torch.no_grad():
        F1.copy_(gate_reference(E, Z1))
        if Z2 is not None:
            F2.copy_(gate_reference(E, Z2))
    return F1, F2


def _emul_gate2_bwd(dF1, dF2, E, Z1, Z2, dE, dZ1, dZ2, workspace, de_accumulate=False):
    with torch.no_grad():
        de, dz = gate_grads_reference(dF1, E, Z1)
        dZ1.copy_(dz)
        if Z2 is not None:
            de2, dz = gate_grads_reference(dF2, E, Z2)
            dZ2.copy_(dz)
            de = de + de2
        dE.add_(de) if de_accumulate else dE.copy_(de)
    return dE, dZ1, dZ2


def _emul_biagg_fwd(X, Y, T, w_x, w_y, b_x, b_y, out_add, out):
    with torch.no_grad():
        t = X @ w_x.reshape(-1, 1) + (Y * (w_y.reshape(1, -1) + T)).sum(dim=1, keepdim=True)
        t = t + (b_x if b_x is not None else 0.0) + (b_y if b_y is not None else 0.0)
        if out_add is not None:
            t = t + out_add.reshape(-1, 1)
        out.copy_(t.reshape(out.shape))
    return out


def _emul_biagg_bwd(g, X, Y, T, w_x, w_y, dT, dY, dXr, dw_x, dw_y, db, workspace):
    with torch.no_grad():
        gc = g.reshape(-1, 1)
        dT.copy_(gc * Y)
        dY.copy_(gc * (w_y.reshape(1, -1) + T))
        if dXr is not None:
            dXr.copy_(gc * w_x.reshape(1, -1))
        dw_x.copy_((X * gc).sum(dim=0).reshape(dw_x.shape))
        dw_y.copy_((Y * gc).sum(dim=0).reshape(dw_y.shape))
        db.fill_(float(gc.sum()))
    return dT, dY, dXr, dw_x, dw_y, db


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "gate2_fwd", _emul_gate2_fwd)
    monkeypatch.setattr(ops, "gate2_bwd", _emul_gate2_bwd)
    monkeypatch.setattr(ops, "biagg_fwd", _emul_biagg_fwd)
    monkeypatch.setattr(ops, "biagg_bwd", _emul_biagg_bwd)
    monkeypatch.setattr(ops, "gate2_workspace_floats", lambda B, W: 1)
    monkeypatch.setattr(ops, "biagg_workspace_floats", lambda B, dx, dy: 1)


def build_finalmlp(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.FinalMLP / zoo.DualMLP with a fixture's hyper-parameters and initial weights (shared with
    tests/test_gpu_finalmlp.py)."""
    m = g.meta
    kw = dict(extra, mlp1_hidden_units=m["mlp1"], mlp2_hidden_units=m["mlp2"])
    if m["model"] == "DualMLP":
        kw.pop("fused", None)
        return build_from_golden(zoo.DualMLP, g, tmp_path, gpu=gpu, **kw)
    return build_from_golden(zoo.FinalMLP, g, tmp_path, gpu=gpu, use_fs=m["use_fs"], fs_hidden_units=m["fs_hidden"],
                             fs1_context=m["fs1_context"], fs2_context=m["fs2_context"], num_heads=m["num_heads"],
                             **kw)


def _build(g, tmp_path, monkeypatch, **extra):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_finalmlp(zoo, g, tmp_path, **extra)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", FINALMLP_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    m = g.meta
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts keys, shapes, dtypes)
    if m["model"] == "FinalMLP":
        for k in ("fusion_module.w_x.weight", "fusion_module.w_x.bias", "fusion_module.w_y.weight",
                  "fusion_module.w_y.bias", "fusion_module.w_xy"):
            assert k in g.state0, k
        assert g.state0["fusion_module.w_xy"].shape == (m["mlp1"][-1] * m["mlp2"][-1] // m["num_heads"], 1)
        for n in (1, 2):
            ctx = m["fs%d_context" % n]
            assert ("fs_module.fs%d_ctx_bias" % n in g.state0) == (m["use_fs"] and not ctx)
            assert any(k.startswith("fs_module.fs%d_ctx_emb." % n) for k in g.state0) == (m["use_fs"] and bool(ctx))
            assert ("fs_module.fs%d_gate.mlp.0.weight" % n in g.state0) == m["use_fs"]
    else:
        assert "mlp1.mlp.0.weight" in g.state0 and "mlp2.mlp.0.weight" in g.state0
        assert not any("fusion_module" in k or "fs_module" in k for k in g.state0)
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", FINALMLP_CASES)
def test_training_trajectory_and_trained_weights(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)
    check_trajectory(model, g)


@pytest.mark.parametrize("case", [c for c in FINALMLP_CASES if c != "dualmlp_adam"])
def test_fused_and_module_by_module_routes_agree(case, tmp_path, monkeypatch):
    g = Golden(case)
    a = _build(g, tmp_path, monkeypatch, fused=True)
    b = _build(g, tmp_path, monkeypatch, fused=False)
    assert a._fused and a.fusion_module.fused and not b._fused and not b.fusion_module.fused
    if g.meta["use_fs"]:
        assert a.fs_module.fused and not b.fs_module.fused
    else:
        assert not hasattr(a, "fs_module")
    a.train(), b.train()
    for i in range(g.meta["steps"]):
        la, lb = float(a.train_step(tb(g.batches[i])).item()), float(b.train_step(tb(g.batches[i])).item())
        assert abs(la - lb) <= 1e-5, (i, la, lb)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert_weights_close(sa[k].numpy(), sb[k].numpy(), g.meta["lr"], g.meta["steps"], k)


def test_fused_switch_follows_the_environment(tmp_path, monkeypatch):
    g = Golden("finalmlp_adam")
    monkeypatch.setenv("FX_FINALMLP_FUSED", "0")
    assert not _build(g, tmp_path, monkeypatch)._fused
    assert _build(g, tmp_path, monkeypatch, fused=True)._fused
    monkeypatch.delenv("FX_FINALMLP_FUSED")
    assert _build(g, tmp_path, monkeypatch)._fused


def test_fixtures_exercise_the_gates_and_the_bilinear_head():
    """What make_golden_finalmlp.py asserted when it wrote the fixtures, re-checked from the committed files."""
    for case in FINALMLP_CASES:
        g = Golden(case)
        m = g.meta
        loss = list(g.expect["loss"])
        assert all(a != b for a, b in zip(loss, loss[1:])), (case, loss)
        if m["model"] != "FinalMLP":
            continue
        assert m["bilinear_share"] >= 0.05, (case, m["bilinear_share"])
        if not m["use_fs"]:
            assert m["gate_spread"] == [] and m["gate_share"] is None
            continue
        assert len(m["gate_spread"]) == 2 and all(s >= 0.2 for s in m["gate_spread"]), (case, m["gate_spread"])
        assert m["gate_share"] >= 0.05, (case, m["gate_share"])
        for n in (1, 2):
            k = "fs_module.fs%d_ctx_bias" % n
            if not m["fs%d_context" % n]:
                # the perturbation is part of state0, and training moves it
                assert np.abs(g.state0[k]).max() > 0 and not np.array_equal(g.state0[k], g.state1[k]), (case, k)
                # the no-context gate recomputed from state0 alone: its spread over the columns
                h = torch.from_numpy(g.state0[k])
                keys = sorted((kk for kk in g.state0 if kk.startswith("fs_module.fs%d_gate.mlp." % n)
                               and kk.endswith(".weight")), key=lambda s: int(s.split(".")[-2]))
                for i, kk in enumerate(keys):
                    h = h @ torch.from_numpy(g.state0[kk]).t() + torch.from_numpy(g.state0[kk[:-6] + "bias"])
                    if i < len(keys) - 1:
                        h = torch.relu(h)
                gate = 2.0 * torch.sigmoid(h)
                assert float(gate.max() - gate.min()) >= 0.2, (case, k)
    assert Golden("finalmlp_ctx_sgd").meta["embedding_dim"] % 4 != 0                # the scalar arm
    assert Golden("finalmlp_ctx_sgd").meta["net_reg"] > 0
    m = Golden("finalmlp_mixed").meta
    assert bool(m["fs1_context"]) != bool(m["fs2_context"])
    m = Golden("finalmlp_nofs_heads4").meta
    assert m["num_heads"] == 4 and m["mlp1"][-1] // 4 != m["mlp2"][-1] // 4


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen)


def test_emulated_ops_match_torch_autograd():
    """The emulations above (= the kernels' formulas) against autograd of the forward formulas."""
    gen = torch.Generator().manual_seed(3)
    B, W = 7, 5
    E = _rand(gen, B, W).requires_grad_(True)
    Z1, Z2 = _rand(gen, B, W).requires_grad_(True), _rand(gen, 1, W).requires_grad_(True)
    g1, g2 = _rand(gen, B, W), _rand(gen, B, W)
    want = torch.autograd.grad([gate_reference(E, Z1), gate_reference(E, Z2)], [E, Z1, Z2], [g1, g2])
    dE, dZ1, dZ2 = torch.full((B, W), 3.0), torch.empty(B, W), torch.empty(1, W)
    _emul_gate2_bwd(g1, g2, E.detach(), Z1.detach(), Z2.detach(), dE, dZ1, dZ2, None, de_accumulate=True)
    for a, b in zip((dE - 3.0, dZ1, dZ2), want):
        assert torch.allclose(a, b, atol=1e-5)
    dx, dy, H = 6, 4, 2
    X, Y = _rand(gen, B, dx).requires_grad_(True), _rand(gen, B, dy).requires_grad_(True)
    w_x, w_y = _rand(gen, 1, dx).requires_grad_(True), _rand(gen, 1, dy).requires_grad_(True)
    b_x, b_y = _rand(gen, 1).requires_grad_(True), _rand(gen, 1).requires_grad_(True)
    w_xy = _rand(gen, dx * dy // H, 1).requires_grad_(True)
    g = _rand(gen, B, 1)
    out = head_reference(X, Y, w_x, b_x, w_y, b_y, w_xy, H)
    want = torch.autograd.grad(out, [Y, w_x, w_y, b_x, b_y], g)
    T = head_t_reference(X, w_xy, H).detach()
    got = torch.empty(B, 1)
    _emul_biagg_fwd(X.detach(), Y.detach(), T, w_x.detach(), w_y.detach(), b_x.detach(), b_y.detach(), None, got)
    assert torch.allclose(got, out, atol=1e-5)
    dT, dY, dXr = torch.empty(B, dy), torch.empty(B, dy), torch.empty(B, dx)
    dwx, dwy, db = torch.empty(1, dx), torch.empty(1, dy), torch.empty(2)
    _emul_biagg_bwd(g, X.detach(), Y.detach(), T, w_x.detach(), w_y.detach(), dT, dY, dXr, dwx, dwy, db, None)
    for a, b in zip((dY, dwx, dwy, db[0:1], db[1:2]), want):
        assert torch.allclose(a, b, atol=1e-5)
    assert torch.allclose(dT, g * Y.detach()) and torch.allclose(dXr, g * w_x.detach())


@pytest.mark.parametrize("contexts", [([], []), (["C2"], []), ([], ["C1", "C3"]), (["C2"], ["C1", "C3"])],
                         ids=["none", "first", "second", "both"])
def test_feature_selection_alone_matches_the_formulas(contexts, tmp_path, monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    from fuxictr_amd.features import FeatureMap
    g = Golden("finalmlp_adam")
    D = 4
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": D})
    W = fmap.num_fields * D
    torch.manual_seed(4)
    fs = layers.FeatureSelection(fmap, W, D, [6], contexts[0], contexts[1])
    with torch.no_grad():
        for k, p in fs.named_parameters():
            if "embedding" not in k:
                p.copy_(0.5 * torch.randn(p.shape))
    batch = tb(g.batches[0])
    B = len(batch["C1"])
    emb = torch.randn(B, W, requires_grad=True)
    params = [p for k, p in fs.named_parameters() if "embedding" not in k]

    def restated():
        outs = []
        for n, ctx in ((1, contexts[0]), (2, contexts[1])):
            gate = getattr(fs, "fs%d_gate" % n)
            if ctx:
                h = getattr(fs, "fs%d_ctx_emb" % n)(batch).flatten(start_dim=1).detach()
            else:
                h = getattr(fs, "fs%d_ctx_bias" % n)
            lins = [m for m in gate.mlp if isinstance(m, torch.nn.Linear)]
            for i, lin in enumerate(lins):
                h = h @ lin.weight.t() + lin.bias
                if i < len(lins) - 1:
                    h = torch.relu(h)
            outs.append(gate_reference(emb, h))
        return outs
    want = restated()
    gy = [torch.randn(B, W), torch.randn(B, W)]
    want_g = torch.autograd.grad(want, [emb] + params, gy)
    for fused in (True, False):
        fs.fused = fused
        got = fs(batch, emb)
        for a, b in zip(got, want):
            assert tuple(a.shape) == (B, W) and torch.allclose(a, b, atol=1e-5)
        got_g = torch.autograd.grad(list(got), [emb] + params, gy)
        for a, b in zip(got_g, want_g):
            assert torch.allclose(a, b, atol=1e-4), (fused, (a - b).abs().max())


@pytest.mark.parametrize("H", [1, 2, 4])
def test_interaction_aggregation_alone_matches_the_formulas(H, monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    torch.manual_seed(6 + H)
    B, dx, dy = 9, 8, 12
    agg = layers.InteractionAggregation(dx, dy, output_dim=1, num_heads=H)
    assert sorted(agg.state_dict()) == ["w_x.bias", "w_x.weight", "w_xy", "w_y.bias", "w_y.weight"]
    assert tuple(agg.w_xy.shape) == (dx * dy // H, 1)
    with torch.no_grad():
        agg.w_x.bias.fill_(0.3), agg.w_y.bias.fill_(-0.2)
    x, y = torch.randn(B, dx, requires_grad=True), torch.randn(B, dy, requires_grad=True)
    add = torch.randn(B, 1, requires_grad=True)
    params = [agg.w_x.weight, agg.w_x.bias, agg.w_y.weight, agg.w_y.bias, agg.w_xy]
    # the per-sample bilinear form written out head by head
    Wv = agg.w_xy.view(H, dx // H, dy // H)
    want = agg.w_x.bias + agg.w_y.bias + x @ agg.w_x.weight.t() + y @ agg.w_y.weight.t()
    for h in range(H):
        xh, yh = x[:, h * (dx // H):(h + 1) * (dx // H)], y[:, h * (dy // H):(h + 1) * (dy // H)]
        want = want + ((xh @ Wv[h]) * yh).sum(dim=1, keepdim=True)
    assert torch.allclose(want, head_reference(x, y, agg.w_x.weight, agg.w_x.bias, agg.w_y.weight, agg.w_y.bias,
                                               agg.w_xy, H), atol=1e-5)
    gy = torch.randn(B, 1)
    for with_add in (False, True):
        ref = want + add if with_add else want
        inputs = [x, y] + params + ([add] if with_add else [])
        want_g = torch.autograd.grad(ref, inputs, gy, retain_graph=True)
        for fused in (True, False):
            agg.fused = fused
            got = agg(x, y, out_add=add if with_add else None)
            assert tuple(got.shape) == (B, 1) and torch.allclose(got, ref, atol=1e-5)
            got_g = torch.autograd.grad(got, inputs, gy)
            for a, b in zip(got_g, want_g):
                assert a.shape == b.shape and torch.allclose(a, b, atol=1e-4), (fused, (a - b).abs().max())


@pytest.mark.parametrize("case", ["finalmlp_adam", "finalmlp_mixed"])
def test_a_gate_without_context_runs_its_tower_on_one_bias_row_not_on_the_batch(case, tmp_path, monkeypatch):
    """The reference repeats the [1, D] bias B times (FinalMLP.py:180); the native tower's first GEMM reads
    layers._GATE_ROWS rows whatever the batch size is: row 0 the bias, the rest zeros."""
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=True)
    from fuxictr_amd import layers, ops
    seen = []
    real = ops.gemm

    def spy(A, B_, C_, **kw):
        seen.append((B_, A.detach().clone()))
        return real(A, B_, C_, **kw)
    monkeypatch.setattr(ops, "gemm", spy)
    model.eval()
    B = g.meta["B"]
    assert layers._GATE_ROWS < B
    with torch.no_grad():
        model.forward(tb(g.batches[0]))
    for n in (1, 2):
        first = getattr(model.fs_module, "fs%d_gate" % n).mlp[0].weight
        rows = [a for w, a in seen if w is first]
        assert len(rows) == 1
        if g.meta["fs%d_context" % n]:
            assert rows[0].shape[0] == B
        else:
            bias = getattr(model.fs_module, "fs%d_ctx_bias" % n)
            assert rows[0].shape[0] == layers._GATE_ROWS
            assert torch.equal(rows[0][:1], bias.detach()) and not rows[0][1:].any()
    # module by module: B rows, as the reference
    seen.clear()
    model.fs_module.fused = False
    with torch.no_grad():
        model.forward(tb(g.batches[0]))
    first = model.fs_module.fs2_gate.mlp[0].weight
    assert [a.shape[0] for w, a in seen if w is first] == [B]


def test_limits_and_unknown_options_raise(tmp_path, monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers, zoo
    with pytest.raises(NotImplementedError, match="output_dim=2"):
        layers.InteractionAggregation(8, 8, output_dim=2)
    with pytest.raises(AssertionError, match="divisible by num_heads"):
        layers.InteractionAggregation(8, 9, num_heads=2)
    agg = layers.InteractionAggregation(8, 12, num_heads=2)
    with pytest.raises(NotImplementedError, match="built for"):
        agg(torch.zeros(3, 8), torch.zeros(3, 8))
    g = Golden("finalmlp_adam")
    from fuxictr_amd.features import FeatureMap
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": 8})
    kw = dict(gpu=-1, embedding_dim=8, optimizer="adam", loss="binary_crossentropy", task="binary_classification",
              metrics=["AUC"], verbose=0, model_root=str(tmp_path))
    with pytest.raises(AssertionError, match="divisible by num_heads"):
        zoo.FinalMLP(fmap, mlp1_hidden_units=[16, 6], mlp2_hidden_units=[8], num_heads=4, **kw)
    with pytest.raises(TypeError):
        layers.FeatureSelection(fmap, 80, 8, [16], [], [], "extra")
    # the reference's defaults
    import inspect
    sig = inspect.signature(zoo.FinalMLP.__init__).parameters
    assert sig["embedding_dim"].default == 10 and sig["fs_hidden_units"].default == [64]
    assert sig["num_heads"].default == 1 and sig["use_fs"].default is True and sig["fs1_context"].default == []
    assert sig["mlp1_hidden_units"].default == [64, 64, 64]
    assert inspect.signature(zoo.DualMLP.__init__).parameters["mlp2_hidden_units"].default == [64, 64, 64]


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib
    for name in ("fx_gate2_fwd", "fx_gate2_bwd", "fx_gate2_workspace_floats", "fx_biagg_fwd", "fx_biagg_bwd",
                 "fx_biagg_workspace_floats", "fx_finalmlp_slab_rows"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    one = 16        # (any non-null address: validation happens before anything is read)
    st = lib.fx_gate2_fwd(one, 8, 4, 0, one, 8, None, 0, one, 8, None, 0, None)
    assert st == 1 and b"W=0" in lib.fx_last_error()
    st = lib.fx_gate2_fwd(None, 8, 4, 8, one, 8, None, 0, one, 8, None, 0, None)
    assert st == 1 and b"null E" in lib.fx_last_error()
    st = lib.fx_gate2_fwd(one, 7, 4, 8, one, 8, None, 0, one, 8, None, 0, None)
    assert st == 1 and b"E row stride" in lib.fx_last_error()
    st = lib.fx_gate2_fwd(one, 8, 4, 8, one, 4, None, 0, one, 8, None, 0, None)
    assert st == 1 and b"Z1 row stride" in lib.fx_last_error() and b"broadcast" in lib.fx_last_error()
    st = lib.fx_gate2_fwd(one, 8, 4, 8, one, 0, one, 0, one, 8, None, 8, None)
    assert st == 1 and b"null F2" in lib.fx_last_error()
    st = lib.fx_gate2_bwd(one, 8, None, 0, one, 8, 0, 8, one, 8, None, 0, one, 8, 0, one, 8, None, 0, None, None)
    assert st == 1 and b"B=0" in lib.fx_last_error()
    st = lib.fx_gate2_bwd(one, 8, None, 0, one, 8, 4, 8, one, 0, None, 0, one, 8, 0, one, 0, None, 0, None, None)
    assert st == 1 and b"workspace" in lib.fx_last_error()
    st = lib.fx_gate2_bwd(one, 8, None, 0, one, 8, 4, 8, one, 8, None, 0, one, 8, 0, one, 4, None, 0, None, None)
    assert st == 1 and b"dZ1 row stride" in lib.fx_last_error()
    st = lib.fx_biagg_fwd(one, 8, one, 8, one, 8, 4, 0, 8, one, one, None, None, None, one, None)
    assert st == 1 and b"dx=0" in lib.fx_last_error()
    st = lib.fx_biagg_fwd(one, 8, one, 7, one, 8, 4, 8, 8, one, one, None, None, None, one, None)
    assert st == 1 and b"row stride" in lib.fx_last_error()
    st = lib.fx_biagg_fwd(one, 8, one, 8, None, 8, 4, 8, 8, one, one, None, None, None, one, None)
    assert st == 1 and b"null X / Y / T" in lib.fx_last_error()
    st = lib.fx_biagg_bwd(one, one, 8, one, 8, one, 8, 4, 8, 8, one, one, one, 8, one, 8, None, 0, one, one, one,
                          None, None)
    assert st == 1 and b"workspace" in lib.fx_last_error()
    st = lib.fx_biagg_bwd(one, one, 8, one, 8, one, 8, 4, 8, 8, one, one, one, 8, one, 8, one, 7, one, one, one,
                          one, None)
    assert st == 1 and b"dXr" in lib.fx_last_error()
    # slabs of 16 rows up to 256 of them, longer ones beyond; one partial per slab
    assert lib.fx_finalmlp_slab_rows(1) == 16 and lib.fx_finalmlp_slab_rows(4096) == 16
    assert lib.fx_finalmlp_slab_rows(10000) == 40
    assert lib.fx_gate2_workspace_floats(1, 624) == 2 * 624
    assert lib.fx_gate2_workspace_floats(33, 50) == 3 * 2 * 50
    assert lib.fx_gate2_workspace_floats(10000, 624) == 250 * 2 * 624
    assert lib.fx_biagg_workspace_floats(4096, 512, 256) == 256 * (512 + 256 + 1)
    assert lib.fx_biagg_workspace_floats(0, 512, 256) == 0
