"""MaskNet on the native layers, host side (no GPU): zoo.MaskNet + layers.FieldLayerNorm / LayerNorm / MaskBlock /
SerialMaskNet / ParallelMaskNet wired end to end with the kernels replaced by torch-CPU emulations —
tests/_cpu_emul.py for the existing ops, the fx_layernorm_* / fx_mask_grad wrappers emulated here from their
formulas in fp32 torch (checked against torch's own LayerNorm and autograd below) — against fixtures recorded
from the REAL reference's model_zoo.MaskNet (tests/golden/make_golden_masknet.py).  Checks the parameter names (the per-field `emb_norm.<i>.*`
views of one packed storage included), the fused composition (one stage node per block / per parallel stage, the
mask product in a GEMM epilogue, blocks side by side without a cat), the module-by-module one, the autograd
nodes' plumbing and the optimizer protocol; the HIP kernels themselves are held to an fp64 restatement in
tests/test_gpu_layernorm.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, losses 1e-4 per step, trained weights
through conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden, assert_weights_close
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

MASKNET_CASES = ["masknet_serial_adam", "masknet_parallel_adam", "masknet_zoo_test", "masknet_plain_sgd"]


def layernorm_reference(X, G, N, gamma, beta, eps, relu):
    """-> (Y [rows, G*N], mu [rows, G], rstd [rows, G]) from the formulas, in the dtype of the arguments: biased
    variance of the centred values, eps inside the square root."""
    x = X[:, :G * N].reshape(X.shape[0], G, N)
    mu = x.mean(dim=-1, keepdim=True)
    d = x - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps)
    z = d * rstd * gamma.reshape(G, N) + beta.reshape(G, N)
    if relu:
        z = torch.relu(z)
    return z.reshape(X.shape[0], G * N), mu.squeeze(-1), rstd.squeeze(-1)


def mask_grad_reference(dM, Vmask, H, nb):
    rows = dM.shape[0]
    return (dM[:, :nb * H] * Vmask[:, :nb * H]).reshape(rows, nb, H).sum(dim=1)


def _emul_layernorm_fwd(X, G, N, gamma, beta, eps, relu, Y, stats, y_col=0):
    with torch.no_grad():
        y, mu, rstd = layernorm_reference(X, G, N, gamma, beta, eps, relu)
        Y[:, y_col:y_col + G * N].copy_(y)
        stats.view(-1, G, 2).copy_(torch.stack([mu, rstd], dim=-1))
    return Y


def _emul_layernorm_bwd(X, G, N, gamma, relu, Y, stats, dY, dX, dgamma, dbeta, workspace, y_col=0, dy_col=0,
                        dx_accumulate=False):
    """The backward's formulas on the saved statistics (the entry point is not given eps: it only enters through
    rstd).  tests/test_gpu_layernorm.py holds the kernel to autograd in fp64."""
    with torch.no_grad():
        rows = X.shape[0]
        g = dY[:, dy_col:dy_col + G * N]
        if relu:                                # the mask is the sign of the forward's own Y
            g = g * (Y[:, y_col:y_col + G * N] > 0).to(g.dtype)
        g = g.reshape(rows, G, N)
        st = stats.view(rows, G, 2)
        mu, rstd = st[:, :, 0:1], st[:, :, 1:2]
        xh = (X[:, :G * N].reshape(rows, G, N) - mu) * rstd
        gh = g * gamma.reshape(G, N)
        gx = rstd * (gh - gh.mean(dim=-1, keepdim=True) - xh * (gh * xh).mean(dim=-1, keepdim=True))
        gx = gx.reshape(rows, G * N)
        dX[:, :G * N].add_(gx) if dx_accumulate else dX[:, :G * N].copy_(gx)
        dgamma.copy_((g * xh).sum(dim=0).reshape(dgamma.shape))
        dbeta.copy_(g.sum(dim=0).reshape(dbeta.shape))
    return dX, dgamma, dbeta


def _emul_mask_grad(dM, Vmask, H, nb, out, accumulate=False):
    with torch.no_grad():
        t = mask_grad_reference(dM, Vmask, H, nb)
        out[:, :H].add_(t) if accumulate else out[:, :H].copy_(t)
    return out


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "layernorm_fwd", _emul_layernorm_fwd)
    monkeypatch.setattr(ops, "layernorm_bwd", _emul_layernorm_bwd)
    monkeypatch.setattr(ops, "mask_grad", _emul_mask_grad)
    monkeypatch.setattr(ops, "layernorm_workspace_floats", lambda rows, G, N: 1)


def build_masknet(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.MaskNet with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_masknet.py)."""
    m = g.meta
    return build_from_golden(zoo.MaskNet, g, tmp_path, gpu=gpu, dnn_hidden_units=m["hidden"],
                             model_type=m["model_type"], parallel_num_blocks=m["num_blocks"],
                             parallel_block_dim=m["block_dim"], reduction_ratio=m["ratio"],
                             emb_layernorm=m["emb_layernorm"], net_layernorm=m["net_layernorm"], **extra)


def _build(g, tmp_path, monkeypatch, **extra):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_masknet(zoo, g, tmp_path, **extra)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", MASKNET_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts keys, shapes, dtypes)
    assert "mask_net.mask_blocks.0.mask_layer.2.bias" in g.state0
    assert "mask_net.mask_blocks.0.hidden_layer.0.bias" not in g.state0
    assert ("emb_norm.0.weight" in g.state0) == bool(g.meta["emb_layernorm"])
    assert ("mask_net.mask_blocks.0.hidden_layer.1.weight" in g.state0) == bool(g.meta["net_layernorm"])
    assert ("mask_net.dnn.mlp.0.weight" in g.state0) == (g.meta["model_type"] == "ParallelMaskNet")
    assert ("mask_net.fc.0.weight" in g.state0) == (g.meta["model_type"] == "SerialMaskNet")
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", MASKNET_CASES)
def test_training_trajectory_and_trained_weights(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch, fused=fused)
    check_trajectory(model, g)


@pytest.mark.parametrize("case", MASKNET_CASES)
def test_fused_and_module_by_module_routes_agree(case, tmp_path, monkeypatch):
    g = Golden(case)
    a = _build(g, tmp_path, monkeypatch, fused=True)
    b = _build(g, tmp_path, monkeypatch, fused=False)
    assert a._fused and a.mask_net.fused and not b._fused and not b.mask_net.fused
    a.train(), b.train()
    for i in range(g.meta["steps"]):
        la, lb = float(a.train_step(tb(g.batches[i])).item()), float(b.train_step(tb(g.batches[i])).item())
        assert abs(la - lb) <= 1e-5, (i, la, lb)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert_weights_close(sa[k].numpy(), sb[k].numpy(), g.meta["lr"], g.meta["steps"], k)


def test_fixtures_exercise_the_layernorms_their_relus_and_the_mask():
    """What make_golden_masknet.py asserted when it wrote the fixtures, re-read from their meta."""
    for case in MASKNET_CASES:
        m = Golden(case).meta
        assert len(m["relu_zero_share"]) == (len(m["hidden"]) if m["model_type"] == "SerialMaskNet"
                                             else m["num_blocks"]) * int(m["net_layernorm"])
        for z in m["relu_zero_share"]:
            assert 0.1 <= z <= 0.9, (case, z)
        assert m["emb_var_share"] >= 0.9, (case, m["emb_var_share"])
        assert m["mask_share"] >= 0.05, (case, m["mask_share"])
    assert Golden("masknet_parallel_adam").meta["embedding_dim"] % 4 != 0          # the scalar path
    assert Golden("masknet_plain_sgd").meta["net_reg"] > 0


def test_emb_norm_parameters_are_views_of_one_packed_storage(tmp_path, monkeypatch):
    """state_dict / load_state_dict / reset_parameters / the dense optimizer see 2 F ordinary Parameters; the
    kernel sees one [2, F, D] tensor."""
    g = Golden("masknet_serial_adam")
    model = _build(g, tmp_path, monkeypatch)
    F, D = model.num_fields, g.meta["embedding_dim"]
    norm = model.emb_norm
    assert len(norm) == F and tuple(norm._packed.shape) == (2, F, D)
    names = dict(model.named_parameters())
    for i in range(F):
        w, b = names["emb_norm.%d.weight" % i], names["emb_norm.%d.bias" % i]
        assert isinstance(w, torch.nn.Parameter) and tuple(w.shape) == (D,) and w.requires_grad
        assert w.data_ptr() == norm._packed[0, i].data_ptr() and b.data_ptr() == norm._packed[1, i].data_ptr()
    dense = [p for grp in model.optimizer.param_groups for p in grp["params"]]
    assert sum(any(p is names["emb_norm.%d.%s" % (i, s)] for p in dense) for i in range(F)
               for s in ("weight", "bias")) == 2 * F
    # load_state_dict writes through the views; state_dict reads the same numbers back
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for i in range(F):
        sd["emb_norm.%d.weight" % i] = torch.full((D,), 1.0 + i)
        sd["emb_norm.%d.bias" % i] = torch.full((D,), -0.5 * i)
    model.load_state_dict(sd, strict=True)
    assert torch.equal(norm._packed[0], (1.0 + torch.arange(F, dtype=torch.float32))[:, None].expand(F, D))
    assert torch.equal(norm._packed[1], (-0.5 * torch.arange(F, dtype=torch.float32))[:, None].expand(F, D))
    back = model.state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    # fixture round trip: state0 in, state0 out
    s0 = {k: torch.from_numpy(v) for k, v in g.state0.items()}
    model.load_state_dict(s0, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, s0[k]), k
    # reset_parameters leaves a LayerNorm's ones / zeros alone, as the reference's does; .to() keeps the aliasing
    model.reset_parameters()
    model.to(torch.device("cpu"))
    model.float()
    assert norm[3].weight.data_ptr() == norm._packed[0, 3].data_ptr()
    # a training step moves the packed storage (the optimizer updates the views in place)
    before = norm._packed.clone()
    model.train()
    model.train_step(tb(g.batches[0]))
    assert not torch.equal(before, norm._packed)
    assert norm[0].weight.data_ptr() == norm._packed[0, 0].data_ptr()


def test_layers_alone_match_torch(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    torch.manual_seed(5)
    x = torch.randn(6, 12, requires_grad=True)
    ln, ref = layers.LayerNorm(12), torch.nn.LayerNorm(12)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(12)), ln.bias.copy_(torch.randn(12))
        ref.weight.copy_(ln.weight), ref.bias.copy_(ln.bias)
    assert sorted(ln.state_dict()) == ["bias", "weight"]
    for relu in (False, True):
        y = ln(x, relu=relu)
        y2 = ref(x).relu() if relu else ref(x)
        assert torch.allclose(y, y2, atol=1e-6)
        gy = torch.randn_like(y)
        got = torch.autograd.grad(y, [x, ln.weight, ln.bias], gy)
        want = torch.autograd.grad(y2, [x, ref.weight, ref.bias], gy)
        for a, b in zip(got, want):
            assert torch.allclose(a, b, atol=1e-5)
    # the per-field norm against one torch LayerNorm per field
    emb = torch.randn(5, 3, 4, requires_grad=True)
    fn = layers.FieldLayerNorm(3, 4)
    with torch.no_grad():
        fn._packed.copy_(torch.randn(2, 3, 4))
    out = fn(emb)
    want = torch.cat([torch.nn.functional.layer_norm(emb[:, i], (4,), fn[i].weight, fn[i].bias) for i in range(3)],
                     dim=1)
    assert tuple(out.shape) == (5, 12) and torch.allclose(out, want, atol=1e-6)
    gy = torch.randn_like(out)
    params = [p for m in fn for p in (m.weight, m.bias)]
    got = torch.autograd.grad(out, [emb] + params, gy)
    ref_grads = torch.autograd.grad(want, [emb] + params, gy)
    for a, b in zip(got, ref_grads):
        assert torch.allclose(a, b, atol=1e-5)


@pytest.mark.parametrize("kw", [dict(layer_norm=False), dict(hidden_activation="Tanh"), dict(dropout_rate=0.5),
                                dict()], ids=["no-layernorm", "tanh", "dropout", "fused"])
def test_mask_block_combinations_run_after_the_fused_prefix(kw, monkeypatch):
    """LayerNorm off, another activation, dropout: the stage node ends at the hidden GEMM and hidden_layer[1:]
    runs module by module — the same numbers as the reference's composition (eval mode: dropout is the identity)."""
    _install(monkeypatch)
    from fuxictr_amd import layers
    torch.manual_seed(2)
    blocks = [layers.MaskBlock(12, 12, 6, reduction_ratio=1.5, **kw) for _ in range(2)]
    assert blocks[0].mask_layer[0].out_features == 18 and blocks[0].hidden_layer[0].bias is None
    assert blocks[0]._ln_fused == (not kw)
    for b in blocks:
        b.eval()
        for lin in (b.mask_layer[0], b.mask_layer[2], b.hidden_layer[0]):
            torch.nn.init.normal_(lin.weight, std=0.4)
    v_emb = torch.randn(7, 12, requires_grad=True)
    v_hid = torch.randn(7, 12, requires_grad=True)
    for group in ([blocks[0]], blocks):
        got = layers.mask_stage(group, v_emb, v_hid)
        want = torch.cat([b(v_emb, v_hid) for b in group], dim=-1)
        assert tuple(got.shape) == (7, 6 * len(group)) and torch.allclose(got, want, atol=1e-5)
        params = [p for b in group for p in b.parameters()]
        gy = torch.randn_like(got)
        ga = torch.autograd.grad(got, [v_emb, v_hid] + params, gy)
        gb = torch.autograd.grad(want, [v_emb, v_hid] + params, gy)
        for a, b in zip(ga, gb):
            assert torch.allclose(a, b, atol=1e-4), (a - b).abs().max()


def test_reduction_ratio_is_truncated_as_the_reference_does(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    assert layers.MaskBlock(100, 100, 8, reduction_ratio=0.5).mask_layer[0].out_features == 50
    assert layers.MaskBlock(100, 33, 8, reduction_ratio=0.35).mask_layer[0].out_features == int(33 * 0.35)
    assert layers.MaskBlock(100, 7, 8, reduction_ratio=2.9).mask_layer[2].in_features == int(7 * 2.9)
    with pytest.raises(ValueError, match="reduction_ratio"):
        layers.MaskBlock(100, 3, 8, reduction_ratio=0.1)
    net = layers.ParallelMaskNet(30, output_dim=1, num_blocks=2, block_dim=5, hidden_units=[7], reduction_ratio=0.5)
    assert sorted(k for k in net.state_dict() if k.endswith("weight")) == sorted(
        ["dnn.mlp.0.weight", "dnn.mlp.2.weight"]
        + ["mask_blocks.%d.%s.weight" % (i, n) for i in range(2)
           for n in ("mask_layer.0", "mask_layer.2", "hidden_layer.0", "hidden_layer.1")])


def test_limits_and_unknown_options_raise(tmp_path, monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers, ops, zoo
    with pytest.raises(NotImplementedError, match="N=8193"):
        layers.LayerNorm(8193)
    with pytest.raises(NotImplementedError, match="N=8193"):
        layers.MaskBlock(16, 16, 8193)
    with pytest.raises(NotImplementedError, match="G=65"):
        layers.FieldLayerNorm(65, 8)
    with pytest.raises(NotImplementedError, match="N=0"):
        ops.layernorm_check(1, 0)
    with pytest.raises(NotImplementedError, match="built for"):
        layers.FieldLayerNorm(4, 8)(torch.zeros(2, 5, 8))
    layers.LayerNorm(8192), layers.FieldLayerNorm(64, 4)               # the limits themselves are accepted
    g = Golden("masknet_serial_adam")
    from fuxictr_amd.features import FeatureMap
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": 8})
    with pytest.raises(ValueError, match="model_type=MaskNetSerial"):
        zoo.MaskNet(fmap, model_type="MaskNetSerial", gpu=-1, embedding_dim=8, optimizer="adam",
                    loss="binary_crossentropy", task="binary_classification", metrics=["AUC"], verbose=0,
                    model_root=str(tmp_path))


def test_entry_points_are_declared_and_validate_before_the_device():
    from fuxictr_amd import _lib, patch
    for name in ("fx_layernorm_fwd", "fx_layernorm_bwd", "fx_layernorm_workspace_floats", "fx_mask_grad"):
        assert name in _lib.SIGNATURES
    assert "MaskBlock" not in patch.LAYER_NAMES          # the reference's MaskBlock lives in its model file
    lib = _lib.load()
    st = lib.fx_layernorm_fwd(None, 8193, 4, 1, 8193, None, None, 1e-5, 0, None, 8193, 0, None, None)
    assert st == 1 and b"N <= 8192" in lib.fx_last_error()
    st = lib.fx_layernorm_fwd(None, 65 * 4, 4, 65, 4, None, None, 1e-5, 0, None, 65 * 4, 0, None, None)
    assert st == 1 and b"G <= 64" in lib.fx_last_error()
    st = lib.fx_layernorm_fwd(None, 8, 0, 2, 8, None, None, 1e-5, 0, None, 16, 0, None, None)
    assert st == 1 and b"row stride" in lib.fx_last_error()
    st = lib.fx_layernorm_bwd(None, 16, 0, 2, 8, None, 1, None, 16, 0, None, None, 16, 0, None, 16, 0, None, None,
                              None, None)
    assert st == 1 and b"rows=0" in lib.fx_last_error()
    st = lib.fx_mask_grad(None, 4, None, 8, 0, 4, 2, None, 4, 0, None)
    assert st == 1 and b"row stride" in lib.fx_last_error()
    # one partial pair per slab of rows: never more slabs than rows, at most 256
    assert lib.fx_layernorm_workspace_floats(1, 39, 16) == 2 * 624
    assert lib.fx_layernorm_workspace_floats(33, 5, 10) == 33 * 2 * 50
    assert lib.fx_layernorm_workspace_floats(4096, 39, 16) == 256 * 2 * 624
    assert lib.fx_layernorm_workspace_floats(4096, 1, 8192) == 32 * 2 * 8192
