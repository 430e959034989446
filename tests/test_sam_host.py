"""SAM (all four interaction types) on the native layers, host side (no GPU): zoo.SAM with gpu=-1, where layers.SAMBlock takes the
reference's own torch ops and the other kernels are replaced by the torch-CPU emulations of tests/_cpu_emul.py, against
fixtures recorded from the REAL reference's model_zoo.SAM (tests/golden/make_golden_sam.py).  Checks the parameter
names, the forward composition and the optimizer protocol; the HIP kernels themselves are held to fp64 in
tests/test_gpu_sam_kernel.py.

Stated tolerances (those of tests/zoo_cases.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

SAM_CASES = ["sam_zoo_test", "sam_2a_adam", "sam_3a_weighted_res_adam", "sam_3e_concat_sgd"]


def sam_reference(kind, X, W, w, bias):
    """fc(flatten(SAM2A / SAM2E block of X [B, F, D])) [B] in plain torch (SAM.py:172-173, :199-201, :88): W [F, F, D]
    (SAM2A), w = fc.weight viewed [F, F, D], bias [1]; the [B, F, F, D] tensor is formed."""
    S = torch.bmm(X, X.transpose(1, 2))
    out = S.unsqueeze(-1) * (W if kind == "SAM2A" else torch.einsum("bnd,bmd->bnmd", X, X))
    return out.flatten(start_dim=1) @ w.reshape(-1) + bias


def sam_layer_reference(kind, X, K, Q, W):
    """One SAM3A / SAM3E layer (SAM.py:234-240, :268-275) in plain torch: K, Q (None: no residual) [D, D] as nn.Linear
    weights, W [F, F, D] (SAM3A); the [B, F, F, D] tensor is formed."""
    S = torch.bmm(X, (X @ K.T).transpose(1, 2))
    out = (S.unsqueeze(-1) * (W if kind == "SAM3A" else torch.einsum("bnd,bmd->bnmd", X, X))).sum(dim=2)
    return out if Q is None else out + X @ Q.T


def build_sam(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.SAM with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_sam.py)."""
    kw = dict(interaction_type=g.meta["interaction_type"], aggregation=g.meta["aggregation"],
              num_interaction_layers=g.meta["num_interaction_layers"], use_residual=g.meta["use_residual"],
              net_dropout=0)
    kw.update(extra)
    return build_from_golden(zoo.SAM, g, tmp_path, gpu=gpu, **kw)


def _build(g, tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_sam(zoo, g, tmp_path)


@pytest.mark.parametrize("case", SAM_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    F, D = model.feature_map.num_fields, g.meta["embedding_dim"]
    kind = g.meta["interaction_type"]
    width = D if g.meta["aggregation"] != "concat" else F * D * (F if kind in ("SAM2A", "SAM2E") else 1)
    assert tuple(g.state0["fc.weight"].shape) == (1, width) and "fc.bias" in g.state0
    assert ("block.layers.0.W" in g.state0) == (kind in ("SAM2A", "SAM3A"))
    assert ("block.layers.1.K.weight" in g.state0) == (kind in ("SAM3A", "SAM3E"))
    assert ("block.layers.0.Q.weight" in g.state0) == bool(g.meta["use_residual"])
    assert ("block.weight" in g.state0) == (g.meta["aggregation"] == "weighted_pooling")
    assert 1e-2 <= g.meta["block_absmax"] <= 10.0        # the generator's window
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", SAM_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    check_trajectory(_build(g, tmp_path, monkeypatch), g)


def test_constructor_raises_outside_the_envelope_for_pooling_and_for_dropout(tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops, zoo
    g = Golden("sam_2a_adam")
    lim = ops.sam_limits()
    assert (lim["F_max"], lim["D_max"]) == (64, 64)
    with pytest.raises(NotImplementedError, match="embedding_dim <= 64"):
        build_sam(zoo, g, tmp_path, embedding_dim=65)
    for kind in ("SAM2A", "SAM2E"):
        with pytest.raises(AssertionError, match="Only aggregation=concat"):
            build_sam(zoo, g, tmp_path, interaction_type=kind, aggregation="sum_pooling")
        with pytest.raises(NotImplementedError, match="net_dropout=0.1"):
            build_sam(zoo, g, tmp_path, interaction_type=kind, net_dropout=0.1)
    with pytest.raises(ValueError, match="not supported"):
        build_sam(zoo, g, tmp_path, interaction_type="SAM4")


def test_entry_points_validate_before_the_device():
    from fuxictr_amd import _lib
    lib = _lib.load()

    def fwd(B, F, D, kind, x_ld=1 << 20):
        return lib.fx_sam_logit_fwd(None, x_ld, B, F, D, kind, *[None] * 6)

    def bwd(B, F, D, kind, x_ld=1 << 20):
        return lib.fx_sam_logit_bwd(None, x_ld, B, F, D, kind, None, None, None, None, 1 << 20, 0, *[None] * 5)
    for call in (fwd, bwd):
        assert call(4, 65, 8, 0) == 1 and b"F <= 64" in lib.fx_last_error()
        assert call(4, 8, 65, 1) == 1 and b"D <= 64" in lib.fx_last_error()
        assert call(4, 8, 8, 2) == 1 and b"type=2" in lib.fx_last_error()
        assert call(4, 8, 8, 0, x_ld=63) == 1 and b"stride" in lib.fx_last_error()
        assert call(4, 8, 8, 0) == 1 and b"null X" in lib.fx_last_error()

    def lfwd(B, F, D, kind, x_ld=1 << 20):
        return lib.fx_sam_layer_fwd(None, x_ld, B, F, D, kind, *[None] * 6)

    def lbwd(B, F, D, kind, x_ld=1 << 20):
        return lib.fx_sam_layer_bwd(None, x_ld, B, F, D, kind, None, None, None, None, None, 1 << 20, 0, *[None] * 5)
    for call in (lfwd, lbwd):
        assert call(4, 65, 8, 2) == 1 and b"F <= 64" in lib.fx_last_error()
        assert call(4, 8, 65, 3) == 1 and b"D <= 64" in lib.fx_last_error()
        assert call(4, 8, 8, 1) == 1 and b"type=1" in lib.fx_last_error()
        assert call(4, 8, 8, 2, x_ld=63) == 1 and b"stride" in lib.fx_last_error()
        assert call(4, 8, 8, 3) == 1 and b"null X" in lib.fx_last_error()
    for shape in ((4, 65, 8, 0), (4, 8, 65, 1), (4, 8, 8, 4), (4, 65, 8, 2)):
        assert lib.fx_sam_workspace_floats(*shape) == 0
    # S / dS [B, F, F], a dK | dQ partial row per workgroup (one per sample here); 3A past 256 samples: dW's slabs
    assert lib.fx_sam_workspace_floats(9, 20, 8, 2) == 9 * 400 + 9 * 128
    assert lib.fx_sam_workspace_floats(9, 20, 8, 3) == 9 * 128
    assert lib.fx_sam_workspace_floats(600, 20, 8, 2) == 600 * 400 + 512 * 128 + 3 * 3200
    # F 20 -> 2 x 2 tiles of 16, 3 of them on or above the diagonal; B 9 at <= 4 samples per tile -> 3 workgroups
    assert lib.fx_sam_workspace_floats(9, 20, 8, 0) == 400 + (3 + 1) * (3 * 256 + 4)
    # the two wsym layouts, dlogit S [B, F, F], a 4-float partial row per workgroup and their sum
    assert lib.fx_sam_workspace_floats(9, 20, 8, 1) == 2 * 3200 + 9 * 400 + (3 + 1) * 4
