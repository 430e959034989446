"""FFMv2 and ONNv2 on the native layers, host side (no GPU): zoo.FFMv2 / zoo.ONNv2 with gpu=-1, where
layers.field_aware_interaction takes the torch composition and the other kernels are replaced by the torch-CPU
emulations of tests/_cpu_emul.py, against fixtures recorded from the REAL reference's FFMv2 and ONNv2
(tests/golden/make_golden_ffm.py).  Checks the parameter names, the forward composition (the slot rule included) and
the optimizer protocol; the HIP kernels themselves are held to fp64 in tests/test_gpu_ffm_kernel.py.

Stated tolerances (those of tests/zoo_cases.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close."""
import os

import pytest

import _cpu_emul
from conftest import GOLDEN, Golden
from zoo_cases import OMIT, allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

FFM_CASES = ["ffmv2_adam", "ffmv2_sgd", "onnv2_adam", "onnv2_zoo_test"]


def build_ffm(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.FFMv2 / zoo.ONNv2 with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_ffm.py).
    FFMv2 takes one `regularizer`, which feeds the embedding and the net regularizer."""
    m = g.meta
    if m["model"] == "FFMv2":
        own = dict(regularizer=m["regularizer"], embedding_regularizer=OMIT, net_regularizer=OMIT)
    else:
        own = dict(hidden_units=m["hidden_units"], hidden_activations=m["hidden_activations"], net_dropout=0,
                   batch_norm=False)
    own.update(extra)
    return build_from_golden(getattr(zoo, m["model"]), g, tmp_path, gpu=gpu, **own)


def _build(g, tmp_path, monkeypatch, **extra):
    _cpu_emul.install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_ffm(zoo, g, tmp_path, **extra)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", FFM_CASES)
def test_state_dict_keys_and_forward_logits(case, fused, tmp_path, monkeypatch):
    g = Golden(case)
    m = g.meta
    model = _build(g, tmp_path, monkeypatch, fused=fused)            # (asserts the keys, shapes and dtypes)
    F, D = model.feature_map.num_fields, m["embedding_dim"]
    assert F == m["n_dense"] + len(m["cards"]) and model._fused == fused
    wide = [v for k, v in g.state0.items() if k.startswith("embedding_layer.") and v.ndim == 2 and min(v.shape) > 1]
    assert wide and all(v.shape[1] == D * (F if m["model"] == "ONNv2" else F - 1) for v in wide)
    assert not any("mask" in k for k in g.state0)                    # plain attributes in the reference
    if m["model"] == "ONNv2":
        assert g.state0["dnn.mlp.0.weight"].shape[1] == F * D + F * (F - 1) // 2
        assert tuple(model.diag_mask.shape) == tuple(model.triu_mask.shape) == (F, F)
    else:
        assert g.state0["lr_layer.bias"].shape == (1,)
    assert 1e-2 <= m["pair_absmax"] <= 10.0                          # the generator's window
    assert os.path.getsize(os.path.join(GOLDEN, case + ".npz")) <= \
        os.path.getsize(os.path.join(GOLDEN, "masknet_parallel_adam.npz"))
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", FFM_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    check_trajectory(_build(g, tmp_path, monkeypatch), g)


@pytest.mark.parametrize("case,too_wide", [("ffmv2_adam", 33), ("onnv2_adam", 29)])
def test_constructor_raises_at_a_table_row_wider_than_256(case, too_wide, tmp_path, monkeypatch):
    """9 fields: FFMv2 keeps 8 vectors per field (8 * 33 = 264), ONNv2 9 (9 * 29 = 261); 32 / 28 are the widest."""
    g = Golden(case)
    with pytest.raises(NotImplementedError, match="limit .* is 256"):
        _build(g, tmp_path, monkeypatch, embedding_dim=too_wide)


def test_entry_points_validate_before_the_device_and_tile_rows():
    from fuxictr_amd import _lib, ops
    lib = _lib.load()
    one = 16        # (any non-null address: validation happens before anything is read)
    big = 1 << 20

    def fwd(B, F, D, mode, X=one, ldx=big, addend=None, ldo=big):
        return lib.fx_ffm_fwd(X, ldx, B, F, D, mode, addend, one, ldo, None)

    def bwd(B, F, D, mode, X=one, ldx=big, lddx=big, ldg=big):
        return lib.fx_ffm_bwd(one, ldg, X, ldx, B, F, D, mode, one, lddx, None)
    for call in (fwd, bwd):
        assert call(4, 65, 1, 0) == 1 and b"F=65, limit" in lib.fx_last_error()
        assert call(4, 5, 52, 0) == 1 and b"C*D=260, limit 256" in lib.fx_last_error()
        assert call(4, 6, 0, 1) == 1 and b"D=0, limit" in lib.fx_last_error()
        assert call(4, 6, 4, 2) == 1 and b"mode=2" in lib.fx_last_error()
        assert call(-1, 6, 4, 0) == 1 and b"B=-1" in lib.fx_last_error()
        assert call(4, 6, 4, 0, ldx=143) == 1 and b"X row stride" in lib.fx_last_error()
        assert call(4, 6, 4, 0, X=None) == 1 and b"null" in lib.fx_last_error()
        assert call(0, 6, 4, 0, X=None) == 0                         # no rows
    assert fwd(4, 6, 4, 0, ldo=38) == 1 and b"out row stride" in lib.fx_last_error()       # 6 * 4 + 15 = 39
    assert fwd(4, 6, 4, 0, addend=one) == 1 and b"addend" in lib.fx_last_error()
    assert bwd(4, 6, 4, 1, lddx=119) == 1 and b"dX row stride" in lib.fx_last_error()      # 6 * 5 * 4 = 120
    assert bwd(4, 6, 4, 0, ldg=38) == 1 and b"g row stride" in lib.fx_last_error()
    lim = ops.ffm_limits()
    assert (lim["F_min"], lim["F_max"], lim["CD_max"]) == (2, 64, 256) and lim["workgroups"] >= 256
    assert ops.ffm_in_envelope("onn", 64, 4) and ops.ffm_in_envelope("ffm", 2, 256) and not ops.ffm_in_envelope("onn", 2, 129)
    # by hand.  LDS floats per sample: F rows of RS (C*D rounded up to VEC floats, + VEC where RS / VEC is even), the g
    # row (F*D + P with "onn", 1 with "ffm") and 4 for the waves' sums; once per workgroup the P pairs rounded up to 4.
    # T = what fits 80 KB = 20480 floats (one sample needs more: 160 KB), at most 32.
    assert ops.ffm_tile_rows("onn", 39, 4) == (20480 - 744) // (39 * 156 + 156 + 741 + 4) == 2
    assert ops.ffm_tile_rows("onn", 39, 2) == (20480 - 744) // (39 * 78 + 78 + 741 + 4) == 5
    assert ops.ffm_tile_rows("ffm", 39, 4) == (20480 - 744) // (39 * 156 + 1 + 4) == 3          # 152 -> 156
    assert ops.ffm_tile_rows("onn", 64, 4) == (40960 - 2016) // (64 * 260 + 256 + 2016 + 4) == 2  # 256 -> 260; whole
    assert ops.ffm_tile_rows("onn", 9, 3) == min(32, (20480 - 36) // (9 * 27 + 27 + 36 + 4)) == lim["tile_samples"]
    assert ops.ffm_tile_rows("ffm", 20, 3) == (20480 - 192) // (20 * 57 + 1 + 4) == 17            # an odd row as it is
    assert ops.ffm_tile_rows("onn", 65, 1) == 0 and ops.ffm_tile_rows("ffm", 6, 52) == 0
