"""CrossNetMix without a GPU: the layer's checkpoint surface, the entry points' argument checks (status 1 and a
message before the device is touched), the envelope, and the drop-in binding of patch.install()."""
import ctypes
import importlib
import os

import pytest
import torch

from fuxictr_amd import _lib, layers, ops
from test_dropin_reference_zoo import REF, patched_reference  # noqa: F401  (the checkout's place, the fixture)
from zoo_cases import build_from_golden

MIX_CASES = ["dcnv2_mix_parallel_adam", "dcnv2_mix_crossonly_d10_sgd", "dcnv2_mix_stacked_e1", "dcnv2_mix_sp_r8_e3"]


def build_mix(model_cls, g, tmp_path, gpu=-1, **extra):
    """zoo.DCNv2 (or the reference's class) with a fixture's hyper-parameters and initial weights."""
    m = g.meta
    return build_from_golden(model_cls, g, tmp_path, gpu=gpu, model_structure=m["structure"], use_low_rank_mixture=True,
                             low_rank=m["low_rank"], num_experts=m["num_experts"], num_cross_layers=m["n_cross"],
                             stacked_dnn_hidden_units=m["stacked"], parallel_dnn_hidden_units=m["hidden"],
                             dnn_activations="relu", **extra)


def test_layer_has_the_reference_checkpoint_surface():
    torch.manual_seed(0)
    m = layers.CrossNetMix(40, layer_num=3, low_rank=8, num_experts=2)
    want = {"gating.%d.weight" % e: (1, 40) for e in range(2)}
    for l in range(3):
        want.update({"U_list.%d" % l: (2, 40, 8), "V_list.%d" % l: (2, 40, 8), "C_list.%d" % l: (2, 8, 8),
                     "bias.%d" % l: (40, 1)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert (m.layer_num, m.num_experts) == (3, 2)
    # xavier_normal_ on [E, W, r]: fan_in = W r, fan_out = E r; nn.Linear's uniform of bound 1 / sqrt(W); zeros
    for p, (fi, fo) in ((m.U_list[0], (40 * 8, 2 * 8)), (m.C_list[0], (8 * 8, 2 * 8))):
        assert abs(float(p.detach().std()) / (2.0 / (fi + fo)) ** 0.5 - 1.0) < 0.25
    assert float(m.gating[0].weight.abs().max()) <= 40 ** -0.5 and float(m.bias[1].abs().max()) == 0.0


def test_limits_are_the_documented_envelope():
    lim = ops.crossmix_limits()
    assert lim == {"tile_rows": 16, "W_max": 4096, "r_max": 64, "E_max": 16, "Er_max": 256, "layers_max": 8,
                   "workgroups_max": 512}
    ops.crossmix_check(2048, 32, 4, 8)
    ops.crossmix_check(624, 64, 1, 3)
    with pytest.raises(NotImplementedError, match="num_experts\\*low_rank <= 256"):
        layers.CrossNetMix(16, low_rank=64, num_experts=5)


@pytest.mark.parametrize("what, r, E, L, nulls", [("null U / V / C / bias / gate list", 8, 2, 2, True),
                                                  ("num_experts*low_rank=320", 64, 5, 2, False),
                                                  ("layers=0", 8, 2, 0, False)])
def test_entry_points_refuse_before_touching_the_device(what, r, E, L, nulls):
    lib = _lib.load()
    one = (ctypes.c_void_p * 16)(*([1] * 16))                   # non-null pointers that are never followed
    lists = [None] * 5 if nulls else [one] * 5
    st = lib.fx_crossmix_fwd(1, 24, 4, 24, r, E, L, *lists, 1, 24, 1, 1, None)
    assert st == 1 and what.encode() in lib.fx_last_error(), lib.fx_last_error()
    st = lib.fx_crossmix_bwd(1, 24, 1, 24, 4, 24, r, E, L, *lists, 1, 1, 24, 1, 1, 1, 1, 1, 1, None)
    assert st == 1 and what.encode() in lib.fx_last_error(), lib.fx_last_error()
    assert (lib.fx_crossmix_workspace_floats(4, 24, r, E, L) == 0) == (not nulls)      # 0 outside the envelope


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "fuxictr")), reason="reference checkout not present")
def test_patch_binds_the_reference_name_to_the_native_layer(patched_reference):  # noqa: F811
    from fuxictr.pytorch.layers.interactions import cross_net
    model_file = importlib.import_module("model_zoo.DCNv2.src.DCNv2")
    assert cross_net.CrossNetMix is layers.CrossNetMix and model_file.CrossNetMix is layers.CrossNetMix
