"""FwFM and FmFM end to end on a real MI355X: zoo.FwFM / zoo.FmFM on the native layers (the field-pair interaction on
csrc/fx_pairfm.hip) against the fixtures recorded from the REAL reference's model_zoo.FwFM / model_zoo.FmFM
(tests/golden/make_golden_pairfm.py), with the tolerances of tests/test_gpu_afm.py / test_gpu_models.py:
  forward logits |d| <= 1e-4, pred atol 2e-5, loss trajectory |d| <= 1e-4 per step, trained weights
  conftest.assert_weights_close.
The kernels alone are held to the fp64 restatement in tests/test_gpu_pairfm_kernel.py.
"""
import pytest

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import zoo  # noqa: E402
from test_pairfm_host import PAIRFM_CASES, build_pairfm  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402



def build_native(g, tmp_path, hip_graph=False, fused=True):
    return build_pairfm(zoo, g, tmp_path, gpu=0, hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", PAIRFM_CASES)
def test_forward_logits_match_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    assert model._fused == fused and model._native
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", PAIRFM_CASES)
def test_training_trajectory_matches_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_trajectory(model, g)


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits (no atomics in the
    kernels); the capture really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("fmfm_matrixed_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)
