"""DIEN end to end on a real MI355X: zoo.DIEN on the native layers (the recurrent layers and the attention scores on
csrc/fx_gru.hip) against the fixtures recorded from the REAL reference's model_zoo.DIEN
(tests/golden/make_golden_dien.py), with the tolerances of tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import pytest

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import zoo  # noqa: E402
from test_dien_host import DIEN_CASES, build_dien  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402


def build_native(g, tmp_path, sparse_update="exact", hip_graph=False):
    return build_dien(zoo.DIEN, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph)


@pytest.mark.parametrize("case", DIEN_CASES)
def test_forward_logits_match_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", DIEN_CASES)
def test_training_trajectory_matches_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_trajectory(model, g)


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits; the capture really
    happened (`_graph_state`), it did not fall back to eager: the lengths never leave the device."""
    g = Golden("dien_augru_pair_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)
