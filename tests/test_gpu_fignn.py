"""FiGNN end to end on a real MI355X: zoo.FiGNN on the native layers (the graph propagation and the head on
csrc/fx_fignn.hip) against the fixtures recorded from the REAL reference's model_zoo.FiGNN
(tests/golden/make_golden_fignn.py), with the tolerances of tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import pytest

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import zoo  # noqa: E402
from test_fignn_host import FIGNN_CASES, build_fignn  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402


def build_native(g, tmp_path, sparse_update="exact", hip_graph=False):
    return build_fignn(zoo.FiGNN, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph)


@pytest.mark.parametrize("case", FIGNN_CASES)
def test_forward_logits_match_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", FIGNN_CASES)
def test_training_trajectory_matches_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_trajectory(model, g)


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order, no atomics -> same bits; the capture
    really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("fignn_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)
