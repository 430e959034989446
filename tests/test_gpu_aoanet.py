"""AOANet end to end on a real MI355X: zoo.AOANet on layers.GeneralizedInteractionNet (csrc/fx_gin.hip) against the
fixtures recorded from the REAL reference's model_zoo.AOANet (tests/golden/make_golden_aoanet.py), with the tolerances
of tests/zoo_cases.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import pytest

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import zoo  # noqa: E402
from test_aoanet_host import AOANET_CASES, build_aoanet  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402


@pytest.mark.parametrize("case", AOANET_CASES)
def test_forward_logits_match_reference(case, tmp_path):
    g = Golden(case)
    check_forward(build_aoanet(zoo, g, tmp_path, gpu=0), g, "0")


@pytest.mark.parametrize("case", AOANET_CASES)
def test_training_trajectory_matches_reference(case, tmp_path):
    g = Golden(case)
    check_trajectory(build_aoanet(zoo, g, tmp_path, gpu=0), g)


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order, no atomics -> same bits; the capture
    really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("aoanet_adam")
    check_graph_replay(lambda hip_graph: build_aoanet(zoo, g, tmp_path, gpu=0, hip_graph=hip_graph), g)
