"""FFMv2 and ONNv2 end to end on a real MI355X: zoo.FFMv2 / zoo.ONNv2 on layers.field_aware_interaction
(csrc/fx_ffm.hip) against the fixtures recorded from the REAL reference's classes (tests/golden/make_golden_ffm.py),
with the tolerances of tests/zoo_cases.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import pytest

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import zoo  # noqa: E402
from test_ffm_host import FFM_CASES, build_ffm  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402


@pytest.mark.parametrize("case", FFM_CASES)
def test_forward_logits_match_reference(case, tmp_path):
    g = Golden(case)
    check_forward(build_ffm(zoo, g, tmp_path, gpu=0), g, "0")


@pytest.mark.parametrize("case", FFM_CASES)
def test_training_trajectory_matches_reference(case, tmp_path):
    g = Golden(case)
    check_trajectory(build_ffm(zoo, g, tmp_path, gpu=0), g)


@pytest.mark.parametrize("case", ["ffmv2_adam", "onnv2_adam"])
def test_hip_graph_replay_is_bit_identical_to_eager(case, tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order, no atomics -> same bits; the capture
    really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden(case)
    check_graph_replay(lambda hip_graph: build_ffm(zoo, g, tmp_path, gpu=0, hip_graph=hip_graph), g)
