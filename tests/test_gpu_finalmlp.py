"""FinalMLP and DualMLP end to end on a real MI355X: zoo.FinalMLP / zoo.DualMLP on the native layers (both feature
gates and the aggregation head on csrc/fx_finalmlp.hip, the per-head products on the GEMM dispatcher) against the
fixtures recorded from the REAL reference's model_zoo.FinalMLP / DualMLP (tests/golden/make_golden_finalmlp.py),
with the tolerances of tests/test_gpu_masknet.py / test_gpu_models.py:
  forward logits |d| <= 1e-4, pred atol 2e-5, loss trajectory |d| <= 1e-4 per step, trained weights
  conftest.assert_weights_close.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import synthetic, zoo  # noqa: E402
from test_finalmlp_host import FINALMLP_CASES, build_finalmlp  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory, tb  # noqa: E402



def build_native(g, tmp_path, sparse_update="exact", hip_graph=False, fused=True):
    return build_finalmlp(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", FINALMLP_CASES)
def test_forward_logits_match_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", FINALMLP_CASES)
def test_training_trajectory_matches_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_trajectory(model, g)


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits (no atomics in the
    broadcast gate's dZ or in dw_x / dw_y / db); the capture really happened (`_graph_state`), it did not fall back
    to eager.  One gate with context features and one without."""
    g = Golden("finalmlp_mixed")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)


def test_criteo_shaped_step_is_finite_and_repeatable(tmp_path):
    """26 sparse + 13 dense fields, D = 16, B = 4096, towers [1024, 512] / [1024, 512, 256], gate towers
    [1024, 512] without context features, two heads (the reference's FinalMLP_default): one training step twice from
    the same seed: everything finite, the same bits."""
    cards = [max(2, int(c * 0.01)) for c in synthetic.CRITEO_CARDS]
    rng = np.random.default_rng(0)
    b = synthetic.criteo_batch(rng, 4096, cards=cards)
    b["label"] = (b["I1"] + b["I2"] > 1.0).astype(np.float32)
    batch = tb(b)
    results = []
    for _ in range(2):
        fmap, _ = synthetic.criteo_feature_map(cards=cards, embedding_dim=16)
        torch.manual_seed(0)
        model = zoo.FinalMLP(fmap, model_id="finalmlp_criteo", gpu=0, embedding_dim=16,
                             mlp1_hidden_units=[1024, 512], mlp2_hidden_units=[1024, 512, 256],
                             fs_hidden_units=[1024, 512], fs1_context=[], fs2_context=[], num_heads=2,
                             optimizer="adam", loss="binary_crossentropy", learning_rate=1e-3,
                             task="binary_classification", metrics=["logloss", "AUC"], verbose=0,
                             model_root=str(tmp_path), sparse_update="exact")
        assert model._fused
        model.train()
        loss = float(model.train_step(batch).item())
        model.eval()
        sd = {k: v.clone() for k, v in model.state_dict().items() if "embedding" not in k}
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
        # the step reached the gates: the bias of each gate tower's last Linear moved off its zero (the towers' hidden
        # ReLUs sit at exactly 0 on a fresh model, so nothing reaches the layers below them yet)
        assert bool(sd["fs_module.fs1_gate.mlp.4.bias"].abs().max() > 0)
        assert bool(sd["fs_module.fs2_gate.mlp.4.bias"].abs().max() > 0)
        results.append((loss, sd))
        model.optimizer.check_errors()
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k
