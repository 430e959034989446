"""MaskNet end to end on a real MI355X: zoo.MaskNet on the native layers (grouped LayerNorm, LayerNorm + ReLU and the
mask gradient on csrc/fx_layernorm.hip, the mask product in GEMM epilogues) against the fixtures recorded from the
REAL reference's model_zoo.MaskNet (tests/golden/make_golden_masknet.py), with the tolerances of
tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import synthetic, zoo  # noqa: E402
from test_masknet_host import MASKNET_CASES, build_masknet  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory, tb  # noqa: E402



def build_native(g, tmp_path, sparse_update="exact", hip_graph=False, fused=True):
    return build_masknet(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", MASKNET_CASES)
def test_forward_logits_match_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", MASKNET_CASES)
def test_training_trajectory_matches_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_trajectory(model, g)


@pytest.mark.parametrize("case", ["masknet_serial_adam", "masknet_parallel_adam"])
def test_hip_graph_replay_is_bit_identical_to_eager(case, tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits (no atomics in the
    LayerNorm's dgamma / dbeta); the capture really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden(case)
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)


def test_lazy_mode_runs_and_equals_exact_on_step_one(tmp_path):
    g = Golden("masknet_serial_adam")
    for mode in ("exact", "lazy"):
        model = build_native(g, tmp_path, mode)
        model.train()
        for i in range(g.meta["steps"]):
            loss = model.train_step(tb(g.batches[i]))
        assert np.isfinite(float(loss.item()))
        model.eval()
    # step 1 is identical in both modes (no row has pending steps yet)
    e1, l1 = build_native(g, tmp_path, "exact"), build_native(g, tmp_path, "lazy")
    a = float(e1.train_step(tb(g.batches[0])).item())
    b = float(l1.train_step(tb(g.batches[0])).item())
    assert a == b


@pytest.mark.parametrize("model_type", ["SerialMaskNet", "ParallelMaskNet"])
def test_criteo_sized_step_is_finite_and_repeatable(model_type, tmp_path):
    """39 fields, D = 16, B = 4096, blocks [256, 256] (ParallelMaskNet: 2 blocks of 256 and a 256-wide tower): one
    training step twice from the same seed: everything finite, the same bits."""
    cards = [max(2, int(c * 0.01)) for c in synthetic.CRITEO_CARDS]
    rng = np.random.default_rng(0)
    b = synthetic.criteo_batch(rng, 4096, cards=cards)
    b["label"] = (b["I1"] + b["I2"] > 1.0).astype(np.float32)
    batch = tb(b)
    results = []
    for _ in range(2):
        fmap, _ = synthetic.criteo_feature_map(cards=cards, embedding_dim=16)
        torch.manual_seed(0)
        model = zoo.MaskNet(fmap, model_id="masknet_criteo", gpu=0, embedding_dim=16, dnn_hidden_units=[256, 256],
                            model_type=model_type, parallel_num_blocks=2, parallel_block_dim=256,
                            optimizer="adam", loss="binary_crossentropy", learning_rate=1e-3,
                            task="binary_classification", metrics=["logloss", "AUC"], verbose=0,
                            model_root=str(tmp_path), sparse_update="exact")
        model.train()
        loss = float(model.train_step(batch).item())
        model.eval()
        sd = {k: v.clone() for k, v in model.state_dict().items() if "embedding" not in k}
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
        results.append((loss, sd))
        model.optimizer.check_errors()
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k
