"""AutoInt end to end on a real MI355X: zoo.AutoInt on the native layers (the interaction layers on
csrc/fx_mhsa.hip) against the fixtures recorded from the REAL reference's model_zoo.AutoInt
(tests/golden/make_golden_autoint.py), with the tolerances of tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import synthetic, zoo  # noqa: E402
from test_autoint_host import AUTOINT_CASES, build_autoint  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory, tb  # noqa: E402



def build_native(g, tmp_path, sparse_update="exact", hip_graph=False):
    return build_autoint(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph)


@pytest.mark.parametrize("case", AUTOINT_CASES)
def test_forward_logits_match_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", AUTOINT_CASES)
def test_training_trajectory_matches_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_trajectory(model, g)


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits; the capture really
    happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("autoint_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)


def test_lazy_mode_runs_and_differs_only_on_idle_rows(tmp_path):
    g = Golden("autoint_adam")
    exact = build_native(g, tmp_path, "exact")
    lazy = build_native(g, tmp_path, "lazy")
    for model in (exact, lazy):
        model.train()
        for i in range(g.meta["steps"]):
            loss = model.train_step(tb(g.batches[i]))
        assert np.isfinite(float(loss.item()))
        model.eval()
    k = "self_attention.0.W_q.weight"
    assert (exact.state_dict()[k] - lazy.state_dict()[k]).abs().max().item() < 5e-2
    # step 1 is identical in both modes (no row has pending steps yet)
    e1, l1 = build_native(g, tmp_path, "exact"), build_native(g, tmp_path, "lazy")
    a = float(e1.train_step(tb(g.batches[0])).item())
    b = float(l1.train_step(tb(g.batches[0])).item())
    assert a == b


def test_criteo_sized_run_trains(tmp_path):
    """39 fields (the synthetic Criteo schema at 1 % of its vocabulary), B = 4096, D = A = 16, 2 heads, 3 layers,
    deep tower 4 x 1024: 20 steps, the loss finite and falling, no error flag raised on the device."""
    cards = [max(2, int(c * 0.01)) for c in synthetic.CRITEO_CARDS]
    fmap, _ = synthetic.criteo_feature_map(cards=cards, embedding_dim=16)
    torch.manual_seed(0)
    model = zoo.AutoInt(fmap, model_id="autoint_criteo", gpu=0, embedding_dim=16, attention_dim=16,
                        num_heads=2, attention_layers=3, dnn_hidden_units=[1024] * 4, optimizer="adam",
                        loss="binary_crossentropy", learning_rate=1e-3, task="binary_classification",
                        metrics=["logloss", "AUC"], verbose=0, model_root=str(tmp_path),
                        sparse_update="exact")
    rng = np.random.default_rng(0)
    batches = []
    for _ in range(4):
        b = synthetic.criteo_batch(rng, 4096, cards=cards)
        b["label"] = (b["I1"] + b["I2"] > 1.0).astype(np.float32)       # something to learn
        batches.append(tb(b))
    model.train()
    losses = [float(model.train_step(batches[i % 4]).item()) for i in range(20)]
    print("criteo-sized AutoInt losses", ["%.4f" % v for v in losses])
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    model.optimizer.check_errors()
