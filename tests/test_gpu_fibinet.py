"""FiBiNET end to end on a real MI355X: zoo.FiBiNET on the native layers (squeeze-excitation and bilinear
interaction on csrc/fx_bilinear.hip) against the fixtures recorded from the REAL reference's model_zoo.FiBiNET
(tests/golden/make_golden_fibinet.py), with the tolerances of tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import synthetic, zoo  # noqa: E402
from test_fibinet_host import FIBINET_CASES, build_fibinet  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory, tb  # noqa: E402



def build_native(g, tmp_path, sparse_update="exact", hip_graph=False, fused=True):
    return build_fibinet(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("case", FIBINET_CASES)
def test_forward_logits_match_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", FIBINET_CASES)
def test_training_trajectory_matches_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    check_trajectory(model, g)


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits; the capture really
    happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("fibinet_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)


def test_lazy_mode_runs_and_differs_only_on_idle_rows(tmp_path):
    g = Golden("fibinet_adam")
    exact = build_native(g, tmp_path, "exact")
    lazy = build_native(g, tmp_path, "lazy")
    for model in (exact, lazy):
        model.train()
        for i in range(g.meta["steps"]):
            loss = model.train_step(tb(g.batches[i]))
        assert np.isfinite(float(loss.item()))
        model.eval()
    k = "bilinear_interaction1.bilinear_W"
    assert (exact.state_dict()[k] - lazy.state_dict()[k]).abs().max().item() < 5e-2
    # step 1 is identical in both modes (no row has pending steps yet)
    e1, l1 = build_native(g, tmp_path, "exact"), build_native(g, tmp_path, "lazy")
    a = float(e1.train_step(tb(g.batches[0])).item())
    b = float(l1.train_step(tb(g.batches[0])).item())
    assert a == b


@pytest.mark.parametrize("case", FIBINET_CASES)
def test_fused_and_unfused_routes_agree_to_the_bit(case, tmp_path):
    """The fused route multiplies by the gates inside the bilinear kernel (v = a * x as it is loaded), the unfused
    one reads V = X * A written by the excitation kernel: the same fp32 product, then the same instruction
    sequence; the backward sums dX in another order (branch 1, + branch 2, + excitation against autograd's
    sum of three tensors), so the losses of step 1 agree to the bit and the later ones to rounding."""
    g = Golden(case)
    a, b = build_native(g, tmp_path, fused=True), build_native(g, tmp_path, fused=False)
    assert a._fused and not b._fused
    a.eval(), b.eval()
    with torch.no_grad():
        pa = a.forward(tb(g.batches[-1]))["y_pred"]
        pb = b.forward(tb(g.batches[-1]))["y_pred"]
    assert torch.equal(pa._fx_logit, pb._fx_logit)
    a.train(), b.train()
    for i in range(g.meta["steps"]):
        la, lb = float(a.train_step(tb(g.batches[i])).item()), float(b.train_step(tb(g.batches[i])).item())
        print(case, i, la, lb)
        assert (la == lb) if i == 0 else abs(la - lb) <= 1e-5, (i, la, lb)


def test_criteo_sized_forward_backward_is_finite_and_repeatable(tmp_path):
    """39 fields, D = 16, B = 4096, field_interaction, tower 2 x 256: one forward + backward twice from the same
    weights: everything finite, the same bits."""
    cards = [max(2, int(c * 0.01)) for c in synthetic.CRITEO_CARDS]
    rng = np.random.default_rng(0)
    b = synthetic.criteo_batch(rng, 4096, cards=cards)
    b["label"] = (b["I1"] + b["I2"] > 1.0).astype(np.float32)
    batch = tb(b)
    results = []
    for _ in range(2):
        fmap, _ = synthetic.criteo_feature_map(cards=cards, embedding_dim=16)
        torch.manual_seed(0)
        model = zoo.FiBiNET(fmap, model_id="fibinet_criteo", gpu=0, embedding_dim=16, hidden_units=[256, 256],
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
