"""FiBiNET end to end on a real MI355X: zoo.FiBiNET on the native layers (squeeze-excitation and bilinear
interaction on csrc/fx_bilinear.hip) against the fixtures recorded from the REAL reference's model_zoo.FiBiNET
(tests/golden/make_golden_fibinet.py), with the tolerances of tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden, assert_weights_close  # noqa: E402
from fuxictr_amd import synthetic, zoo  # noqa: E402
from test_fibinet_host import FIBINET_CASES, build_fibinet, tb  # noqa: E402

LOGIT_TOL = 1e-4


def build_native(g, tmp_path, sparse_update="exact", hip_graph=False, fused=True):
    return build_fibinet(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("case", FIBINET_CASES)
def test_forward_logits_match_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    model.eval()
    with torch.no_grad():
        p = model.forward(tb(g.batches[-1]))["y_pred"]
    err = np.abs(p._fx_logit.reshape(-1).cpu().numpy() - g.expect["logit0"]).max()
    print(case, "max |logit - reference| %.3e" % err)
    assert err <= LOGIT_TOL, err
    np.testing.assert_allclose(p.reshape(-1).cpu().numpy(), g.expect["pred0"], atol=2e-5)


@pytest.mark.parametrize("case", FIBINET_CASES)
def test_training_trajectory_matches_reference(case, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path)
    model.train()
    losses = [float(model.train_step(tb(g.batches[i])).item()) for i in range(g.meta["steps"])]
    print(case, "max |loss - reference| %.3e" % np.abs(np.asarray(losses) - g.expect["loss"]).max())
    np.testing.assert_allclose(losses, g.expect["loss"], rtol=0, atol=1e-4)
    model.eval()                                   # flushes pending zero-gradient steps
    with torch.no_grad():
        p = model.forward(tb(g.batches[-1]))["y_pred"]
    assert np.abs(p._fx_logit.reshape(-1).cpu().numpy() - g.expect["logit1"]).max() <= LOGIT_TOL
    np.testing.assert_allclose(p.reshape(-1).cpu().numpy(), g.expect["pred1"], atol=2e-5)
    sd = model.state_dict()
    for k, ref in g.state1.items():
        if ref.dtype.kind == "i":
            assert np.array_equal(sd[k].cpu().numpy(), ref), k
        else:
            assert_weights_close(sd[k].cpu().numpy(), ref, g.meta["lr"], g.meta["steps"], k)
    model.optimizer.check_errors()


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits; the capture really
    happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("fibinet_adam")
    eager = build_native(g, tmp_path, hip_graph=False)
    graph = build_native(g, tmp_path, hip_graph=True)
    eager.train()
    graph.train()
    n = len(g.batches)
    for i in range(9):                       # eager warm-ups + probe + replays
        b = tb(g.batches[i % n])
        le = float(eager.train_step(b).item())
        lg = float(graph.train_step(b).item())
        assert le == lg, (i, le, lg)
    assert graph._graph_state is not None
    eager.eval()
    graph.eval()
    se, sg = eager.state_dict(), graph.state_dict()
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    graph.optimizer.check_errors()


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
