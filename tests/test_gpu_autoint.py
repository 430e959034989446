"""AutoInt end to end on a real MI355X: zoo.AutoInt on the native layers (the interaction layers on
csrc/fx_mhsa.hip) against the fixtures recorded from the REAL reference's model_zoo.AutoInt
(tests/golden/make_golden_autoint.py), with the tolerances of tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden, assert_weights_close  # noqa: E402
from fuxictr_amd import synthetic, zoo  # noqa: E402
from test_autoint_host import AUTOINT_CASES, build_autoint, tb  # noqa: E402

LOGIT_TOL = 1e-4


def build_native(g, tmp_path, sparse_update="exact", hip_graph=False):
    return build_autoint(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph)


@pytest.mark.parametrize("case", AUTOINT_CASES)
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


@pytest.mark.parametrize("case", AUTOINT_CASES)
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
        assert_weights_close(sd[k].cpu().numpy(), ref, g.meta["lr"], g.meta["steps"], k)
    model.optimizer.check_errors()


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits; the capture really
    happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("autoint_adam")
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
