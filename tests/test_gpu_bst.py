"""BST end to end on a real MI355X: zoo.BST on the native layers (each transformer block on csrc/fx_bst.hip) against
the fixtures recorded from the REAL reference's model_zoo.BST (tests/golden/make_golden_bst.py), with the tolerances
of tests/test_gpu_models.py:
  forward logits |d| <= 1e-4, loss trajectory |d| <= 1e-4 per step, trained weights conftest.assert_weights_close.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden, assert_weights_close  # noqa: E402
from fuxictr_amd import zoo  # noqa: E402
from test_bst_host import BST_CASES, build_bst, tb  # noqa: E402

LOGIT_TOL = 1e-4


def build_native(g, tmp_path, sparse_update="exact", hip_graph=False):
    return build_bst(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph)


@pytest.mark.parametrize("case", BST_CASES)
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


@pytest.mark.parametrize("case", BST_CASES)
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
    sd = model.state_dict()
    for k, ref in g.state1.items():
        assert_weights_close(sd[k].cpu().numpy(), ref, g.meta["lr"], g.meta["steps"], k)
    model.optimizer.check_errors()


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits; the capture really
    happened (`_graph_state`), it did not fall back to eager.  (The captured step's static batch lists its features
    by packed matrix, not in the batch's order: the DNN's input is assembled in the feature map's order.)"""
    g = Golden("bst_pair_adam")
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
