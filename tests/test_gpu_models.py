"""End-to-end parity on a real MI355X: the native DeepFM / DCNv2 (fuxictr_amd.zoo on the native
layers, every op through libfxctr.so) against golden vectors recorded from the REAL reference
(tests/golden/, made by make_golden.py) and against the oracle on the same inputs.

Stated tolerances (BASELINE.json north_star: logits within 1e-4 fp32 of the reference forward):
  forward logits        |d| <= 1e-4   (observed ~1e-6: exact-fp32 MFMA, same formulas)
  loss trajectory       |d| <= 1e-4 per step over the recorded steps (dense-Adam semantics, `exact`)
  weights after k steps |d| <= 2e-5 (see conftest.assert_weights_close for Adam's eps-conditioning)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden, _din_fields  # noqa: E402
from fuxictr_amd import synthetic, zoo  # noqa: E402
from oracle import ctr_oracle as O  # noqa: E402
from zoo_cases import build_from_golden, check_forward, check_graph_replay, check_trajectory, tb  # noqa: E402


def build_native(g, tmp_path, sparse_update="exact", optimizer=None, hip_graph=False):
    m = g.meta
    if m["model"] == "DeepFM":
        cls, own = zoo.DeepFM, dict(hidden_units=m["hidden"], batch_norm=m.get("batch_norm", False))
    elif m["model"] == "xDeepFM":
        cls, own = zoo.xDeepFM, dict(dnn_hidden_units=m["hidden"], cin_hidden_units=m["cin"])
    elif m["model"] == "DLRM":
        cls, own = zoo.DLRM, dict(top_mlp_units=m["hidden"], bottom_mlp_units=m["bottom"],
                                  interaction_op=m.get("interaction_op", "dot"))
    elif m["model"] == "DIN":
        cls, own = zoo.DIN, dict(dnn_hidden_units=m["hidden"], dnn_activations="relu",
                                 attention_hidden_units=m["att_hidden"], attention_hidden_activations="Dice",
                                 din_target_field=_din_fields(m, "din_target", "adgroup_id"),
                                 din_sequence_field=_din_fields(m, "din_sequence", "click_sequence"),
                                 din_use_softmax=m.get("din_softmax", False))
    else:
        cls, own = zoo.DCNv2, dict(model_structure=m.get("structure", "parallel"), num_cross_layers=m["n_cross"],
                                   parallel_dnn_hidden_units=m["hidden"], stacked_dnn_hidden_units=m.get("stacked", []))
    return build_from_golden(cls, g, tmp_path, gpu=0, optimizer=optimizer or m["optimizer"],
                             sparse_update=sparse_update, hip_graph=hip_graph, **own)


def test_forward_logits_match_reference(golden, tmp_path):
    model = build_native(golden, tmp_path)
    err, pred = check_forward(model, golden, "0")
    assert err <= 2e-5, "fp32 MFMA path is expected to be far inside the 1e-4 budget: %g" % err
    np.testing.assert_allclose(pred, golden.expect["pred0"], atol=2e-6)


def test_training_trajectory_matches_reference(golden, tmp_path):
    """`exact` sparse update == the reference's dense clip + Adam/SGD over every parameter."""
    model = build_native(golden, tmp_path)
    check_trajectory(model, golden)


def test_auc_matches_oracle_to_4_decimals(tmp_path):
    """Train native and oracle from the same weights on the same batches; AUC/logloss of a held
    out set agree to 4 decimals (sklearn on float64 on both sides, like metrics.py:49-51)."""
    from sklearn.metrics import log_loss, roc_auc_score
    g = Golden("deepfm_adam")
    m = g.meta
    model = build_native(g, tmp_path)
    tr = O.OracleTrainer(g.cfg(), g.state0, g.features, lr=m["lr"], max_norm=m["max_norm"])
    rng = np.random.default_rng(123)
    from make_golden import make_batches
    train = make_batches(rng, g.spec, 256, 12)
    # teacher labels so that AUC is far from 0.5
    w = rng.normal(size=len(g.features))
    def relabel(b):
        s = sum(w[i] * (np.asarray(b[f], dtype=np.float64) % 7 - 3) / 3.0
                for i, f in enumerate(g.features))
        b["label"] = (rng.random(len(s)) < 1 / (1 + np.exp(-s))).astype(np.float32)
        return b
    train = [relabel(b) for b in train]
    test = [relabel(b) for b in make_batches(rng, g.spec, 2048, 2)]
    model.train()
    for b in train:
        t = tb(b)
        model.train_step(t)
        tr.train_step(t, t["label"])
    model.eval()
    y = np.concatenate([b["label"] for b in test]).astype(np.float64)
    with torch.no_grad():
        pn = np.concatenate([model.forward(tb(b))["y_pred"].reshape(-1).cpu().numpy() for b in test])
    po = np.concatenate([tr.predict(tb(b)).reshape(-1).numpy() for b in test])
    auc_n, auc_o = roc_auc_score(y, pn.astype(np.float64)), roc_auc_score(y, po.astype(np.float64))
    ll_n, ll_o = log_loss(y, pn.astype(np.float64)), log_loss(y, po.astype(np.float64))
    assert abs(auc_n - auc_o) < 5e-5, (auc_n, auc_o)
    assert abs(ll_n - ll_o) < 5e-5, (ll_n, ll_o)
    assert auc_n > 0.55
    assert np.abs(pn - po).max() <= 1e-4


def test_lazy_mode_runs_and_differs_only_on_idle_rows(tmp_path):
    g = Golden("deepfm_adam")
    exact = build_native(g, tmp_path, "exact")
    lazy = build_native(g, tmp_path, "lazy")
    for model in (exact, lazy):
        model.train()
        for i in range(g.meta["steps"]):
            loss = model.train_step(tb(g.batches[i]))
        assert np.isfinite(float(loss.item()))
        model.eval()
    k = "mlp.mlp.0.weight"
    d_dense = (exact.state_dict()[k] - lazy.state_dict()[k]).abs().max().item()
    assert d_dense < 5e-2           # same model family, small documented deviation
    # step 1 is identical in both modes (no row has pending steps yet)
    e1, l1 = build_native(g, tmp_path, "exact"), build_native(g, tmp_path, "lazy")
    a = float(e1.train_step(tb(g.batches[0])).item())
    b = float(l1.train_step(tb(g.batches[0])).item())
    assert a == b


@pytest.mark.parametrize("case", ["deepfm_adam", "dcnv2_adam", "deepfm_sgd"])
def test_hip_graph_replay_is_bit_identical_to_eager(case, tmp_path):
    """`hip_graph: true` replays the captured step; same kernels, same order -> same bits."""
    g = Golden(case)
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)


def test_bad_id_raises_like_the_reference(tmp_path):
    g = Golden("deepfm_d10")
    model = build_native(g, tmp_path)
    b = tb(g.batches[0])
    b["C3"] = b["C3"].clone()
    b["C3"][0] = 10 ** 6
    model.train()
    model.train_step(b)
    with pytest.raises(IndexError):
        model.optimizer.check_errors()


def test_fit_evaluate_checkpoint_roundtrip(tmp_path):
    """BaseModel.fit / evaluate / save_weights / load_weights on the native path (rank_model.py
    :236-270, :350-381, :417-433), driven like run_expid.py does."""
    g = Golden("dcnv2_adam")
    model = build_native(g, tmp_path)

    class Gen(list):
        pass
    train = Gen(tb(b) for b in g.batches[:-1])
    valid = Gen([tb(g.batches[-1])])
    model.fit(train, epochs=2, validation_data=valid, max_gradient_norm=10.0)
    logs = model.evaluate(valid)
    assert set(logs) == {"logloss", "AUC"} and 0 < logs["logloss"] < 1
    pred = model.predict(valid)
    assert pred.shape == (len(g.batches[-1]["label"]),) and pred.dtype == np.float64
    other = build_native(g, tmp_path)
    other.load_weights(model.checkpoint)
    np.testing.assert_array_equal(other.predict(valid), pred)
    assert model.count_parameters() == sum(v.size for v in g.state0.values())


@pytest.mark.parametrize("dist", ["powerlaw", "uniform"])
def test_full_criteo_scale_properties(tmp_path, dist):
    """BASELINE config c2 at full size (33.76 M rows, D=16, B=4096, MLP 4x1024): the oracle is too
    slow here, so check size-independent properties: gather == table rows bit-exact, only rows of
    the batch move in a step (checksum of all other rows unchanged), determinism across runs."""
    fmap, _ = synthetic.criteo_feature_map(embedding_dim=16)
    def make():
        torch.manual_seed(0)
        return zoo.DeepFM(fmap, model_id="c2", gpu=0, embedding_dim=16, hidden_units=[1024] * 4,
                          optimizer="adam", loss="binary_crossentropy", learning_rate=1e-3,
                          task="binary_classification", metrics=["logloss", "AUC"], verbose=0,
                          model_root=str(tmp_path), sparse_update="exact")
    model = make()
    rng = np.random.default_rng(0)
    batches = [tb(synthetic.criteo_batch(rng, 4096, dist=dist)) for _ in range(3)]
    layer = model.embedding_layer.embedding_layer
    grp = layer.table_groups()[0]
    assert grp.total_rows == 33762577 + 26
    # (1) gather is bit-exact against direct indexing of the packed table
    model.eval()
    with torch.no_grad():
        X = model.get_inputs(batches[0])
        rec = model.embedding_layer(X)
    assert rec.shape == (4096, 39, 16)
    plan = list(grp.plans.values())[0]
    for f in ["C1", "C3", "C26"]:
        s, _ = plan.slot[f]
        base = grp.table_of(f)[0]
        rows = batches[0][f].to("cuda:0") + base
        assert torch.equal(rec[:, s], grp.table[rows])
    j, _ = plan.slot["I5"]
    assert torch.equal(rec[:, j], batches[0]["I5"].to("cuda:0").view(-1, 1) * grp.num_w[4])
    # (2) a step moves only rows of the batch
    table_before = grp.table.clone()
    model.train()
    losses = [float(model.train_step(b).item()) for b in batches]
    assert all(np.isfinite(losses))
    touched = torch.zeros(grp.total_rows, dtype=torch.bool, device="cuda:0")
    for b in batches:
        for f, (base, V, _) in grp.tables.items():
            touched[b[f].to("cuda:0") + base] = True
    changed = (grp.table != table_before).any(dim=1)
    assert not bool((changed & ~touched).any())
    assert int(changed.sum()) > 0.5 * int(touched.sum())
    model.optimizer.check_errors()
    # (3) determinism: a second model from the same seed reproduces the losses bit for bit
    del table_before
    model2 = make()
    model2.train()
    losses2 = [float(model2.train_step(b).item()) for b in batches]
    assert losses == losses2
    assert torch.equal(model2.embedding_layer.embedding_layer.table_groups()[0].table, grp.table)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["deepfm_adam", "dcnv2_adam"])
def test_checkpoint_resume_continues_the_uninterrupted_trajectory(case, tmp_path):
    """save_checkpoint / load_checkpoint (weights + Adam moments + row stamps + step): training
    3 steps, saving, loading into a NEW model and training on == training straight through.
    (Not bit-identical in exact mode: saving flushes the pending zero-gradient replays, so a row's
    replay is split in two and the bias-correction powers are re-derived at the split: ~1e-7.)"""
    g = Golden(case)
    n = g.meta["steps"]
    a = build_native(g, tmp_path)
    a.train()
    for i in range(n):
        a.train_step(tb(g.batches[i]))
    b = build_native(g, tmp_path)
    b.train()
    for i in range(3):
        b.train_step(tb(g.batches[i]))
    path = str(tmp_path / "ck" / "resume.model")
    b.save_checkpoint(path)
    c = build_native(g, tmp_path)
    c.load_checkpoint(path)
    c.train()
    for i in range(3, n):
        c.train_step(tb(g.batches[i]))
    a.eval()
    c.eval()
    sa, sc = a.state_dict(), c.state_dict()
    for k in sa:
        assert (sa[k] - sc[k]).abs().max().item() <= 1e-6, k
