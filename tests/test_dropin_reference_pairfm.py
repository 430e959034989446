"""Drop-in check of FwFM and FmFM against the reference's OWN model classes (build container only: skipped where no
reference checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the
reference's unmodified `model_zoo.FwFM` / `model_zoo.FmFM` are constructed from layers.FeatureEmbedding,
layers.InnerProductInteraction ("inner_product"), layers.LogisticRegression and their own nn.Linear / bare Parameter
(the module-by-module composition: the fused node is zoo.FwFM's / zoo.FmFM's) and — with the kernels replaced by the
CPU emulations of tests/_cpu_emul.py — reproduce the fixtures the same classes produced on the stock torch layers,
without a call of either fx_pairfm_* op and with no change to patch.LAYER_NAMES."""
import numpy as np
import pytest
import torch

from conftest import Golden, assert_weights_close
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_pairfm_host import CALLS, PAIRFM_CASES, _install, tb


@pytest.mark.parametrize("case", PAIRFM_CASES)
def test_reference_pairfm_models_run_on_the_native_layers(case, patched_reference, monkeypatch, tmp_path):  # noqa: F811
    _install(monkeypatch)
    from fuxictr_amd import layers
    from fuxictr_amd.features import FeatureMap
    import model_zoo
    g = Golden(case)
    m = g.meta
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": m["embedding_dim"]})
    kw = dict(model_id=m["name"], gpu=-1, embedding_dim=m["embedding_dim"], learning_rate=m["lr"],
              optimizer=m["optimizer"], loss="binary_crossentropy", task="binary_classification",
              metrics=["logloss", "AUC"], verbose=0, model_root=str(tmp_path), regularizer=m["regularizer"])
    if m["model"] == "FmFM":
        model = model_zoo.FmFM(fmap, field_interaction_type=m["field_interaction_type"], **kw)
        assert type(model.lr_layer) is layers.LogisticRegression
    else:
        model = model_zoo.FwFM(fmap, linear_type=m["linear_type"], **kw)
        assert type(model.inner_product_layer) is layers.InnerProductInteraction
    assert type(model.embedding_layer) is layers.FeatureEmbedding
    sd = {k: torch.from_numpy(v) for k, v in g.state0.items()}
    assert sorted(model.state_dict().keys()) == sorted(sd.keys())
    model.load_state_dict(sd, strict=True)
    model._max_gradient_norm = m["max_norm"]
    model.eval()
    with torch.no_grad():
        p = model.forward(tb(g.batches[-1]))["y_pred"]
    np.testing.assert_allclose(p.reshape(-1).numpy(), g.expect["pred0"], atol=2e-5)
    model.train()
    losses = [float(model.train_step(tb(g.batches[i])).item()) for i in range(m["steps"])]
    np.testing.assert_allclose(losses, g.expect["loss"], rtol=0, atol=1e-4)
    model.eval()
    out = model.state_dict()
    for k, ref in g.state1.items():
        if ref.dtype.kind in "ib":
            assert np.array_equal(out[k].numpy(), ref), k
        else:
            assert_weights_close(out[k].numpy(), ref, m["lr"], m["steps"], k)
    assert CALLS == {"pairfm_fwd": 0, "pairfm_bwd": 0}
