"""Drop-in check of AFM against the reference's OWN model class (build container only: skipped where no reference
checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the
reference's unmodified `model_zoo.AFM` is constructed from layers.InnerProductInteraction ("elementwise_product"),
layers.LogisticRegression and its own attention nn.Sequential (the module-by-module composition: the fused node is
zoo.AFM's) and — with the kernels replaced by the CPU emulations of tests/_cpu_emul.py — reproduces the fixtures the
same class produced on the stock torch layers, without a call of either fx_afm_attn_* op."""
import numpy as np
import pytest
import torch

from conftest import Golden, assert_weights_close
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_afm_host import AFM_CASES, CALLS, _install, tb


@pytest.mark.parametrize("case", AFM_CASES)
def test_reference_afm_runs_on_the_native_layers(case, patched_reference, monkeypatch, tmp_path):  # noqa: F811
    _install(monkeypatch)
    from fuxictr_amd import layers
    from fuxictr_amd.features import FeatureMap
    from model_zoo import AFM
    g = Golden(case)
    m = g.meta
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": m["embedding_dim"]})
    model = AFM(fmap, model_id=m["name"], gpu=-1, embedding_dim=m["embedding_dim"], learning_rate=m["lr"],
                optimizer=m["optimizer"], loss="binary_crossentropy", task="binary_classification",
                metrics=["logloss", "AUC"], verbose=0, model_root=str(tmp_path),
                embedding_regularizer=m.get("emb_reg", 0), net_regularizer=m.get("net_reg", 0),
                attention_dim=m["attention_dim"], attention_dropout=[0, 0], use_attention=m["use_attention"])
    assert type(model.product_layer) is layers.InnerProductInteraction
    assert type(model.lr_layer) is layers.LogisticRegression
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
        if ref.dtype.kind == "i":
            assert np.array_equal(out[k].numpy(), ref), k
        else:
            assert_weights_close(out[k].numpy(), ref, m["lr"], m["steps"], k)
    assert CALLS == {"afm_attn_fwd": 0, "afm_attn_bwd": 0}
