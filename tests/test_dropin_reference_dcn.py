"""Drop-in check of DCN against the reference's OWN model class (build container only: skipped where no reference
checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the
reference's unmodified `model_zoo.DCN` is constructed from layers.CrossNet (the fused node: one cross_net_fwd and one
cross_net_bwd per step) and layers.MLP_Block and — with the kernels replaced by the CPU emulations of
tests/_cpu_emul.py and tests/test_dcn_host.py — reproduces the fixtures the same class produced on the stock torch
layers."""
import numpy as np
import pytest
import torch

from conftest import Golden, assert_weights_close
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_dcn_host import CALLS, DCN_CASES, _install, _reset_calls, tb


@pytest.mark.parametrize("case", DCN_CASES)
def test_reference_dcn_runs_on_the_native_layers(case, patched_reference, monkeypatch, tmp_path):  # noqa: F811
    _install(monkeypatch)
    from fuxictr_amd import layers
    from fuxictr_amd.features import FeatureMap
    from model_zoo import DCN
    assert DCN.__module__.startswith("model_zoo")
    g = Golden(case)
    m = g.meta
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": m["embedding_dim"]})
    model = DCN(fmap, model_id=m["name"], gpu=-1, embedding_dim=m["embedding_dim"], learning_rate=m["lr"],
                optimizer=m["optimizer"], loss="binary_crossentropy", task="binary_classification",
                metrics=["logloss", "AUC"], verbose=0, model_root=str(tmp_path),
                embedding_regularizer=m.get("emb_reg", 0), net_regularizer=m.get("net_reg", 0),
                dnn_hidden_units=m["dnn"], dnn_activations="relu", num_cross_layers=m["n_cross"])
    assert type(model.crossnet) is layers.CrossNet
    assert (model.dnn is None) == (not m["dnn"])
    assert model.dnn is None or type(model.dnn) is layers.MLP_Block
    sd = {k: torch.from_numpy(v) for k, v in g.state0.items()}
    assert sorted(model.state_dict().keys()) == sorted(sd.keys())
    model.load_state_dict(sd, strict=True)
    model._max_gradient_norm = m["max_norm"]
    model.eval()
    _reset_calls()
    with torch.no_grad():
        p = model.forward(tb(g.batches[-1]))["y_pred"]
    np.testing.assert_allclose(p.reshape(-1).numpy(), g.expect["pred0"], atol=2e-5)
    assert CALLS == {"cross_net_fwd": 1, "cross_net_bwd": 0}
    model.train()
    _reset_calls()
    losses = [float(model.train_step(tb(g.batches[i])).item()) for i in range(m["steps"])]
    np.testing.assert_allclose(losses, g.expect["loss"], rtol=0, atol=1e-4)
    assert CALLS == {"cross_net_fwd": m["steps"], "cross_net_bwd": m["steps"]}
    model.eval()
    with torch.no_grad():
        p = model.forward(tb(g.batches[-1]))["y_pred"]
    np.testing.assert_allclose(p.reshape(-1).numpy(), g.expect["pred1"], atol=2e-5)
    out = model.state_dict()
    for k, ref in g.state1.items():
        if ref.dtype.kind == "i":
            assert np.array_equal(out[k].numpy(), ref), k
        else:
            assert_weights_close(out[k].numpy(), ref, m["lr"], m["steps"], k)
