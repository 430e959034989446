"""Drop-in check of FFMv2 and ONNv2 against the reference's OWN model classes (build container only: skipped where no
reference checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the
reference's unmodified FFMv2 / ONNv2 are constructed from layers.FeatureEmbedding (one wide table), layers.MLP_Block /
layers.LogisticRegression and their own inline torch ops for the interaction (the fused node is zoo.FFMv2's /
zoo.ONNv2's; the reference writes this interaction in the model class, so there is no layer to re-bind and
patch.LAYER_NAMES does not change) and, with the kernels replaced by the CPU emulations of tests/_cpu_emul.py,
reproduce the fixtures the same classes produced on the stock torch layers."""
import pytest

import _cpu_emul
from conftest import Golden
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_ffm_host import FFM_CASES
from zoo_cases import OMIT, allow_cpu_optimizer, check_dropin


@pytest.mark.parametrize("case", FFM_CASES)
def test_reference_field_aware_models_run_on_the_native_layers(case, patched_reference, monkeypatch, tmp_path):  # noqa: F811
    _cpu_emul.install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import layers
    g = Golden(case)
    m = g.meta
    if m["model"] == "FFMv2":
        from model_zoo.FFM.src.FFMv2 import FFMv2 as cls
        own = dict(regularizer=m["regularizer"], embedding_regularizer=OMIT, net_regularizer=OMIT)
        own_layer = ("lr_layer", layers.LogisticRegression)
    else:
        from model_zoo.ONN.ONN_torch.src.ONNv2 import ONNv2 as cls
        own = dict(hidden_units=m["hidden_units"], hidden_activations=m["hidden_activations"], net_dropout=0,
                   batch_norm=False)
        own_layer = ("dnn", layers.MLP_Block)
    check_dropin(cls, g, tmp_path, [own_layer, ("embedding_layer", layers.FeatureEmbedding)], **own)
