"""Drop-in check of FwFM and FmFM against the reference's OWN model classes (build container only: skipped where no
reference checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the
reference's unmodified `model_zoo.FwFM` / `model_zoo.FmFM` are constructed from layers.FeatureEmbedding,
layers.InnerProductInteraction ("inner_product"), layers.LogisticRegression and their own nn.Linear / bare Parameter
(the module-by-module composition: the fused node is zoo.FwFM's / zoo.FmFM's) and — with the kernels replaced by the
CPU emulations of tests/_cpu_emul.py — reproduce the fixtures the same classes produced on the stock torch layers,
without a call of either fx_pairfm_* op and with no change to patch.LAYER_NAMES."""
import pytest

from conftest import Golden
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_pairfm_host import CALLS, PAIRFM_CASES, _install
from zoo_cases import OMIT, check_dropin


@pytest.mark.parametrize("case", PAIRFM_CASES)
def test_reference_pairfm_models_run_on_the_native_layers(case, patched_reference, monkeypatch, tmp_path):  # noqa: F811
    _install(monkeypatch)
    from fuxictr_amd import layers
    import model_zoo
    g = Golden(case)
    m = g.meta
    if m["model"] == "FmFM":
        own = {"field_interaction_type": m["field_interaction_type"]}
        own_layer = ("lr_layer", layers.LogisticRegression)
    else:
        own = {"linear_type": m["linear_type"]}
        own_layer = ("inner_product_layer", layers.InnerProductInteraction)
    none = {"pairfm_fwd": 0, "pairfm_bwd": 0}                        # module by module: the fused node is the zoo's
    check_dropin(getattr(model_zoo, m["model"]), g, tmp_path, [own_layer, ("embedding_layer", layers.FeatureEmbedding)],
                 calls=CALLS, forward_calls=none, final_calls=none, regularizer=m["regularizer"],
                 embedding_regularizer=OMIT, net_regularizer=OMIT, **own)
