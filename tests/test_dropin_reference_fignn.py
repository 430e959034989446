"""Drop-in check of FiGNN against the reference's OWN model class (build container only: skipped where no reference
checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the reference's
unmodified `model_zoo.FiGNN` is constructed from layers.FeatureEmbedding; its FiGNN_Layer, GraphLayer and
AttentionalPrediction are defined in the model file itself, so they keep torch's composition (the fused propagation is
zoo.FiGNN's) and - with the kernels replaced by the CPU emulations of tests/_cpu_emul.py - reproduce the fixtures the
same class produced on the stock torch layers."""
import pytest

from conftest import Golden
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_fignn_host import FIGNN_CASES, fignn_keywords
from zoo_cases import check_dropin


@pytest.mark.parametrize("case", FIGNN_CASES)
def test_reference_fignn_runs_on_the_native_layers(case, patched_reference, tmp_path):  # noqa: F811
    from fuxictr_amd import layers
    from model_zoo import FiGNN
    g = Golden(case)
    check_dropin(FiGNN, g, tmp_path, [("embedding_layer", layers.FeatureEmbedding)], **fignn_keywords(g))
