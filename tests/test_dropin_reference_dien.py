"""Drop-in check of DIEN against the reference's OWN model class (build container only: skipped where no reference
checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the reference's
unmodified `model_zoo.DIEN` is constructed from layers.FeatureEmbeddingDict and layers.MLP_Block; it keeps torch's own
nn.GRU, its DynamicGRU cells, its packing and its host read of the lengths (the fused recurrence is zoo.DIEN's) and —
with the kernels replaced by the CPU emulations of tests/_cpu_emul.py — reproduces the fixtures the same class
produced on the stock torch layers."""
import pytest

from conftest import Golden
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_dien_host import DIEN_CASES, _field
from zoo_cases import check_dropin


@pytest.mark.parametrize("case", DIEN_CASES)
def test_reference_dien_runs_on_the_native_layers(case, patched_reference, tmp_path):  # noqa: F811
    from fuxictr_amd import layers
    from model_zoo import DIEN
    g = Golden(case)
    m = g.meta
    check_dropin(DIEN, g, tmp_path, [("embedding_layer", layers.FeatureEmbeddingDict), ("dnn", layers.MLP_Block)],
                 dnn_hidden_units=m["hidden"], dnn_activations=m["dnn_activations"], batch_norm=m["batch_norm"],
                 dien_target_field=[_field(f) for f in m["dien_target"]],
                 dien_sequence_field=[_field(f) for f in m["dien_sequence"]],
                 dien_neg_seq_field=[_field(f) for f in m["dien_neg"]], gru_type=m["gru_type"],
                 enable_sum_pooling=m["sum_pooling"], attention_type=m["attention_type"],
                 use_attention_softmax=m["use_softmax"], aux_loss_alpha=0)
