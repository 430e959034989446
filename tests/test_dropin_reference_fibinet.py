"""Drop-in check of FiBiNET against the reference's OWN model class (build container only: skipped where no
reference checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()`
the reference's unmodified `model_zoo.FiBiNET` is constructed from layers.SqueezeExcitation and
layers.BilinearInteractionV2 (the unfused composition: V, the two branch tensors and their cat) and — with the
kernels replaced by the CPU emulations of tests/_cpu_emul.py and tests/test_fibinet_host.py — reproduces the
fixtures the same class produced on the stock torch layers."""
import pytest

from conftest import Golden
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_fibinet_host import FIBINET_CASES, _install
from zoo_cases import check_dropin


@pytest.mark.parametrize("case", FIBINET_CASES)
def test_reference_fibinet_runs_on_the_native_layers(case, patched_reference, monkeypatch, tmp_path):  # noqa: F811
    _install(monkeypatch)
    from fuxictr_amd import layers
    from model_zoo import FiBiNET
    g = Golden(case)
    m = g.meta
    check_dropin(FiBiNET, g, tmp_path, [("senet_layer", layers.SqueezeExcitation),
                                        ("bilinear_interaction1", layers.BilinearInteractionV2)],
                 hidden_units=m["hidden"], excitation_activation=m["excitation"], reduction_ratio=m["ratio"],
                 bilinear_type=m["bilinear_type"])
