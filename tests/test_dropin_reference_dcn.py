"""Drop-in check of DCN against the reference's OWN model class (build container only: skipped where no reference
checkout is importable, like tests/test_dropin_reference_zoo.py).  After `fuxictr_amd.patch.install()` the
reference's unmodified `model_zoo.DCN` is constructed from layers.CrossNet (the fused node: one cross_net_fwd and one
cross_net_bwd per step) and layers.MLP_Block and — with the kernels replaced by the CPU emulations of
tests/_cpu_emul.py and tests/test_dcn_host.py — reproduces the fixtures the same class produced on the stock torch
layers."""
import pytest

from conftest import Golden
from test_dropin_reference_zoo import pytestmark, patched_reference  # noqa: F401  (skip rule, fixture)
from test_dcn_host import CALLS, DCN_CASES, _install
from zoo_cases import check_dropin


@pytest.mark.parametrize("case", DCN_CASES)
def test_reference_dcn_runs_on_the_native_layers(case, patched_reference, monkeypatch, tmp_path):  # noqa: F811
    _install(monkeypatch)
    from fuxictr_amd import layers
    from model_zoo import DCN
    assert DCN.__module__.startswith("model_zoo")
    g = Golden(case)
    m = g.meta
    # one cross_net_fwd per forward, one launch-pair per step; the tower is there exactly where the case has one
    tower = layers.MLP_Block if m["dnn"] else type(None)
    check_dropin(DCN, g, tmp_path, [("crossnet", layers.CrossNet), ("dnn", tower)],
                 calls=CALLS, forward_calls={"cross_net_fwd": 1, "cross_net_bwd": 0},
                 final_calls={"cross_net_fwd": m["steps"] + 1, "cross_net_bwd": m["steps"]},
                 dnn_hidden_units=m["dnn"], dnn_activations="relu", num_cross_layers=m["n_cross"])
