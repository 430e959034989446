"""The shared checks of tests/zoo_cases.py still bite (no GPU): on fixture dcn_one_layer (B = 64, three steps, one cross
layer), built the way tests/test_dcn_host.py builds it, they pass with the fixture untouched and raise on each
perturbation of a copy of the arrays the Golden object holds (the file is never touched)."""
import pytest

from conftest import Golden
from test_dcn_host import _build
from zoo_cases import LOGIT_TOL, check_forward, check_trajectory


def _golden():
    g = Golden("dcn_one_layer")
    for part in (g.state0, g.state1, g.expect):
        for k in part:
            part[k] = part[k].copy()
    return g


def test_the_untouched_fixture_passes(tmp_path, monkeypatch):
    g = _golden()
    model = _build(g, tmp_path, monkeypatch)
    check_forward(model, g, "0")
    check_trajectory(model, g)


def test_a_shifted_logit_fails_the_forward_check(tmp_path, monkeypatch):
    g = _golden()
    g.expect["logit0"][0] += 2 * LOGIT_TOL
    with pytest.raises(AssertionError):
        check_forward(_build(g, tmp_path, monkeypatch), g, "0")


def _a_float_weight(g):
    g.state1[next(k for k, v in g.state1.items() if v.dtype.kind == "f")].reshape(-1)[0] += 0.1


@pytest.mark.parametrize("perturb, message", [
    (lambda g: g.expect["loss"].__setitem__(1, g.expect["loss"][1] + 2e-4), "atol=0.0001"),
    (lambda g: g.expect["pred1"].__setitem__(0, g.expect["pred1"][0] + 1e-4), "atol=2e-05"),
    # 0.1 is above lr * steps + tol = 0.03002 of this case: assert_weights_close's second assertion
    (_a_float_weight, r"^\('[^']+', 0\.(09|10)\d*\)"),
], ids=["loss", "pred1", "state1"])
def test_a_shifted_loss_prediction_or_weight_fails_the_trajectory_check(perturb, message, tmp_path, monkeypatch):
    g = _golden()
    assert g.meta["lr"] * g.meta["steps"] + 2e-5 < 0.1
    perturb(g)
    with pytest.raises(AssertionError, match=message):
        check_trajectory(_build(g, tmp_path, monkeypatch), g)


def test_a_renamed_key_fails_the_build(tmp_path, monkeypatch):
    g = _golden()
    g.state0["renamed." + "fc.weight"] = g.state0.pop("fc.weight")
    with pytest.raises(AssertionError):
        _build(g, tmp_path, monkeypatch)
