"""The host group metrics of rank_model.evaluate_metrics (gAUC, avgAUC, MRR, NDCG(k=K)) against the values the
reference's fuxictr.metrics.evaluate_metrics gave on tests/golden/group_metrics.npz
(tests/golden/make_golden_group_metrics.py), their tie rule, their names and their errors.  No GPU."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuxictr_amd.rank_model import evaluate_metrics, group_keys, ndcg_cutoff

TOL = 1e-12      # absolute, as tests/test_gpu_kernels.py::test_binary_metrics_match_sklearn


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "group_metrics.npz"))


@pytest.mark.parametrize("case", ["a", "b"])
def test_host_group_metrics_match_the_reference(fixture, case):
    """Case A: predictions distinct inside every group, all five group metrics + AUC + logloss.  Case B: heavy
    ties (21 distinct predictions), gAUC and avgAUC — the reference defines nothing else under ties."""
    z = fixture
    names = [str(m) for m in z["names_" + case]]
    got = evaluate_metrics(z["y_true"].astype(np.float64), z["y_pred_" + case].astype(np.float64), names,
                           z["group_id"])
    assert list(got.keys()) == names
    for name, ref in zip(names, z["values_" + case]):
        print("%s: host %.17g reference %.17g diff %.3g" % (name, got[name], ref, abs(got[name] - ref)))
    for name, ref in zip(names, z["values_" + case]):
        assert abs(got[name] - ref) <= TOL, (name, got[name], ref)


def test_tie_rule_later_sample_ranks_first():
    """One group of 6; the three 0.5s are a tie run.  Descending order with the later sample first among equal
    predictions: s5 (0.9, y 0), s4 (0.5, y 1), s3 (0.5, y 0), s1 (0.5, y 0), s2 (0.3, y 1), s0 (0.1, y 0)."""
    y = np.array([0, 0, 1, 0, 1, 0], dtype=np.float64)
    p = np.array([0.1, 0.5, 0.3, 0.5, 0.5, 0.9])
    g = np.zeros(6, dtype=np.int64)
    got = evaluate_metrics(y, p, ["MRR", "NDCG(k=1)", "NDCG(k=2)", "NDCG(k=5)", "gAUC", "avgAUC"], g)
    assert abs(got["MRR"] - (1 / 2 + 1 / 5) / (2 + 1e-12)) <= 1e-15
    assert got["NDCG(k=1)"] == 0.0
    idcg2 = 1.0 + 1.0 / np.log2(3.0)
    assert abs(got["NDCG(k=2)"] - (1.0 / np.log2(3.0)) / (idcg2 + 1e-12)) <= 1e-15
    assert abs(got["NDCG(k=5)"] - (1.0 / np.log2(3.0) + 1.0 / np.log2(6.0)) / (idcg2 + 1e-12)) <= 1e-15
    # ascending average ranks: 0.1 -> 1, 0.3 -> 2, the 0.5s -> 4, 0.9 -> 6; positives: 2 + 4; U = 6 - 3 = 3
    assert got["gAUC"] == 3.0 / 8.0 and got["avgAUC"] == 3.0 / 8.0
    # the same samples with the tie run reversed in the input: the positive now comes first, so it ranks last
    order = np.array([0, 4, 2, 3, 1, 5])
    swapped = evaluate_metrics(y[order], p[order], ["MRR", "gAUC"], g)
    assert abs(swapped["MRR"] - (1 / 4 + 1 / 5) / (2 + 1e-12)) <= 1e-15
    assert swapped["gAUC"] == 3.0 / 8.0


def test_ndcg_names():
    rng = np.random.default_rng(0)
    y = (rng.random(200) < 0.4).astype(np.float64)
    p = rng.random(200)
    g = rng.integers(0, 17, size=200)
    got = evaluate_metrics(y, p, ["NDCG(3)", "NDCG(k=3)"], g)
    assert got["NDCG(3)"] == got["NDCG(k=3)"] and 0.0 < got["NDCG(3)"] < 1.0
    assert ndcg_cutoff("NDCG(k=12)") == 12 and ndcg_cutoff("NDCG(7)") == 7
    for bad in ["NDCG", "NDCG()", "NDCG(k=0)", "NDCG(k=-1)", "NDCG(k=__import__('os'))", "NDCG(k=3) "]:
        with pytest.raises(NotImplementedError):
            evaluate_metrics(y, p, [bad], g)


def test_errors():
    y, p, g = np.array([0.0, 1.0]), np.array([0.2, 0.7]), np.array([1, 1])
    with pytest.raises(ValueError, match="not supported"):
        evaluate_metrics(y, p, ["gAUC", "accuracy"], g)
    for name in ["gAUC", "avgAUC", "MRR", "NDCG(k=2)"]:
        with pytest.raises(AssertionError, match="group_index is required."):
            evaluate_metrics(y, p, [name])
    assert list(evaluate_metrics(y, p, ["AUC", "logloss"]).keys()) == ["AUC", "logloss"]   # as before


def test_single_class_groups_give_nan():
    y = np.array([1, 1, 0, 0, 0], dtype=np.float64)
    p = np.array([0.3, 0.6, 0.2, 0.9, 0.5])
    g = np.array([5, 5, 9, 9, 9])
    got = evaluate_metrics(y, p, ["gAUC", "avgAUC", "MRR", "NDCG(k=1)"], g)
    assert np.isnan(got["gAUC"]) and np.isnan(got["avgAUC"])
    assert abs(got["MRR"] - 0.5 * (1.0 + 0.5) / (2 + 1e-12)) <= 1e-15      # the all-negative group adds 0
    assert abs(got["NDCG(k=1)"] - 0.5 / (1.0 + 1e-12)) <= 1e-15


def test_group_keys():
    keys, bits = group_keys(np.array([-50, 20, -50, 6], dtype=np.int64))
    assert keys.dtype == np.uint32 and keys.tolist() == [0, 70, 0, 56] and bits == 7
    wide = np.array([-50, 10 ** 12, -50, 3], dtype=np.int64)
    keys, bits = group_keys(wide)
    assert keys.tolist() == [0, 2, 0, 1] and bits == 2
    keys, bits = group_keys(np.array(["b", "a", "b"]))
    assert keys.tolist() == [1, 0, 1] and bits == 1
    keys, bits = group_keys(np.array([4, 4, 4]))
    assert keys.tolist() == [0, 0, 0] and bits == 1
    keys, bits = group_keys(np.array([0, 2 ** 32 - 1], dtype=np.uint64))
    assert keys.tolist() == [0, 2 ** 32 - 1] and bits == 32
