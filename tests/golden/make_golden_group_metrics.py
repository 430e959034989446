"""Generate tests/golden/group_metrics.npz by running the REAL reference's fuxictr.metrics.evaluate_metrics
(pandas.groupby + a process pool + one roc_auc_score call per group) on seeded synthetic data.

Run in the build container only (the reference does not travel to the GPU box):
    python tests/golden/make_golden_group_metrics.py
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed file).

Case A: ~6000 samples, power-law group sizes, ids of the form c * 7 - 50 (negative ids) and, in a second copy,
the same shifted by 10^12 (ids wider than 32 bits); predictions are distinct inside every group, so the
reference's unstable argsort()[::-1] defines every metric.  Case B: the same data with the predictions rounded
to 1/20 (21 values, heavy ties): only gAUC and avgAUC are recorded, the reference defines nothing else there.
The generator asserts that the data cover what the tests rely on."""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

METRICS_A = ["gAUC", "avgAUC", "MRR", "NDCG(k=1)", "NDCG(k=5)", "AUC", "logloss"]
METRICS_B = ["gAUC", "avgAUC"]


def make_data(seed=20240607):
    rng = np.random.default_rng(seed)
    # one group longer than the sort's 2048-item tile, a power-law tail, a block of one-sample groups
    sizes = [2100] + [int(s) for s in np.minimum(rng.zipf(1.7, size=150), 60)] + [1] * 40
    sizes = np.asarray(sizes)
    ids = np.arange(sizes.size, dtype=np.int64) * 7 - 50
    g = np.repeat(ids, sizes)
    g = np.concatenate([g, g + 10 ** 12])                      # the second copy: other groups, wide ids
    n = g.size
    y = (rng.random(n) < 0.3).astype(np.float32)
    big = [i for i in ids[1:] if (np.repeat(ids, sizes) == i).sum() >= 3]
    y[g == big[0]] = 1.0                                       # an all-positive group
    y[g == big[1]] = 0.0                                       # an all-negative group
    # n distinct float32 predictions, correlated with the label
    score = rng.random(n) + 0.35 * y
    p = ((np.argsort(np.argsort(score)) + 0.5) / n).astype(np.float32)
    perm = rng.permutation(n)                                  # groups interleaved in the input
    return y[perm], p[perm], g[perm]


def _groups(g):
    order = np.argsort(g, kind="stable")
    gs = g[order]
    starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
    return [order[a:b] for a, b in zip(starts, np.r_[starts[1:], g.size])]


def check_coverage(y, p_a, p_b, g):
    groups = _groups(g)
    sizes = np.asarray([len(ix) for ix in groups])
    assert all(np.unique(p_a[ix]).size == len(ix) for ix in groups), "case A: tied predictions in a group"
    assert (sizes == 1).any(), "no group of one sample"
    assert any(len(ix) > 1 and y[ix].all() for ix in groups), "no all-positive group"
    assert any(len(ix) > 1 and not y[ix].any() for ix in groups), "no all-negative group"
    assert sizes.max() > 2048, "no group longer than the sort's tile"
    assert g.min() < 0 and g.max() - g.min() >= 2 ** 32, "ids neither negative nor wide"
    mixed_run = False
    for ix in groups:
        for v in np.unique(p_b[ix]):
            run = y[ix][p_b[ix] == v]
            mixed_run |= bool(run.size > 1 and run.any() and not run.all())
    assert mixed_run, "case B: no tie run with positives and negatives"


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from fuxictr.metrics import evaluate_metrics
    y, p_a, g = make_data()
    p_b = (np.round(p_a.astype(np.float64) * 20.0) / 20.0).astype(np.float32)
    check_coverage(y, p_a, p_b, g)
    y64 = y.astype(np.float64)
    ref_a = evaluate_metrics(y64, p_a.astype(np.float64), METRICS_A, g)
    ref_b = evaluate_metrics(y64, p_b.astype(np.float64), METRICS_B, g)
    out = os.path.join(os.environ.get("FX_GOLDEN_OUT") or HERE, "group_metrics.npz")
    np.savez_compressed(out, y_true=y, y_pred_a=p_a, y_pred_b=p_b, group_id=g,
                        names_a=np.asarray(METRICS_A), values_a=np.asarray([ref_a[m] for m in METRICS_A]),
                        names_b=np.asarray(METRICS_B), values_b=np.asarray([ref_b[m] for m in METRICS_B]))
    print("%s: n=%d, %d groups, %d bytes" % (out, y.size, np.unique(g).size, os.path.getsize(out)))
    for m in METRICS_A:
        print("  A %-10s %.17g" % (m, ref_a[m]))
    for m in METRICS_B:
        print("  B %-10s %.17g" % (m, ref_b[m]))


if __name__ == "__main__":
    main()
