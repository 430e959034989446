"""fx_group_metrics (csrc/fx_group_metrics.hip) on a real MI355X: against the reference's values on
tests/golden/group_metrics.npz, against the host restatement rank_model.group_metric_values over sizes and group
patterns that put group and tie-run boundaries on wave (64), tile (1024 / 2048) and chunk edges, its determinism,
its argument errors, and BaseModel.evaluate's device path against its host path."""
import copy
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLDEN, Golden
from fuxictr_amd import _lib, ops
from fuxictr_amd.rank_model import Monitor, group_keys, group_metric_values

pytestmark = pytest.mark.gpu

TOL = 1e-12      # absolute, as tests/test_gpu_kernels.py::test_binary_metrics_match_sklearn
KS = [1, 3, 10]
NAMES = ["gAUC", "avgAUC", "MRR"] + ["NDCG(k=%d)" % k for k in KS]
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 70000]
PATTERNS = ["one_group", "own_group", "groups_of_64", "groups_of_65", "power_law", "heavy_ties", "saturated",
            "key_bits_1", "key_bits_32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_metrics(y, p, keys, bits, ks=KS):
    return ops.group_metrics(_dev(p), _dev(y), _dev(keys.view(np.int32)), bits, ks)


def _agree(got, ref, names):
    for name in names:
        print("%s: device %.17g host %.17g" % (name, got[name], ref[name]))
    for name in names:
        if np.isnan(ref[name]):
            assert np.isnan(got[name]), (name, got[name])
        else:
            assert abs(got[name] - ref[name]) <= TOL, (name, got[name], ref[name])


def _power_law_ids(rng, n):
    """One big group (5000 samples at n = 70000, n // 2 below 10000) and Zipf-sized small ones."""
    big = 5000 if n >= 10000 else n // 2
    sizes = [big]
    while sum(sizes) < n:
        sizes.append(int(min(rng.zipf(1.6), 300)))
    return np.repeat(np.arange(len(sizes)), sizes)[:n]


_CASES = {}


def _case(pattern, n):
    """(labels, predictions, uint32 keys, key bits, host metrics), computed once per (pattern, n)."""
    if (pattern, n) in _CASES:
        return _CASES[(pattern, n)]
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + n)
    y = (rng.random(n) < 0.35).astype(np.float32)
    p = rng.random(n).astype(np.float32)
    bits = None
    if pattern == "one_group":
        ids = np.zeros(n, dtype=np.int64)
    elif pattern == "own_group":
        ids = rng.permutation(n)
    elif pattern == "groups_of_64":
        ids = np.arange(n) // 64                 # in input order: group edges on wave and tile edges
    elif pattern == "groups_of_65":
        ids = np.arange(n) // 65
    elif pattern == "power_law":
        ids = rng.permutation(_power_law_ids(rng, n))
    elif pattern == "heavy_ties":
        ids = rng.permutation(_power_law_ids(rng, n))
        p = (np.round(rng.random(n) * 20.0) / 20.0).astype(np.float32)       # 21 distinct predictions
    elif pattern == "saturated":
        ids = rng.permutation(_power_law_ids(rng, n))
        p = np.where(rng.random(n) < 0.7, (rng.random(n) < 0.5).astype(np.float32), p).astype(np.float32)
    elif pattern == "key_bits_1":
        ids = rng.integers(0, 2, size=n)
        bits = 1
    else:
        ids = rng.choice(np.array([2 ** 31, 2 ** 32 - 1, 2 ** 31 + 2 ** 16, 7, 2 ** 24 + 5, 2 ** 8],
                                  dtype=np.int64), size=n)
        bits = 32
    if bits is None:
        keys, bits = group_keys(ids)
    else:
        keys = ids.astype(np.uint32)
    ref = group_metric_values(y.astype(np.float64), p.astype(np.float64), keys, NAMES)
    _CASES[(pattern, n)] = (y, p, keys, bits, ref)
    return _CASES[(pattern, n)]


@pytest.mark.parametrize("case", ["a", "b"])
def test_group_metrics_match_the_reference(case):
    z = np.load(os.path.join(GOLDEN, "group_metrics.npz"))
    names = [str(m) for m in z["names_" + case] if str(m) not in ("AUC", "logloss")]
    keys, bits = group_keys(z["group_id"])
    got = _device_metrics(z["y_true"], z["y_pred_" + case], keys, bits, [1, 5])
    ref = {str(m): float(v) for m, v in zip(z["names_" + case], z["values_" + case])}
    _agree(got, ref, names)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_group_metrics_match_the_host(pattern, n):
    y, p, keys, bits, ref = _case(pattern, n)
    _agree(_device_metrics(y, p, keys, bits), ref, NAMES)


def test_eight_cutoffs_and_none():
    y, p, keys, bits, _ = _case("heavy_ties", 2049)
    ks = [1, 2, 3, 5, 8, 64, 1000, 10 ** 6]
    names = ["gAUC", "avgAUC", "MRR"] + ["NDCG(k=%d)" % k for k in ks]
    ref = group_metric_values(y.astype(np.float64), p.astype(np.float64), keys, names)
    _agree(_device_metrics(y, p, keys, bits, ks), ref, names)
    got = _device_metrics(y, p, keys, bits, [])
    assert list(got.keys()) == ["gAUC", "avgAUC", "MRR"]
    _agree(got, ref, ["gAUC", "avgAUC", "MRR"])


def test_two_runs_give_the_same_bits():
    y, p, keys, bits, _ = _case("heavy_ties", 70000)
    runs = [_device_metrics(y, p, keys, bits) for _ in range(2)]
    a, b = ([struct.pack("<d", r[name]) for name in NAMES] for r in runs)
    assert a == b


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    n = 100
    y, p = _dev(np.zeros(n, dtype=np.float32)), _dev(np.full(n, 0.5, dtype=np.float32))
    keys = _dev(np.zeros(n, dtype=np.int32))
    nbytes = int(lib.fx_group_metrics_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    out = torch.full((2 * (3 + 8) + 1,), -7.0, dtype=torch.float64, device="cuda:0")
    ks9 = (ctypes.c_int32 * 9)(*range(1, 10))
    stream = _lib.stream_ptr(y.device)

    def call(n_, ks, nk, nb, bits=1):
        return lib.fx_group_metrics(_lib.ptr(p), _lib.ptr(y), _lib.ptr(keys), bits, n_, ks, nk, _lib.ptr(ws), nb,
                                    _lib.ptr(out), stream)
    assert call(0, ks9, 1, nbytes) == 1 and b"n=0" in lib.fx_last_error()
    assert call(2 ** 26 + 1, ks9, 1, nbytes) == 1
    assert call(n, ks9, 9, nbytes) == 1 and b"cut-offs" in lib.fx_last_error()
    assert call(n, ks9, 1, nbytes - 257) == 1 and b"workspace too small" in lib.fx_last_error()
    assert call(n, ks9, 1, nbytes, bits=0) == 1 and call(n, ks9, 1, nbytes, bits=33) == 1
    zero = (ctypes.c_int32 * 1)(0)
    assert call(n, zero, 1, nbytes) == 1 and b"< 1" in lib.fx_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    with pytest.raises(_lib.FxError):
        ops.group_metrics(p, y, keys, 1, list(range(1, 10)))
    assert call(n, ks9, 8, nbytes) == 0
    torch.cuda.synchronize()
    assert float(out[5]) == 1.0 and float(out[2 * (3 + 8)]) == 1.0      # one group


def test_model_evaluate_device_path_equals_host_path(tmp_path):
    """DeepFM over a DeviceNpzDataLoader with a `meta` uid column: evaluate with device metrics on
    (fx_binary_metrics + fx_group_metrics) and with device_metrics=False (scikit-learn + numpy)."""
    from fuxictr_amd import zoo
    from fuxictr_amd.dataloader import DeviceNpzDataLoader
    from fuxictr_amd.features import FeatureMap
    from make_golden import make_batches
    g = Golden("deepfm_adam")
    m = g.meta
    rng = np.random.default_rng(11)
    full = dict(make_batches(rng, g.spec, 900, 1)[0])
    full["label"] = (rng.random(900) < 0.4).astype(np.float32)
    full["uid"] = rng.integers(0, 60, size=900).astype(np.int64) * 7 - 50
    path = str(tmp_path / "valid.npz")
    np.savez(path, **full)
    spec = copy.deepcopy(g.spec)
    spec["features"].append({"uid": {"type": "meta"}})
    fmap = FeatureMap(spec["dataset_id"], str(tmp_path))
    fmap.load_dict(spec, {"embedding_dim": m["embedding_dim"], "group_id": "uid"})
    assert fmap.group_id == "uid"
    metrics = ["gAUC", "avgAUC", "MRR", "NDCG(k=3)", "AUC", "logloss"]
    results = []
    for device_metrics in (True, False):
        model = zoo.DeepFM(fmap, model_id="gm%d" % device_metrics, gpu=0, embedding_dim=m["embedding_dim"],
                           hidden_units=m["hidden"], learning_rate=m["lr"], optimizer="adam",
                           loss="binary_crossentropy", task="binary_classification", metrics=metrics,
                           verbose=0, model_root=str(tmp_path), device_metrics=device_metrics)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state0.items()})
        va = DeviceNpzDataLoader(fmap, path, batch_size=256, device="cuda:0")
        results.append(model.evaluate(va, metrics=metrics))
    dev, host = results
    assert list(dev.keys()) == metrics and list(host.keys()) == metrics
    _agree(dev, host, metrics)
    assert 0.0 < dev["gAUC"] < 1.0 and 0.0 < dev["NDCG(k=3)"] < 1.0
    mon = Monitor({"gAUC": 1, "AUC": 1})
    assert mon.get_value(dev) == dev["gAUC"] + dev["AUC"]
