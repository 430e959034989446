"""A/B of the group metrics (gAUC, avgAUC, MRR, NDCG(k=5)), one process, one GPU:
  host    rank_model.group_metric_values on float64 numpy arrays (two stable argsorts + reduceat), including the
          D->H copy of predictions and labels that BaseModel.evaluate pays on that path;
  device  ops.group_metrics (csrc/fx_group_metrics.hip) on device-resident predictions and labels, including the
          upload of the uint32 group keys and the read-back of the sums.
n = 2^20 and 2^22; group sizes follow a power law (Zipf 2.0 capped at 5000: most users have a handful of rows, a
few have thousands — the shape of Taobao's users per validation set), plus one case of a single group.
Device time: events around `--iters` calls after warm-up; host time: perf_counter around one call; `--repeats`
repeats of each, alternated; prints median and min-max and one JSON line.
    python scripts/bench_group_metrics.py [--iters 20] [--repeats 5] [--out profiles/group_metrics_ab.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuxictr_amd import ops  # noqa: E402
from fuxictr_amd.rank_model import group_keys, group_metric_values  # noqa: E402

NAMES = ["gAUC", "avgAUC", "MRR", "NDCG(k=5)"]
KS = [5]


def make_case(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "one_group":
        ids = np.zeros(n, dtype=np.int64)
    else:
        sizes = np.minimum(rng.zipf(2.0, size=n), 5000)
        sizes = sizes[:np.searchsorted(np.cumsum(sizes), n) + 1]
        ids = rng.permutation(np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)[:n])
    y = (rng.random(n) < 0.05).astype(np.float32)
    p = (1.0 / (1.0 + np.exp(-(rng.normal(size=n) + 1.5 * y - 3.0)))).astype(np.float32)
    return y, p, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_group_metrics.py needs cuda:0"
    dev = torch.device("cuda:0")
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("group metrics %s: host numpy (incl. D->H of predictions, labels) vs ops.group_metrics (incl. key upload, "
        "read-back); %s; median [min-max] ms over %d repeats" % (NAMES, torch.cuda.get_device_name(0),
                                                                 args.repeats))
    for kind, n in [("power_law", 1 << 20), ("power_law", 1 << 22), ("one_group", 1 << 20),
                    ("one_group", 1 << 22)]:
        y, p, ids = make_case(kind, n)
        p_dev, y_dev = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
        t0 = time.perf_counter()
        keys, bits = group_keys(ids)
        t_keys = 1e3 * (time.perf_counter() - t0)
        keys_i32 = torch.from_numpy(keys.view(np.int32))

        def device_call():
            return ops.group_metrics(p_dev, y_dev, keys_i32.to(dev), bits, KS)

        def host_call():
            return group_metric_values(y_dev.cpu().numpy().astype(np.float64),
                                       p_dev.cpu().numpy().astype(np.float64), ids, NAMES)
        got, ref = device_call(), host_call()
        diff = max(abs(got[k] - ref[k]) for k in NAMES)
        for _ in range(3):
            device_call()
        t_dev, t_host = [], []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                device_call()
            e1.record()
            torch.cuda.synchronize()
            t_dev.append(e0.elapsed_time(e1) / args.iters)
            t0 = time.perf_counter()
            host_call()
            t_host.append(1e3 * (time.perf_counter() - t0))
        r = {"case": kind, "n": n, "groups": int(np.unique(ids).size), "key_bits": bits,
             "device_ms": statistics.median(t_dev), "device_min_ms": min(t_dev), "device_max_ms": max(t_dev),
             "host_ms": statistics.median(t_host), "host_min_ms": min(t_host), "host_max_ms": max(t_host),
             "host_key_mapping_ms": t_keys, "max_abs_diff": diff}
        r["speedup"] = r["host_ms"] / r["device_ms"]
        results.append(r)
        say("%-10s n=%8d groups=%8d key_bits=%2d  device %8.3f [%.3f-%.3f]  host %9.1f [%.1f-%.1f]  x%.0f  "
            "(key mapping on the host, paid once per evaluation: %.1f ms; max |device - host| %.2e)"
            % (kind, n, r["groups"], bits, r["device_ms"], r["device_min_ms"], r["device_max_ms"], r["host_ms"],
               r["host_min_ms"], r["host_max_ms"], r["speedup"], t_keys, diff))
    say(json.dumps({"bench": "group_metrics", "iters": args.iters, "repeats": args.repeats, "results": results}))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
