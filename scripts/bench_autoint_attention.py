"""A/B of AutoInt's attention stack, forward + backward, one process, one GPU:
  baseline  the stack composed from torch-ROCm ops on the same tensors (the fp32 restatement of
            tests/test_gpu_mhsa.py on cuda:0) — what a user without the native layer runs;
  native    layers.MultiHeadSelfAttention (csrc/fx_mhsa.hip).
Device events around `--iters` iterations after warm-up, the two variants alternated, `--repeats` repeats each;
prints median and min-max per variant and shape, the achieved bytes/s of the native path against its algorithmic
bytes (X read + Y written forward; X, Y, dY read + dX written backward), and one JSON line.
    python scripts/bench_autoint_attention.py [--iters 200] [--repeats 5] [--profile-native]
--profile-native runs only a few native iterations (for a kernel trace: launches per layer).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fuxictr_amd import layers  # noqa: E402
from test_gpu_mhsa import mhsa_reference  # noqa: E402

#          B     F   D   A   H  layers
SHAPES = [(4096, 39, 16, 16, 2, 3), (10000, 39, 40, 40, 2, 3)]


def make_stack(shape, dev):
    B, F, D, A, H, n = shape
    torch.manual_seed(0)
    layers.set_default_device(dev)
    stack = [layers.MultiHeadSelfAttention(D if i == 0 else A, attention_dim=A, num_heads=H).to(dev)
             for i in range(n)]
    x = torch.randn(B, F, D, device=dev, requires_grad=True)
    dy = torch.randn(B, F, A, device=dev)
    return stack, x, dy


def native_step(stack, x, dy):
    h = x
    for layer in stack:
        h = layer(h)
    h.backward(dy)


def baseline_step(stack, x, dy):
    h = x
    for layer in stack:
        h = mhsa_reference(h, layer.W_q.weight, layer.W_k.weight, layer.W_v.weight,
                           layer.W_res.weight if layer.W_res is not None else None, layer.num_heads,
                           layer.use_scale, layer.use_residual, True)
    h.backward(dy)


def drop_grads(stack, x):
    """No accumulation into .grad of an earlier iteration: every backward hands its gradients over as they are."""
    x.grad = None
    for layer in stack:
        for p in layer.parameters():
            p.grad = None


def timed(fn, stack, x, dy, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        drop_grads(stack, x)
        fn(stack, x, dy)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per forward + backward of the stack


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--profile-native", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {}
    for shape in SHAPES:
        stack, x, dy = make_stack(shape, dev)
        if args.profile_native:
            for _ in range(3):
                native_step(stack, x, dy)
            torch.cuda.synchronize()
            continue
        for _ in range(args.warmup):
            native_step(stack, x, dy)
            baseline_step(stack, x, dy)
        torch.cuda.synchronize()
        runs = {"native": [], "baseline": []}
        for _ in range(args.repeats):                  # alternated
            runs["baseline"].append(timed(baseline_step, stack, x, dy, args.iters))
            runs["native"].append(timed(native_step, stack, x, dy, args.iters))
        B, F, D, A, H, n = shape
        # algorithmic bytes of the native stack: per layer X + Y forward, X + Y + dY + dX backward
        nbytes = 0
        for i in range(n):
            d_in = D if i == 0 else A
            nbytes += 4 * B * F * ((d_in + A) + (d_in + A + A + d_in))
        med = {k: statistics.median(v) for k, v in runs.items()}
        key = "B%d_F%d_D%d_A%d_H%d_L%d" % shape
        result[key] = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in runs.items()}
        result[key]["native_GBps_algorithmic"] = nbytes / med["native"] * 1e-3
        result[key]["native_wins"] = med["native"] < min(runs["baseline"])
        for k in ("baseline", "native"):
            print("%-28s %-8s median %9.1f us  min %9.1f  max %9.1f" % (key, k, med[k], min(runs[k]),
                                                                         max(runs[k])))
        print("%-28s native: %.0f GB/s of algorithmic bytes (%.1f MB); native median < baseline min: %s"
              % (key, result[key]["native_GBps_algorithmic"], nbytes / 1e6, result[key]["native_wins"]))
    if result:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
