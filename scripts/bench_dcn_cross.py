"""A/B of DCN's rank-1 cross stack, forward + backward, one process, one GPU:
  module_by_module  layers.CrossNet with fused=False: per layer a Linear to one output (the GEMM dispatcher), torch's
                    product and the two sums, as the reference composes them (cross_net.py:54, 89-92): the yardstick;
  torch             the same composition with stock F.linear instead of FxLinear (for orientation only);
  fused             layers._CrossNetFn: csrc/fx_crossnet.hip, one launch forward and two backward for the whole stack.
Shapes: a 3-layer stack at B 4096 and 10000, widths 624 (39 fields x 16) and 1248 (39 x 32).
Device events around `--iters` iterations after warm-up, the variants alternated, `--repeats` repeats each; prints
median and min-max per variant (the min-max of a variant is the run-to-run spread the comparison is read against),
and for the kernels alone the least bytes they must move — forward 2 floats per element; backward 3 floats per
element plus the rows of column partials, written and read once — over their time, next to the HBM peak (8 TB/s
spec); then one JSON line.
    python scripts/bench_dcn_cross.py [--iters 30] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.nn import functional as tF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuxictr_amd import layers, ops  # noqa: E402

BATCHES = [4096, 10000]
WIDTHS = [624, 1248]
N_LAYERS = 3
HBM_PEAK = 8.0e12      # bytes / s, MI355X (spec)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per call


def cross_torch(layer, x):
    x0 = x
    for ci in layer.cross_net:
        x = x + (tF.linear(x, ci.weight.weight) * x0 + ci.bias)
    return x


def kernel_rates(B, D, dev, iters):
    """The forward and the backward alone: (name, us, bytes)."""
    def rnd(*s):
        return torch.randn(*s, device=dev)
    L = N_LAYERS
    x0, dout, w, b = rnd(B, D), rnd(B, D), rnd(L, D) / D ** 0.5, rnd(L, D)
    out, s, dx0 = torch.empty_like(x0), torch.empty(B, L, device=dev), torch.zeros_like(x0)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    nws = ops.cross_net_workspace_floats(B, D, L)
    ws = torch.empty(nws, device=dev)
    cases = [("cross_net_fwd", lambda: ops.cross_net_fwd(x0, w, b, out, s), 4.0 * (B * D * 2.0 + B * L)),
             ("cross_net_bwd", lambda: ops.cross_net_bwd(dout, x0, w, b, s, dx0, dw, db, True, ws),
              4.0 * (B * D * 3.0 + B * L + 2.0 * nws))]
    res = []
    for name, fn, nbytes in cases:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        res.append((name, statistics.median(timed(fn, iters) for _ in range(5)), nbytes))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcn_cross.py measures on the GPU only")
    dev = torch.device("cuda:0")
    layers.set_default_device(dev)
    result = {}
    for D in WIDTHS:
        torch.manual_seed(0)
        layer = layers.CrossNet(D, N_LAYERS)
        with torch.no_grad():
            for ci in layer.cross_net:
                ci.weight.weight.copy_(torch.randn(1, D, device=dev) / D ** 0.5)
                ci.bias.copy_(0.3 * torch.randn(D, device=dev))
        params = list(layer.parameters())
        for B in BATCHES:
            x = torch.randn(B, D, device=dev, requires_grad=True)
            g = torch.randn(B, D, device=dev)

            def run(fused):
                layer.fused = fused
                return layer(x)
            variants = {"module_by_module": lambda: run(False), "torch": lambda: cross_torch(layer, x),
                        "fused": lambda: run(True)}

            def step(fwd):
                for t in params + [x]:
                    t.grad = None
                torch.autograd.backward(fwd(), g)
            with torch.no_grad():
                base = variants["module_by_module"]()
                agree = float((variants["fused"]() - base).abs().max() / base.abs().max())
            for _ in range(args.warmup):
                for fwd in variants.values():
                    step(fwd)
            torch.cuda.synchronize()
            runs = {k: [] for k in variants}
            for _ in range(args.repeats):                  # alternated
                for k, fwd in variants.items():
                    runs[k].append(timed(lambda: step(fwd), args.iters))
            key = "B%d_D%d_stack%d" % (B, D, N_LAYERS)
            med = {k: statistics.median(v) for k, v in runs.items()}
            result[key] = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in runs.items()}
            result[key]["max_rel_fused_minus_module_by_module"] = agree
            # not slower beyond the spread: the fused variant's slowest repeat against the yardstick's fastest
            result[key]["fused_not_slower"] = bool(med["fused"] <= med["module_by_module"]
                                                   or min(runs["fused"]) <= max(runs["module_by_module"]))
            for k in runs:
                print("%-24s %-17s median %9.1f us  min %9.1f  max %9.1f" % (key, k, med[k], min(runs[k]),
                                                                             max(runs[k])))
            print("%-24s module by module / fused, forward + backward: %.2f (torch / fused: %.2f); "
                  "max |fused - module by module| / max|.| %.2e"
                  % (key, med["module_by_module"] / med["fused"], med["torch"] / med["fused"], agree))
            for name, us, nbytes in kernel_rates(B, D, dev, args.iters):
                bw = nbytes / (us * 1e-6)
                kkey = "B%d_D%d_kernel_%s" % (B, D, name)
                result[kkey] = {"median_us": us, "bytes": nbytes, "GBps": bw * 1e-9,
                                "fraction_of_hbm_peak": bw / HBM_PEAK}
                print("%-40s %8.1f us for %.1f MB = %.0f GB/s = %.1f %% of the HBM peak"
                      % (kkey, us, nbytes / 1e6, bw * 1e-9, 100 * bw / HBM_PEAK))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
