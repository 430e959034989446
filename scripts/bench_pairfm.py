"""A/B of the field-pair interaction of FwFM / FmFM alone, one process, one GPU, the project's Criteo shape
(B 4096, F 39, D 16: P = 741 pairs), the three modes:
  composition  the reference's own formula in plain torch ops (FmFM.py:84-90): index_select x 2 -> [B, P, D] each,
               then matmul against [P, D, D] ("matrix"), the product with [P, D] ("vector") or with [P] ("scalar"),
               the two sums; torch autograd for the backward: the yardstick;
  fused        layers.pair_interaction: one launch of csrc/fx_pairfm.hip forward; backward one launch for dX, one for
               the weight gradient over slabs of samples and the fixed-order reduce.
Device events around `--iters` iterations after warm-up, the variants alternated, `--repeats` repeats each; prints
median and min-max per variant for the forward alone and for forward + backward, and for pairfm_fwd / pairfm_bwd
alone the achieved fraction of the roofline time DESIGN.md derives (the larger of bytes / HBM peak and flops / fp32
vector peak; 8 TB/s and 157.3 TFLOP/s spec); then one JSON line.
    python scripts/bench_pairfm.py [--iters 20] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuxictr_amd import layers, ops  # noqa: E402

B, F, D = 4096, 39, 16
MODES = ("scalar", "vector", "matrix")
HBM_PEAK = 8.0e12      # bytes / s, MI355X (spec)
F32_PEAK = 157.3e12    # flop / s, MI355X vector fp32 (spec)


def roofline(mode, bwd):
    """(bytes, flops, seconds) of one pass, as DESIGN.md derives them"""
    P = F * (F - 1) // 2
    nW = ops.pairfm_weight_floats(mode, F, D)
    per_pair = 2.0 * D * D + 2.0 * D if mode == "matrix" else 4.0 * D
    if not bwd:
        nbytes, flops = 4.0 * (B * F * D + nW + B), B * P * per_pair
    else:       # X read by both launches, dX written, W read and dW written; ordered pairs (2 x) + the weight gradient
        nbytes, flops = 4.0 * (3 * B * F * D + 2 * nW + B), 3.0 * B * P * per_pair
    return nbytes, flops, max(nbytes / HBM_PEAK, flops / F32_PEAK)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per call


def composition(x, W, mode, index):
    left = torch.index_select(x, 1, index[0])
    right = torch.index_select(x, 1, index[1])
    if mode == "matrix":
        left = torch.matmul(left.unsqueeze(2), W).squeeze(2)
    elif mode == "vector":
        left = left * W
    else:
        left = left * W.reshape(1, -1, 1)
    return (left * right).sum(dim=-1).sum(dim=-1, keepdim=True)


def alternated(variants, iters, repeats, warmup):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            runs[k].append(timed(fn, iters))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pairfm.py measures on the GPU only")
    dev = torch.device("cuda:0")
    layers.set_default_device(dev)
    index = torch.triu_indices(F, F, offset=1).to(dev)
    P = index.shape[1]
    result = {}
    for mode in MODES:
        torch.manual_seed(0)
        shape = (P, D, D) if mode == "matrix" else (P, D) if mode == "vector" else (P,)
        W = (torch.randn(*shape, device=dev) * (D ** -0.5 if mode == "matrix" else 1.0)).requires_grad_(True)
        x = torch.randn(B, F, D, device=dev, requires_grad=True)
        g = torch.randn(B, 1, device=dev)
        fwd = {"composition": lambda: composition(x, W, mode, index),
               "fused": lambda: layers.pair_interaction(x, W, mode)}

        def step(f):
            x.grad = None
            W.grad = None
            torch.autograd.backward(f(), g)

        def no_grad(f):
            with torch.no_grad():
                return f()
        with torch.no_grad():
            base = fwd["composition"]()
            agree = float((fwd["fused"]() - base).abs().max() / base.abs().max())
        key = "B%d_F%d_D%d_%s" % (B, F, D, mode)
        result[key] = {"max_rel_fused_minus_composition": agree}
        for what, variants in (("forward", {k: (lambda f=f: no_grad(f)) for k, f in fwd.items()}),
                               ("forward+backward", {k: (lambda f=f: step(f)) for k, f in fwd.items()})):
            runs = alternated(variants, args.iters, args.repeats, args.warmup)
            med = {k: statistics.median(v) for k, v in runs.items()}
            result[key][what] = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in runs.items()}
            for k in runs:
                print("%-24s %-17s %-12s median %9.1f us  min %9.1f  max %9.1f"
                      % (key, what, k, med[k], min(runs[k]), max(runs[k])))
            print("%-24s %-17s composition / fused: %.2f" % (key, what, med["composition"] / med["fused"]))
        print("%-24s max |fused - composition| / max|.| %.2e" % (key, agree))
        # the two ops alone against their roofline times
        rec = x.detach().reshape(B, F * D)
        Wd = W.detach()
        out, drec = torch.empty(B, 1, device=dev), torch.empty(B, F * D, device=dev)
        grads = torch.empty(ops.pairfm_grad_floats(mode, F, D), device=dev)
        ws = torch.empty(ops.pairfm_workspace_floats(mode, B, F, D), device=dev)
        gv = g.reshape(-1).contiguous()
        for name, fn, bwd in (("pairfm_fwd", lambda: ops.pairfm_fwd(rec, F, D, mode, Wd, None, None, None, out), False),
                              ("pairfm_bwd", lambda: ops.pairfm_bwd(gv, rec, F, D, mode, Wd, None, False, drec, grads,
                                                                    ws), True)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            us = statistics.median(timed(fn, args.iters) for _ in range(5))
            nbytes, flops, roof = roofline(mode, bwd)
            kkey = "%s_kernel_%s" % (key, name)
            result[kkey] = {"median_us": us, "bytes": nbytes, "flops": flops, "roofline_us": roof * 1e6,
                            "fraction_of_roofline": roof * 1e6 / us}
            print("%-44s %9.1f us: %.1f MB, %.2f GFLOP: roofline %.1f us, achieved %.1f %% of it"
                  % (kkey, us, nbytes / 1e6, flops * 1e-9, roof * 1e6, 100 * roof * 1e6 / us))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
