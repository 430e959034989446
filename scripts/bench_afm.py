"""A/B of AFM's pairwise attention layer alone, forward + backward, one process, one GPU:
  module_by_module  the reference's composition (AFM.py:84-93): the [B, P, D] products by index_select, the attention
                    nn.Sequential on FxLinear, torch's softmax, weighted sum and weight_p: the yardstick;
  fused             layers.afm_attention: one launch of csrc/fx_afm.hip forward, one launch + the fixed-order reduce
                    backward.
Shapes (B, F, D, A): (4096, 39, 16, 16), the project's Criteo shape, and (10000, 39, 40, 40), the zoo's default config
on Criteo's field count.
Device events around `--iters` iterations after warm-up, the variants alternated, `--repeats` repeats each; prints
median and min-max per variant, and for the two kernels alone the achieved GB/s against the record's bytes (read
forward; read and its gradient written backward) and the FLOP/s against the hidden product's flops (2 P D A per
sample forward; the backward recomputes it twice and forms dW1 and W1^T dz: 5 x), next to the HBM peak (8 TB/s spec)
and the fp32 vector peak (157.3 TFLOP/s spec); then one JSON line.
    python scripts/bench_afm.py [--iters 20] [--repeats 5]
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

SHAPES = [(4096, 39, 16, 16), (10000, 39, 40, 40)]
HBM_PEAK = 8.0e12      # bytes / s, MI355X (spec)
F32_PEAK = 157.3e12    # flop / s, MI355X vector fp32 (spec)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per call


def kernel_rates(shape, att, proj, dev, iters):
    """The two kernels alone: (name, us, bytes, flops)."""
    B, F, D, A = shape
    rec = torch.randn(B, F * D, device=dev)
    g = torch.randn(B, 1, device=dev)
    W1, b1 = att[0].weight.detach(), att[0].bias.detach()
    w2, wp = att[2].weight.detach().reshape(-1), proj.weight.detach().reshape(-1)
    out, stats = torch.empty(B, 1, device=dev), torch.empty(B, 3, device=dev)
    drec = torch.empty_like(rec)
    grads = torch.empty(ops.afm_attn_grad_floats(D, A), device=dev)
    ws = torch.empty(ops.afm_attn_workspace_floats(B, F, D, A), device=dev)
    hidden = 2.0 * B * (F * (F - 1) // 2) * D * A
    cases = [("afm_attn_fwd", lambda: ops.afm_attn_fwd(rec, F, D, W1, b1, w2, wp, None, out, stats),
              4.0 * B * F * D, hidden),
             ("afm_attn_bwd", lambda: ops.afm_attn_bwd(g, rec, F, D, W1, b1, w2, wp, stats, drec, grads, ws),
              8.0 * B * F * D, 5.0 * hidden)]
    res = []
    for name, fn, nbytes, flops in cases:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        res.append((name, statistics.median(timed(fn, iters) for _ in range(5)), nbytes, flops))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_afm.py measures on the GPU only")
    dev = torch.device("cuda:0")
    layers.set_default_device(dev)
    result = {}
    for shape in SHAPES:
        B, F, D, A = shape
        torch.manual_seed(0)
        att = torch.nn.Sequential(layers.FxLinear(D, A), torch.nn.ReLU(), layers.FxLinear(A, 1, bias=False),
                                  torch.nn.Softmax(dim=1)).to(dev)
        proj = layers.FxLinear(D, 1, bias=False).to(dev)
        product = layers.InnerProductInteraction(F, output="elementwise_product").to(dev)
        params = list(att.parameters()) + list(proj.parameters())
        x = torch.randn(B, F, D, device=dev, requires_grad=True)
        add = torch.randn(B, 1, device=dev)
        g = torch.randn(B, 1, device=dev)

        def module_by_module():
            e = product(x)
            return proj(torch.sum(att(e) * e, dim=1)) + add
        variants = {"module_by_module": module_by_module,
                    "fused": lambda: layers.afm_attention(x, att, proj, addend=add)}

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
        key = "B%d_F%d_D%d_A%d" % shape
        med = {k: statistics.median(v) for k, v in runs.items()}
        result[key] = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in runs.items()}
        result[key]["max_rel_fused_minus_module_by_module"] = agree
        for k in runs:
            print("%-24s %-17s median %9.1f us  min %9.1f  max %9.1f" % (key, k, med[k], min(runs[k]), max(runs[k])))
        print("%-24s module by module / fused, forward + backward: %.2f; max |fused - module by module| / max|.| %.2e"
              % (key, med["module_by_module"] / med["fused"], agree))
        for name, us, nbytes, flops in kernel_rates(shape, att, proj, dev, args.iters):
            bw, rate = nbytes / (us * 1e-6), flops / (us * 1e-6)
            kkey = "%s_kernel_%s" % (key, name)
            result[kkey] = {"median_us": us, "bytes": nbytes, "GBps": bw * 1e-9, "fraction_of_hbm_peak": bw / HBM_PEAK,
                            "flops": flops, "TFLOPps": rate * 1e-12, "fraction_of_f32_peak": rate / F32_PEAK}
            print("%-40s %9.1f us: %.1f MB = %.0f GB/s = %.2f %% of the HBM peak; %.2f GFLOP = %.2f TFLOP/s = %.1f %% "
                  "of the fp32 vector peak" % (kkey, us, nbytes / 1e6, bw * 1e-9, 100 * bw / HBM_PEAK, flops * 1e-9,
                                               rate * 1e-12, 100 * rate / F32_PEAK))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
