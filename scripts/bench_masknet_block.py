"""A/B of MaskNet's building blocks, forward and forward + backward, one process, one GPU:
  baseline  the same composition from stock torch-ROCm ops (nn.LayerNorm per field and their cat, F.linear, relu,
            `*`, nn.LayerNorm) on the same tensors — what a user without the native layers runs;
  native    layers.FieldLayerNorm (one grouped launch of csrc/fx_layernorm.hip over the record) and
            layers.mask_stage (_MaskStageFn: the mask product in a GEMM epilogue, LayerNorm + ReLU in one launch,
            blocks side by side without a cat).
Three stages — `emb_norm`, one serial block (width -> width), a 3-block parallel stage (F D -> 3 x width) — at
(B 4096, F 39, D 16, width 256) and (B 10000, F 24, D 40, width 512).  Device events around `--iters` iterations
after warm-up, the two variants alternated, `--repeats` repeats each; prints median and min-max per variant, and
for the LayerNorm kernels alone the bytes they must move (ops' own counts: x and y once, the backward's second pass
over x and dY) over their time, next to the HBM peak (8 TB/s spec, 6.3 TB/s achievable by a copy); then one JSON
line.
    python scripts/bench_masknet_block.py [--iters 50] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn
from torch.nn import functional as tF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuxictr_amd import layers, ops  # noqa: E402

#          B     F   D  width
CONFIGS = [(4096, 39, 16, 256), (10000, 24, 40, 512)]
HBM_PEAK = 8.0e12      # bytes / s, MI355X (spec); a float4 copy reaches 6.3e12


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per call


def block_torch(block, norm, v_emb, v_hid):
    """MaskBlock.forward of the reference on the block's own parameters with stock ops."""
    h = tF.relu(tF.linear(v_emb, block.mask_layer[0].weight, block.mask_layer[0].bias))
    v_mask = tF.linear(h, block.mask_layer[2].weight, block.mask_layer[2].bias)
    z = tF.linear(v_mask * v_hid, block.hidden_layer[0].weight)
    return tF.relu(tF.layer_norm(z, (z.shape[1],), norm.weight, norm.bias, norm.eps))


def make_stages(cfg, dev):
    B, F, D, width = cfg
    layers.set_default_device(dev)
    torch.manual_seed(0)
    emb = torch.randn(B, F, D, device=dev, requires_grad=True)
    flat = torch.randn(B, F * D, device=dev, requires_grad=True)
    hid = torch.randn(B, width, device=dev, requires_grad=True)
    fnorm = layers.FieldLayerNorm(F, D)
    tnorms = nn.ModuleList(nn.LayerNorm(D, device=dev) for _ in range(F))
    serial = layers.MaskBlock(F * D, width, width)
    parallel = [layers.MaskBlock(F * D, F * D, width) for _ in range(3)]
    for blk in [serial] + parallel:
        for lin in (blk.mask_layer[0], blk.mask_layer[2], blk.hidden_layer[0]):
            nn.init.xavier_normal_(lin.weight)
    stages = {
        "emb_norm": (lambda: fnorm(emb),
                     lambda: torch.cat([tnorms[i](emb[:, i, :]) for i in range(F)], dim=1),
                     torch.randn(B, F * D, device=dev)),
        "serial_block": (lambda: layers.mask_stage([serial], flat, hid),
                         lambda: block_torch(serial, serial.hidden_layer[1], flat, hid),
                         torch.randn(B, width, device=dev)),
        "parallel_3_blocks": (lambda: layers.mask_stage(parallel, flat, flat),
                              lambda: torch.cat([block_torch(b, b.hidden_layer[1], flat, flat) for b in parallel],
                                                dim=-1),
                              torch.randn(B, 3 * width, device=dev)),
    }
    leaves = [emb, flat, hid] + list(fnorm.parameters()) + list(tnorms.parameters()) + \
        [p for b in [serial] + parallel for p in b.parameters()]
    return stages, leaves


def kernel_rates(cfg, dev, iters):
    """The LayerNorm launches alone: (name, us, bytes) for emb_norm's shape and the block's."""
    B, F, D, width = cfg
    out = []
    for name, (G, N, relu) in (("emb_norm", (F, D, False)), ("block_ln_relu", (1, width, True))):
        x = torch.randn(B, G * N, device=dev)
        ga, be = torch.ones(G * N, device=dev), torch.zeros(G * N, device=dev)
        y, dy, dx = torch.empty_like(x), torch.randn_like(x), torch.empty_like(x)
        stats = torch.empty(B * G * 2, device=dev)
        dga, dbe = torch.empty_like(ga), torch.empty_like(be)
        ws = torch.empty(ops.layernorm_workspace_floats(B, G, N), device=dev)

        def fwd():
            ops.layernorm_fwd(x, G, N, ga, be, 1e-5, relu, y, stats)

        def bwd():
            ops.layernorm_bwd(x, G, N, ga, relu, y, stats, dy, dx, dga, dbe, ws)
        for _ in range(5):
            fwd(), bwd()
        torch.cuda.synchronize()
        fb = 4.0 * (2.0 * B * G * N + 2.0 * G * N + 2.0 * B * G)
        bb = 4.0 * B * G * N * (5.0 + (2.0 if relu else 0.0))
        out.append((name + "_fwd", statistics.median(timed(fwd, iters) for _ in range(5)), fb))
        out.append((name + "_bwd", statistics.median(timed(bwd, iters) for _ in range(5)), bb))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_masknet_block.py measures on the GPU only")
    dev = torch.device("cuda:0")
    result = {}
    for cfg in CONFIGS:
        stages, leaves = make_stages(cfg, dev)
        for stage, (native, baseline, g) in stages.items():
            def step(fwd):
                for t in leaves:
                    t.grad = None
                fwd().backward(g)
            with torch.no_grad():
                a, b = native(), baseline()
            agree = float((a - b).abs().max())
            for _ in range(args.warmup):
                step(native), step(baseline)
            torch.cuda.synchronize()
            runs = {"baseline_fwd": [], "native_fwd": [], "baseline_fwd_bwd": [], "native_fwd_bwd": []}
            for _ in range(args.repeats):                  # alternated
                with torch.no_grad():
                    runs["baseline_fwd"].append(timed(baseline, args.iters))
                    runs["native_fwd"].append(timed(native, args.iters))
                runs["baseline_fwd_bwd"].append(timed(lambda: step(baseline), args.iters))
                runs["native_fwd_bwd"].append(timed(lambda: step(native), args.iters))
            key = "B%d_F%d_D%d_w%d_%s" % (cfg + (stage,))
            med = {k: statistics.median(v) for k, v in runs.items()}
            result[key] = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in runs.items()}
            result[key]["max_abs_native_minus_baseline"] = agree
            for k in runs:
                print("%-44s %-17s median %9.1f us  min %9.1f  max %9.1f" % (key, k, med[k], min(runs[k]),
                                                                             max(runs[k])))
            print("%-44s baseline / native: forward %.2f, forward + backward %.2f; max |native - baseline| %.2e"
                  % (key, med["baseline_fwd"] / med["native_fwd"], med["baseline_fwd_bwd"] / med["native_fwd_bwd"],
                     agree))
        for name, us, nbytes in kernel_rates(cfg, dev, args.iters):
            bw = nbytes / (us * 1e-6)
            key = "B%d_F%d_D%d_w%d_kernel_%s" % (cfg + (name,))
            result[key] = {"median_us": us, "bytes": nbytes, "GBps": bw * 1e-9, "fraction_of_hbm_peak": bw / HBM_PEAK}
            print("%-44s %8.1f us for %.1f MB = %.0f GB/s = %.1f %% of the HBM peak"
                  % (key, us, nbytes / 1e6, bw * 1e-9, 100 * bw / HBM_PEAK))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
