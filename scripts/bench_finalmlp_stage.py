"""A/B of FinalMLP's two non-tower stages and of the whole model, forward + backward, one process, one GPU:
  baseline  the same formulas from stock torch-ROCm ops on the same tensors, as the reference composes them (the
            gate towers on B rows, `repeat` of the context bias included, sigmoid, `* 2`, `*`; the head from two
            F.linear, two broadcast matmuls over reshaped views, a sum and an add);
  native    layers.FeatureSelection (the towers' Linear / ReLU prefix on the GEMM dispatcher, on one bias row when
            there are no context features, both gates in one launch of csrc/fx_finalmlp.hip) and
            layers.InteractionAggregation (per-head products through gemm_batch, one pass per sample).
Shapes: the reference's FinalMLP_default on Criteo (39 fields, D 16: W 624; towers [1024, 512] / [1024, 512, 256];
gate towers [1024, 512]; heads 1, 2, 4) at B 4096 and B 10000.  With context features the gates read one / two
fields' embeddings per sample.  Then the whole zoo.FinalMLP training step, fused against module by module.
Device events around `--iters` iterations after warm-up, the two variants alternated, `--repeats` repeats each;
prints median and min-max per variant, and for the four kernels alone the bytes they must move (ops' own counts)
over their time, next to the HBM peak (8 TB/s spec, 6.3 TB/s achievable by a copy); then one JSON line.
    python scripts/bench_finalmlp_stage.py [--iters 30] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch
from torch import nn
from torch.nn import functional as tF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuxictr_amd import layers, ops, synthetic, zoo  # noqa: E402

BATCHES = [4096, 10000]
D, X_DIM, Y_DIM, FS_HIDDEN = 16, 512, 256, [1024, 512]
HBM_PEAK = 8.0e12      # bytes / s, MI355X (spec); a float4 copy reaches 6.3e12


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per call


class _Fixed(nn.Module):
    """Stands where a gate's context FeatureEmbedding stands: the looked-up [B, n, D] embeddings, already there."""

    def __init__(self, t):
        super(_Fixed, self).__init__()
        self.t = t

    def forward(self, X):
        return self.t


def gates_torch(fs, flat_emb):
    feats = []
    for n, ctx in ((1, fs.fs1_context), (2, fs.fs2_context)):
        if len(ctx) == 0:
            h = getattr(fs, "fs%d_ctx_bias" % n).repeat(flat_emb.size(0), 1)
        else:
            h = getattr(fs, "fs%d_ctx_emb" % n)(None).flatten(start_dim=1)
        lins = [m for m in getattr(fs, "fs%d_gate" % n).mlp if isinstance(m, nn.Linear)]
        for i, lin in enumerate(lins):
            h = tF.linear(h, lin.weight, lin.bias)
            h = tF.relu(h) if i < len(lins) - 1 else torch.sigmoid(h)
        feats.append(flat_emb * (h * 2))
    return feats


def head_torch(agg, x, y):
    H, dxh, dyh = agg.num_heads, agg.head_x_dim, agg.head_y_dim
    output = tF.linear(x, agg.w_x.weight, agg.w_x.bias) + tF.linear(y, agg.w_y.weight, agg.w_y.bias)
    head_x, head_y = x.view(-1, H, dxh), y.view(-1, H, dyh)
    xy = torch.matmul(torch.matmul(head_x.unsqueeze(2), agg.w_xy.view(H, dxh, -1)).view(-1, H, 1, dyh),
                      head_y.unsqueeze(-1)).squeeze(-1)
    output += xy.sum(dim=1)
    return output


def make_stages(B, fmap, dev):
    layers.set_default_device(dev)
    torch.manual_seed(0)
    W = fmap.num_fields * D
    emb = torch.randn(B, W, device=dev, requires_grad=True)
    x = torch.randn(B, X_DIM, device=dev, requires_grad=True)
    y = torch.randn(B, Y_DIM, device=dev, requires_grad=True)
    stages, leaves = {}, [emb, x, y]
    for name, (c1, c2) in (("gates_no_context", ([], [])), ("gates_context", (["C1"], ["C2", "C3"]))):
        fs = layers.FeatureSelection(fmap, W, D, FS_HIDDEN, c1, c2)
        for n, ctx in ((1, c1), (2, c2)):
            if ctx:
                t = torch.randn(B, len(ctx), D, device=dev, requires_grad=True)
                setattr(fs, "fs%d_ctx_emb" % n, _Fixed(t))
                leaves.append(t)
        with torch.no_grad():
            for k, p in fs.named_parameters():
                p.copy_(torch.randn(p.shape, device=dev) * (0.05 if p.dim() == 2 and p.shape[0] > 1 else 0.5))
        g = [torch.randn(B, W, device=dev), torch.randn(B, W, device=dev)]
        stages[name] = (lambda fs=fs: list(fs(None, emb)), lambda fs=fs: gates_torch(fs, emb), g)
        leaves += list(fs.parameters())
    for H in (1, 2, 4):
        agg = layers.InteractionAggregation(X_DIM, Y_DIM, output_dim=1, num_heads=H)
        nn.init.xavier_normal_(agg.w_x.weight), nn.init.xavier_normal_(agg.w_y.weight)
        stages["head_H%d" % H] = (lambda agg=agg: [agg(x, y)], lambda agg=agg: [head_torch(agg, x, y)],
                                  [torch.randn(B, 1, device=dev)])
        leaves += list(agg.parameters())
    return stages, leaves


def kernel_rates(B, W, dev, iters):
    """The four kernels alone: (name, us, bytes)."""
    out = []

    def rnd(*s):
        return torch.randn(*s, device=dev)
    for name, rows in (("gate2_broadcast", 1), ("gate2_per_sample", B)):
        E, Z1, Z2, F1, F2 = rnd(B, W), rnd(rows, W), rnd(rows, W), rnd(B, W), rnd(B, W)
        dE, dZ1, dZ2 = torch.empty_like(E), torch.empty_like(Z1), torch.empty_like(Z2)
        ws = torch.empty(ops.gate2_workspace_floats(B, W), device=dev)

        def fwd(t=(E, Z1, Z2, F1, F2)):
            ops.gate2_fwd(*t)

        def bwd(t=(F1, F2, E, Z1, Z2, dE, dZ1, dZ2, ws)):
            ops.gate2_bwd(*t)
        out.append((name + "_fwd", fwd, _bytes_gate_fwd(E, Z1, Z2)))
        out.append((name + "_bwd", bwd, _bytes_gate_bwd(E, Z1, Z2)))
    X, Y, T = rnd(B, X_DIM), rnd(B, Y_DIM), rnd(B, Y_DIM)
    wx, wy, bx, by, g, o = rnd(1, X_DIM), rnd(1, Y_DIM), rnd(1), rnd(1), rnd(B, 1), rnd(B, 1)
    dT, dY, dXr = torch.empty_like(T), torch.empty_like(Y), torch.empty_like(X)
    dwx, dwy, db = torch.empty_like(wx), torch.empty_like(wy), torch.empty(2, device=dev)
    ws = torch.empty(ops.biagg_workspace_floats(B, X_DIM, Y_DIM), device=dev)
    out.append(("biagg_fwd", lambda: ops.biagg_fwd(X, Y, T, wx, wy, bx, by, None, o),
                4.0 * B * (X_DIM + 2.0 * Y_DIM + 1.0)))
    out.append(("biagg_bwd", lambda: ops.biagg_bwd(g, X, Y, T, wx, wy, dT, dY, dXr, dwx, dwy, db, ws),
                4.0 * B * (2.0 * X_DIM + 4.0 * Y_DIM + 1.0)))
    res = []
    for name, fn, nbytes in out:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        res.append((name, statistics.median(timed(fn, iters) for _ in range(5)), nbytes))
    return res


def _bytes_gate_fwd(E, Z1, Z2):
    return 4.0 * (3.0 * E.numel() + Z1.numel() + Z2.numel())                   # E, F1, F2; Z


def _bytes_gate_bwd(E, Z1, Z2):
    per = 2.0 * (Z1.numel() + Z2.numel()) if Z1.shape[0] == E.shape[0] else 0.0    # Z read, dZ written
    return 4.0 * (4.0 * E.numel() + per)                                       # E, dE, dF1, dF2


def model_step(B, fmap_args, fused, dev, iters, repeats, tmp):
    fmap, _ = synthetic.criteo_feature_map(**fmap_args)
    torch.manual_seed(0)
    model = zoo.FinalMLP(fmap, model_id="finalmlp_bench", gpu=0, embedding_dim=D, mlp1_hidden_units=[1024, 512],
                         mlp2_hidden_units=[1024, 512, 256], fs_hidden_units=FS_HIDDEN, num_heads=2,
                         optimizer="adam", loss="binary_crossentropy", learning_rate=1e-3,
                         task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=tmp,
                         sparse_update="exact", fused=fused)
    rng = np.random.default_rng(0)
    b = synthetic.criteo_batch(rng, B, cards=fmap_args["cards"])
    b["label"] = (b["I1"] + b["I2"] > 1.0).astype(np.float32)
    batch = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    model.train()
    for _ in range(5):
        model.train_step(batch)
    torch.cuda.synchronize()
    return [timed(lambda: model.train_step(batch), iters) for _ in range(repeats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finalmlp_stage.py measures on the GPU only")
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="fx_bench_finalmlp_")
    cards = [max(2, int(c * 0.01)) for c in synthetic.CRITEO_CARDS]
    fmap_args = dict(cards=cards, embedding_dim=D)
    result = {}
    for B in BATCHES:
        fmap, _ = synthetic.criteo_feature_map(**fmap_args)
        stages, leaves = make_stages(B, fmap, dev)
        for stage, (native, baseline, g) in stages.items():
            def step(fwd):
                for t in leaves:
                    t.grad = None
                torch.autograd.backward(fwd(), g)
            with torch.no_grad():
                agree = max(float((a - b).abs().max()) for a, b in zip(native(), baseline()))
            for _ in range(args.warmup):
                step(native), step(baseline)
            torch.cuda.synchronize()
            runs = {"baseline_fwd_bwd": [], "native_fwd_bwd": []}
            for _ in range(args.repeats):                  # alternated
                runs["baseline_fwd_bwd"].append(timed(lambda: step(baseline), args.iters))
                runs["native_fwd_bwd"].append(timed(lambda: step(native), args.iters))
            key = "B%d_%s" % (B, stage)
            med = {k: statistics.median(v) for k, v in runs.items()}
            result[key] = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in runs.items()}
            result[key]["max_abs_native_minus_baseline"] = agree
            for k in runs:
                print("%-28s %-17s median %9.1f us  min %9.1f  max %9.1f" % (key, k, med[k], min(runs[k]),
                                                                             max(runs[k])))
            print("%-28s baseline / native, forward + backward: %.2f; max |native - baseline| %.2e"
                  % (key, med["baseline_fwd_bwd"] / med["native_fwd_bwd"], agree))
        for name, us, nbytes in kernel_rates(B, fmap.num_fields * D, dev, args.iters):
            bw = nbytes / (us * 1e-6)
            key = "B%d_kernel_%s" % (B, name)
            result[key] = {"median_us": us, "bytes": nbytes, "GBps": bw * 1e-9, "fraction_of_hbm_peak": bw / HBM_PEAK}
            print("%-36s %8.1f us for %.1f MB = %.0f GB/s = %.1f %% of the HBM peak"
                  % (key, us, nbytes / 1e6, bw * 1e-9, 100 * bw / HBM_PEAK))
        steps = {}
        for fused in (True, False):
            steps[fused] = model_step(B, fmap_args, fused, dev, max(5, args.iters // 3), args.repeats, tmp)
        key = "B%d_model_step" % B
        result[key] = {("fused" if f else "module_by_module"): {"median_us": statistics.median(v), "min_us": min(v),
                                                                "max_us": max(v)} for f, v in steps.items()}
        print("%-28s fused median %9.1f us, module by module %9.1f us: %.2f x" % (
            key, statistics.median(steps[True]), statistics.median(steps[False]),
            statistics.median(steps[False]) / statistics.median(steps[True])))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
