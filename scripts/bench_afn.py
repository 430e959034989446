"""A/B of AFN's native logarithmic transformation layer (csrc/fx_lognet.hip: five launches forward in training, eight
backward, exp(.) [B, L, D] never in memory) against the same layer composed from torch ops in fp32 on the same GPU in
the same run (model_zoo/AFN/src/AFN.py:121-138, the reference's own sequence of ops on the same parameters and
BatchNorm1d modules, training mode).  B 4096, F 39, at D 16 and 20 and L 24 and 1200 (the reference's tuned config).

    python scripts/bench_afn.py [--batch 4096] [--iters 20]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up; five rounds that alternate
the two sides, median and spread reported.  The forward's HBM floor is Y written once plus x read, over the peak
bandwidth.  Prints a table for profiles/afn_lognet_ab.txt."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fuxictr_amd import layers  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s, MI355X (HBM3E)


def timed(fns, iters, rounds=5):
    """-> per function (median, min, max) in us; the functions take turns inside every round"""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(1e3 * e0.elapsed_time(e1) / iters)
    return [(statistics.median(t), min(t), max(t)) for t in out]


def torch_layer(x, W, log_bn, exp_bn):
    """the reference's ops"""
    a = log_bn(torch.log(torch.clamp(torch.abs(x), min=1e-5)))
    return torch.flatten(exp_bn(torch.exp(W(a.transpose(2, 1)).transpose(1, 2))), start_dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F = a.batch, 39
    for D, L in ((16, 24), (16, 1200), (20, 24), (20, 1200)):
        torch.manual_seed(0)
        W = nn.Linear(F, L, bias=False).to(dev)
        nn.init.xavier_normal_(W.weight)
        log_bn, exp_bn = nn.BatchNorm1d(F).to(dev), nn.BatchNorm1d(L).to(dev)
        x = torch.randn(B, F, D, device=dev).requires_grad_(True)
        gy = torch.randn(B, L * D, device=dev)
        params = [W.weight, log_bn.weight, log_bn.bias, exp_bn.weight, exp_bn.bias]

        def native_fwd():
            with torch.no_grad():
                return layers.logarithmic_net(x, W, log_bn, exp_bn, True)

        def native_both():
            return torch.autograd.grad(layers.logarithmic_net(x, W, log_bn, exp_bn, True), [x] + params, gy)

        def torch_fwd():
            with torch.no_grad():
                return torch_layer(x, W, log_bn, exp_bn)

        def torch_both():
            return torch.autograd.grad(torch_layer(x, W, log_bn, exp_bn), [x] + params, gy)
        yn, yt = native_fwd(), torch_fwd()
        err = float((yn - yt).abs().max() / yt.abs().max())
        gerr = max(float((g - t).abs().max() / t.abs().max()) for g, t in list(zip(native_both(), torch_both()))[:2])
        print("B %d F %d D %d L %d   max |native - torch| / max |torch|: Y %.2e, dX and dW %.2e   %d timed calls x 5 "
              "rounds" % (B, F, D, L, err, gerr, a.iters))
        names = ["native forward (5 launches)", "torch forward", "native forward + backward",
                 "torch forward + backward"]
        rows = dict(zip(names, timed([native_fwd, torch_fwd, native_both, torch_both], a.iters)))
        for name in names:
            print("%-32s median %9.1f us   min %9.1f   max %9.1f" % ((name,) + rows[name]))
        t = dict((k, v[0]) for k, v in rows.items())
        floor = 1e6 * 4.0 * B * D * (L + F) / HBM_PEAK
        print("speed-up forward %.2f x, forward + backward %.2f x;  forward HBM floor (x in, Y out at %.1f TB/s) "
              "%.2f us: %.1f %% of it achieved" % (
                  t[names[1]] / t[names[0]], t[names[3]] / t[names[2]], HBM_PEAK / 1e12, floor,
                  100.0 * floor / t[names[0]]))


if __name__ == "__main__":
    main()
