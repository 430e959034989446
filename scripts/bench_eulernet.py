"""A/B of EulerNet's native Euler interaction layer (layers.EulerInteractionLayer on csrc/fx_euler.hip: the dense GEMM
over 2 B rows + k_eu_fwd forward; k_eu_bwd, k_eu_bwd_dw, the fixed-order reduces and the dense path's two products in one
GEMM launch backward) against the reference's own sequence of torch ops in fp32 on the same GPU in the same run
(model_zoo/EulerNet/src/EulerNet.py:139-170, on the same parameters).  B 4096, F 39, D 10 and 16, shape [20] and [52],
layer_norm on and off.

    python scripts/bench_eulernet.py [--batch 4096] [--iters 20]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up; five rounds that alternate
the two sides, median and spread reported.  The forward's HBM floor is RP and Z read once and OP written once, over the
peak bandwidth.  Prints a table for profiles/eulernet_ab.txt."""
import argparse
import os
import statistics
import sys

import torch

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F = a.batch, 39
    for D in (10, 16):
        for O in (20, 52):
            for ln in (True, False):
                torch.manual_seed(0)
                layer = layers.EulerInteractionLayer(F * D, O * D, D, ln, 0, 0).to(dev)
                RP = torch.randn(2, B, F, D, device=dev).requires_grad_(True)
                g = torch.randn(2, B, O, D, device=dev)
                params = list(layer.parameters()) if ln else [p for n, p in layer.named_parameters() if "norm" not in n]

                def native_fwd():
                    with torch.no_grad():
                        return layer(RP)

                def native_both():
                    return torch.autograd.grad(layer(RP), [RP] + params, g)

                def torch_fwd():
                    with torch.no_grad():
                        return torch.stack(layer._reference(RP[0], RP[1]))

                def torch_both():
                    return torch.autograd.grad(torch.stack(layer._reference(RP[0], RP[1])), [RP] + params, g)
                yn, yt = native_fwd(), torch_fwd()
                err = float((yn - yt).abs().max() / yt.abs().max())
                gerr = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(native_both(), torch_both()))
                print("B %d F %d D %d O %d layer_norm %s   max |native - torch| / max |torch|: OP %.2e, gradients %.2e"
                      "   %d timed calls x 5 rounds" % (B, F, D, O, ln, err, gerr, a.iters))
                names = ["native forward (2 launches)", "torch forward", "native forward + backward",
                         "torch forward + backward"]
                rows = dict(zip(names, timed([native_fwd, torch_fwd, native_both, torch_both], a.iters)))
                for name in names:
                    print("%-32s median %9.1f us   min %9.1f   max %9.1f" % ((name,) + rows[name]))
                t = dict((k, v[0]) for k, v in rows.items())
                floor = 1e6 * 4.0 * 2 * B * D * (F + 2 * O) / HBM_PEAK
                print("speed-up forward %.2f x, forward + backward %.2f x;  forward HBM floor (RP and Z in, OP out at "
                      "%.1f TB/s) %.2f us: %.1f %% of it achieved" % (
                          t[names[1]] / t[names[0]], t[names[3]] / t[names[2]], HBM_PEAK / 1e12, floor,
                          100.0 * floor / t[names[0]]))


if __name__ == "__main__":
    main()
