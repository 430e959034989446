"""A/B of the native CrossNetMix (csrc/fx_crossmix.hip: the whole stack in one launch per direction, the weight
gradients through the project's GEMM) against the reference's composition (cross_net.py:158-201) in stock torch ops in
fp32, on the same GPU in the same process, the two routes alternating repeat by repeat.
(B, W, r, E, L) = (4096, 624, 32, 4, 3) and (4096, 1248, 32, 4, 3), forward alone and forward + backward.

    python scripts/bench_crossmix.py [--batch 4096] [--iters 30]

Before anything is timed both routes must agree on the same seeded inputs to the bound of
tests/test_gpu_crossmix_kernel.py (4 e32 + 1e-6 max|ref| against the composition in fp64, for the output and dX).
Each repeat times `iters` back-to-back calls between one pair of device events; five repeats, median, min and max.
Beside the table: the forward's floors from the shapes, flops over the fp32-MFMA peak and bytes (x_0 in, L activations
out) over the HBM bandwidth.  Prints the table of profiles/crossmix_ab.txt; exits non-zero without a GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fuxictr_amd import layers  # noqa: E402

MFMA_F32_FLOPS = 157.3e12        # MI355X, dense fp32 matrix peak
HBM_BYTES_PER_S = 8.0e12


def torch_layer(x, m):
    """layers.CrossNetMix's parameters, the reference's forward in torch's ops"""
    x0 = x.unsqueeze(2)
    xl = x0
    for i in range(m.layer_num):
        outs, scores = [], []
        for e in range(m.num_experts):
            scores.append(m.gating[e].weight.to(x.dtype) @ xl.squeeze(2).t())
            v = torch.tanh(torch.matmul(m.V_list[i][e].to(x.dtype).t(), xl))
            v = torch.tanh(torch.matmul(m.C_list[i][e].to(x.dtype), v))
            outs.append((x0 * (torch.matmul(m.U_list[i][e].to(x.dtype), v) + m.bias[i].to(x.dtype))).squeeze(2))
        gate = torch.stack([s.t() for s in scores], 1).softmax(1)
        xl = torch.matmul(torch.stack(outs, 2), gate) + xl
    return xl.squeeze(2)


def repeat(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_crossmix: no GPU")
    dev = torch.device("cuda", 0)
    B, r, E, L = a.batch, 32, 4, 3
    for W in (624, 1248):
        torch.manual_seed(0)
        m = layers.CrossNetMix(W, layer_num=L, low_rank=r, num_experts=E).to(dev)
        with torch.no_grad():
            for b in m.bias:
                b.normal_(0, 0.2)
        x = (torch.randn(B, W, device=dev) * 0.5).requires_grad_(True)
        gy = torch.randn(B, W, device=dev)
        params = list(m.parameters())
        routes = {"fused": lambda: m(x), "torch": lambda: torch_layer(x, m)}

        def fwd(route):
            def run():
                with torch.no_grad():
                    return routes[route]()
            return run

        def both(route):
            return lambda: torch.autograd.grad(routes[route](), [x] + params, gy)
        x64 = x.detach().double().requires_grad_(True)
        out64 = torch_layer(x64, m)
        ref = {"out": out64.detach(), "dX": torch.autograd.grad(out64, x64, gy.double())[0]}
        for name in ("out", "dX"):
            got = {k: (fwd(k)() if name == "out" else both(k)()[0]).double() for k in routes}
            e32 = float((got["torch"] - ref[name]).abs().max())
            bound = 4.0 * e32 + 1e-6 * float(ref[name].abs().max())
            err = float((got["fused"] - ref[name]).abs().max())
            print("B %d W %d r %d E %d L %d  %-3s |fused - fp64| %.2e  bound %.2e" % (B, W, r, E, L, name, err, bound))
            assert err <= bound, (name, err, bound)
        cases = [(k + " " + d, f(k)) for d, f in (("forward", fwd), ("forward + backward", both)) for k in routes]
        for _, fn in cases:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in cases}
        for _ in range(5):                       # the routes alternate inside every repeat
            for name, fn in cases:
                times[name].append(repeat(fn, a.iters))
        for name, _ in cases:
            t = times[name]
            print("%-32s median %9.1f us   min %9.1f   max %9.1f" % (name, statistics.median(t), min(t), max(t)))
        med = {k: statistics.median(v) for k, v in times.items()}
        print("speed-up forward %.2f x, forward + backward %.2f x" % (
            med["torch forward"] / med["fused forward"],
            med["torch forward + backward"] / med["fused forward + backward"]))
        flops = 2.0 * B * L * (W * (E * r + E) + E * r * r + E * r * W)
        floor_mfma, floor_bytes = 1e6 * flops / MFMA_F32_FLOPS, 1e6 * 4.0 * B * W * (1 + L) / HBM_BYTES_PER_S
        print("forward floors: MFMA %.1f us (%.2f GFLOP), bytes %.1f us; the fused forward runs at %.1f %% of the %s "
              "floor" % (floor_mfma, flops / 1e9, floor_bytes, 100.0 * max(floor_mfma, floor_bytes) / med["fused forward"],
                         "MFMA" if floor_mfma > floor_bytes else "byte"))


if __name__ == "__main__":
    main()
