"""A/B of DESTINE's native disentangled self-attention layer (csrc/fx_dsa.hip: one launch forward, two backward)
against the same layer composed from torch ops in fp32 on the same GPU in the same run
(model_zoo/DESTINE/src/DESTINE.py:190-227, the reference's own sequence of ops on the native layer's parameters).
B 4096, H 2, each_layer residual, at F 39, D = A = 16 (Criteo) and at F 24, D = A = 40 (the reference's default).

    python scripts/bench_destine.py [--batch 4096] [--iters 50]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up; five rounds that alternate
the two sides, median and spread reported.  The forward's HBM floor is X in + Y out over the peak bandwidth.
Prints a table for profiles/destine_ab.txt."""
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


def torch_layer(x, layer):
    """layers.DisentangledSelfAttention's parameters, the reference's ops"""
    B, H, hd = x.shape[0], layer.num_heads, layer.head_dim
    unary = layer.W_unary(x)
    q, k, v = layer.W_q(x), layer.W_k(x), layer.W_v(x)
    if layer.relu_before_att:
        q, k, v = q.relu(), k.relu(), v.relu()
    q, k, v = q.view(B * H, -1, hd), k.view(B * H, -1, hd), v.view(B * H, -1, hd)
    pair = torch.bmm(q - q.mean(dim=1, keepdim=True), (k - k.mean(dim=1, keepdim=True)).transpose(1, 2))
    if layer.use_scale:
        pair = pair / hd ** 0.5
    un = torch.softmax(unary, dim=1).view(B * H, -1, 1).transpose(1, 2)
    out = torch.bmm(torch.softmax(pair, dim=2) + un, v).view(B, -1, layer.attention_dim)
    return out + layer.W_res(x) if layer.W_res is not None else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, H = a.batch, 2
    for F, D in ((39, 16), (24, 40)):
        torch.manual_seed(0)
        layer = layers.DisentangledSelfAttention(D, D, H, dropout_rate=0, use_scale=True).to(dev)
        x = torch.randn(B, F, D, device=dev).requires_grad_(True)
        gy = torch.randn(B, F, D, device=dev)
        params = list(layer.parameters())

        def native_fwd():
            with torch.no_grad():
                return layer(x, x, x)

        def native_both():
            return torch.autograd.grad(layer(x, x, x), [x] + params, gy)

        def torch_fwd():
            with torch.no_grad():
                return torch_layer(x, layer)

        def torch_both():
            return torch.autograd.grad(torch_layer(x, layer), [x] + params, gy)
        err = float((native_fwd() - torch_fwd()).abs().max())
        gerr = max(float((g - t).abs().max()) for g, t in zip(native_both(), torch_both()))
        print("B %d F %d D = A %d H %d   max |native - torch| Y %.2e, gradients %.2e   %d timed calls x 5 rounds"
              % (B, F, D, H, err, gerr, a.iters))
        names = ["native forward (1 launch)", "torch forward", "native forward + backward",
                 "torch forward + backward"]
        rows = dict(zip(names, timed([native_fwd, torch_fwd, native_both, torch_both], a.iters)))
        for name in names:
            print("%-32s median %9.1f us   min %9.1f   max %9.1f" % ((name,) + rows[name]))
        t = dict((k, v[0]) for k, v in rows.items())
        floor = 1e6 * 4.0 * B * F * 2 * D / HBM_PEAK
        print("speed-up forward %.2f x, forward + backward %.2f x;  forward HBM floor (X in, Y out at %.1f TB/s) "
              "%.2f us: %.1f %% of it achieved" % (
                  t[names[1]] / t[names[0]], t[names[3]] / t[names[2]], HBM_PEAK / 1e12, floor,
                  100.0 * floor / t[names[0]]))


if __name__ == "__main__":
    main()
