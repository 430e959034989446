"""A/B of FiGNN's native graph propagation (csrc/fx_fignn.hip: the attentional graph and all layers in one launch per
direction) against the same mathematics composed from torch ops in fp32 on the same GPU in the same run
(model_zoo/FiGNN/src/FiGNN.py:128-203 restated without the [F^2, 2 D] concat, so the torch side is not charged for
it).  B 4096, F 39, 3 layers, GRU and residual, at D 16 and at D 40.

    python scripts/bench_fignn.py [--batch 4096] [--iters 50]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up, five rounds, median and
spread reported.  Prints a table for profiles/fignn_ab.txt."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fuxictr_amd import layers  # noqa: E402


def timed(fn, iters, rounds=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def torch_layer(x, layer):
    """layers.FiGNN_Layer's parameters, torch's ops"""
    B, F, D = x.shape
    w = layer.W_attn.weight.reshape(-1)
    pre = (x @ w[:D]).unsqueeze(2) + (x @ w[D:]).unsqueeze(1)
    alpha = torch.nn.functional.leaky_relu(pre, 0.01)
    alpha = alpha.masked_fill(torch.eye(F, dtype=torch.bool, device=x.device), float("-inf"))
    g = torch.softmax(alpha, dim=-1)
    h = x
    for m in layer.gnn:
        o = torch.matmul(m.W_out, h.unsqueeze(-1)).squeeze(-1)
        a = torch.matmul(m.W_in, torch.bmm(g, o).unsqueeze(-1)).squeeze(-1) + m.bias_p
        gi = a @ layer.gru.weight_ih.t() + layer.gru.bias_ih
        gh = h @ layer.gru.weight_hh.t() + layer.gru.bias_hh
        r = torch.sigmoid(gi[..., :D] + gh[..., :D])
        z = torch.sigmoid(gi[..., D:2 * D] + gh[..., D:2 * D])
        n = torch.tanh(gi[..., 2 * D:] + r * gh[..., 2 * D:])
        h = (1 - z) * n + z * h + x
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F, L = a.batch, 39, 3
    for D in (16, 40):
        torch.manual_seed(0)
        layer = layers.FiGNN_Layer(F, D, gnn_layers=L).to(dev)
        with torch.no_grad():
            layer.W_attn.weight.normal_(0, (2 * D) ** -0.5)
        x = (torch.randn(B, F, D, device=dev) * 0.5).requires_grad_(True)
        gy = torch.randn(B, F, D, device=dev)
        params = list(layer.parameters())

        def native_fwd():
            with torch.no_grad():
                return layer(x)

        def native_both():
            torch.autograd.grad(layer(x), [x] + params, gy)

        def torch_fwd():
            with torch.no_grad():
                return torch_layer(x, layer)

        def torch_both():
            torch.autograd.grad(torch_layer(x, layer), [x] + params, gy)
        err = float((native_fwd() - torch_fwd()).abs().max())
        print("B %d F %d D %d layers %d   max |native - torch| h_out %.2e   %d timed calls x 5 rounds"
              % (B, F, D, L, err, a.iters))
        rows = [("native forward (1 launch)", timed(native_fwd, a.iters)),
                ("native forward + backward", timed(native_both, a.iters)),
                ("torch forward", timed(torch_fwd, a.iters)),
                ("torch forward + backward", timed(torch_both, a.iters))]
        for name, (med, lo, hi) in rows:
            print("%-32s median %9.1f us   min %9.1f   max %9.1f" % (name, med, lo, hi))
        t = dict((k, v[0]) for k, v in rows)
        print("speed-up forward %.2f x, forward + backward %.2f x" % (
            t["torch forward"] / t["native forward (1 launch)"],
            t["torch forward + backward"] / t["native forward + backward"]))


if __name__ == "__main__":
    main()
