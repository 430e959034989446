"""A/B of SAM's native block (layers.SAMBlock on csrc/fx_sam.hip) against the same arithmetic as the reference's sequence
of torch ops in fp32 on the same GPU in the same run (model_zoo/SAM/src/SAM.py:150-275; torch forms the [B, F, F, D]
tensor).  All four interaction types at B 4096, F 39, D 16 and 40: SAM2A / SAM2E with the final Linear(F F D, 1) folded
in, SAM3A / SAM3E as 3 layers with the residual, concat and Linear(F D, 1).

    python scripts/bench_sam.py [--batch 4096] [--iters 20]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up; five rounds that alternate
the two sides, median and spread reported.  For SAM2A / SAM2E the forward's HBM floor is X read once and logit written
once, over the peak bandwidth.  Prints a table for profiles/sam_ab.txt."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_eulernet import HBM_PEAK, timed  # noqa: E402
from fuxictr_amd import layers  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F = a.batch, 39
    for D in (16, 40):
        for kind in ("SAM2A", "SAM2E", "SAM3A", "SAM3E"):
            torch.manual_seed(0)
            two = kind in ("SAM2A", "SAM2E")
            block = layers.SAMBlock(3, F, D, True, kind, "concat", 0).to(dev)
            fc = layers.FxLinear(F * D * (F if two else 1), 1).to(dev)
            with torch.no_grad():
                for n, p in block.named_parameters():
                    if n.endswith("W"):
                        p.add_(0.1 * torch.randn_like(p))
            X = (0.3 * torch.randn(B, F, D, device=dev)).requires_grad_(True)
            g = torch.randn(B, 1, device=dev)
            leaves = [X, fc.weight, fc.bias] + list(block.parameters())

            def torch_logit():
                h = X
                for layer in block.layers:
                    S = torch.bmm(h, (layer.K(h) if not two else h).transpose(1, 2))
                    out = S.unsqueeze(-1) * (layer.W if kind[-1] == "A" else torch.einsum("bnd,bmd->bnmd", h, h))
                    h = out if two else out.sum(dim=2) + layer.Q(h)
                return torch.nn.functional.linear(h.flatten(start_dim=1), fc.weight, fc.bias)

            def native_fwd():
                with torch.no_grad():
                    return block.logit(X, fc)

            def native_both():
                return torch.autograd.grad(block.logit(X, fc), leaves, g)

            def torch_fwd():
                with torch.no_grad():
                    return torch_logit()

            def torch_both():
                return torch.autograd.grad(torch_logit(), leaves, g)
            yn, yt = native_fwd(), torch_fwd()
            err = float((yn - yt).abs().max() / yt.abs().max())
            gerr = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(native_both(), torch_both()))
            print("%s%s B %d F %d D %d   max |native - torch| / max |torch|: logit %.2e, gradients %.2e   %d timed calls "
                  "x 5 rounds" % (kind, "" if two else " x 3 layers, residual", B, F, D, err, gerr, a.iters))
            names = ["native forward", "torch forward", "native forward + backward", "torch forward + backward"]
            rows = dict(zip(names, timed([native_fwd, torch_fwd, native_both, torch_both], a.iters)))
            for name in names:
                print("%-32s median %9.1f us   min %9.1f   max %9.1f" % ((name,) + rows[name]))
            t = dict((k, v[0]) for k, v in rows.items())
            print("speed-up forward %.2f x, forward + backward %.2f x" % (t[names[1]] / t[names[0]],
                                                                         t[names[3]] / t[names[2]]))
            if two:
                floor = 1e6 * 4.0 * B * (F * D + 1) / HBM_PEAK
                print("forward HBM floor (X in, logit out at %.1f TB/s) %.2f us: %.1f %% of it achieved (%s-bound as built)"
                      % (HBM_PEAK / 1e12, floor, 100.0 * floor / t[names[0]],
                         "memory" if floor / t[names[0]] > 0.5 else "compute / latency"))


if __name__ == "__main__":
    main()
