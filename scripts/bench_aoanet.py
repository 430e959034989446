"""A/B of AOANet's native interaction stack (layers.GeneralizedInteractionNet on csrc/fx_gin.hip) alone against torch on
the same GPU in the same run, at B 4096, F 39, num_subspaces 4, 3 layers, D 16 and 40.  Two opponents:
  reference  : the reference's own sequence of ops (model_zoo/AOANet/src/AOANet.py:165-170), which forms
               outer_product [B, S F, D, D] (6.4 GB at D 16, 40 GB at D 40, several times that with what autograd
               keeps).  Timed only where four such tensors fit in the free device memory; otherwise the table says so
               and the factorised formula is the opponent;
  factorised : the same layer without that tensor in torch ops (layers.generalized_interaction_composition: what
               fused=False runs).

    python scripts/bench_aoanet.py [--batch 4096] [--iters 20]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up; five rounds that alternate
the sides, median and spread reported.  The HBM floor of the native stack is B_0 read once and every layer's output
written once, the same again for the backward, over the peak bandwidth.  Prints a table for profiles/aoanet_ab.txt."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_eulernet import HBM_PEAK, timed  # noqa: E402
from fuxictr_amd import layers  # noqa: E402


def reference_layer(layer, B_0, B_i):
    outer = torch.einsum("bnh,bnd->bnhd", B_0.repeat(1, layer.input_subspaces, 1),
                         B_i.repeat(1, 1, layer.num_fields).view(B_i.size(0), -1, layer.embedding_dim))
    fusion = layer.W * torch.matmul(outer.permute(0, 2, 3, 1), layer.alpha).permute(0, 3, 1, 2)
    return torch.matmul(fusion, layer.h).squeeze(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F, O, L = a.batch, 39, 4, 3
    for D in (16, 40):
        torch.manual_seed(0)
        net = layers.GeneralizedInteractionNet(L, O, F, D).to(dev)
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.1 * torch.randn_like(p))
        X = (0.3 * torch.randn(B, F, D, device=dev)).requires_grad_(True)
        g = torch.randn(B, O, D, device=dev)
        leaves = [X] + list(net.parameters())

        def stack(one_layer):
            B_i = X
            for layer in net.layers:
                B_i = one_layer(layer, X, B_i)
            return B_i

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def both(fn):
            return lambda: torch.autograd.grad(fn(), leaves, g)
        sides = [("native", lambda: net(X)),
                 ("factorised torch", lambda: stack(lambda layer, B_0, B_i: layer(B_0, B_i)))]
        outer_bytes = 4.0 * B * F * F * D * D
        free = torch.cuda.mem_get_info(dev)[0]
        if 4.0 * outer_bytes < free:
            sides.append(("reference torch", lambda: stack(reference_layer)))
            iters = a.iters if outer_bytes < 8e9 else max(2, a.iters // 5)
            note = "%d timed calls x 5 rounds" % iters
        else:
            iters = a.iters
            note = ("the reference's ops NOT timed: outer_product is %.1f GB, four of them do not fit in the %.0f GB free; "
                    "the factorised formula is the opponent; %d timed calls x 5 rounds" % (outer_bytes / 1e9, free / 1e9, iters))
        want, wantg = fwd(sides[-1][1])(), both(sides[-1][1])()
        err = float((fwd(sides[0][1])() - want).abs().max() / want.abs().max())
        gerr = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(both(sides[0][1])(), wantg))
        del want, wantg
        print("GIN stack B %d F %d O %d L %d D %d   max |native - %s| / max: out %.2e, gradients %.2e   %s"
              % (B, F, O, L, D, sides[-1][0], err, gerr, note))
        fns = [w(fn) for _, fn in sides for w in (fwd, both)]
        names = ["%s %s" % (n, k) for n, _ in sides for k in ("forward", "forward + backward")]
        rows = dict(zip(names, timed(fns, iters)))
        for name in names:
            print("%-40s median %10.1f us   min %10.1f   max %10.1f" % ((name,) + rows[name]))
        t = dict((k, v[0]) for k, v in rows.items())
        for n, _ in sides[1:]:
            print("speed-up against %s: forward %.2f x, forward + backward %.2f x"
                  % (n, t[n + " forward"] / t["native forward"],
                     t[n + " forward + backward"] / t["native forward + backward"]))
        floor = 1e6 * 4.0 * B * (F * D + L * O * D) / HBM_PEAK
        for k, mult in (("forward", 1.0), ("forward + backward", 2.0)):
            share = mult * floor / t["native " + k]
            print("%s HBM floor (B_0 in, %d layer outputs out%s at %.1f TB/s) %.2f us: %.1f %% of it achieved (%s-bound as built)"
                  % (k, L, ", the same again backward" if mult > 1 else "", HBM_PEAK / 1e12, mult * floor, 100.0 * share,
                     "memory" if share > 0.5 else "compute / latency"))


if __name__ == "__main__":
    main()
