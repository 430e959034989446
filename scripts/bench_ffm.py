"""A/B of the field-aware interaction (layers.field_aware_interaction on csrc/fx_ffm.hip) against the same arithmetic as
the reference's sequence of torch ops in fp32 on the same GPU in the same run (model_zoo/ONN/ONN_torch/src/ONNv2.py:88-109:
the masked_select of the own vectors, the transposed copy of [B, F, F, D], the product, the sum, the masked_select of the
upper triangle and the cat; model_zoo/FFM/src/FFMv2.py:87-91: the two masked_selects, the product and the sum, then
`+ lr_out`).  The interaction alone, B 4096, F 39, both modes, D 2 and 4, forward and forward + backward.

    python scripts/bench_ffm.py [--batch 4096] [--iters 20] [--modes onn,ffm] [--dims 2,4]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up; five rounds that alternate the
sides, median and spread reported.  The HBM floor is the record's bytes: X read once forward; X read and dX written
once more for the backward (the ONN output / gradient rows and the FFM sums are left out of the floor: it is a floor).
Prints a table for profiles/ffm_ab.txt."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_eulernet import HBM_PEAK, timed  # noqa: E402
from fuxictr_amd import layers, ops  # noqa: E402


def torch_ops(mode, F, D, dev):
    """-> fn(emb [B, F, C * D], addend) in the reference's own sequence of torch ops"""
    P = F * (F - 1) // 2
    if mode == "onn":
        diag = torch.eye(F, device=dev).bool().unsqueeze(-1)
        triu = torch.triu(torch.ones(F, F, device=dev), 1).bool()

        def onn(emb, addend):
            E = emb.view(-1, F, F, D)
            own = torch.masked_select(E, diag).view(E.shape[0], -1)
            out = (E.transpose(1, 2) * E).sum(dim=-1)
            return torch.cat([own, torch.masked_select(out, triu).view(-1, P)], dim=1)
        return onn
    up = torch.triu(torch.ones(F, F - 1, device=dev), 0).bool().unsqueeze(-1)
    lo = torch.tril(torch.ones(F, F - 1, device=dev), -1).bool().t().unsqueeze(-1)

    def ffm(emb, addend):
        E = emb.view(-1, F, F - 1, D)
        upper, lower = torch.masked_select(E, up), torch.masked_select(E.transpose(1, 2), lo)
        return addend + (upper * lower).view(E.shape[0], -1).sum(dim=-1, keepdim=True)
    return ffm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--modes", default="onn,ffm")
    ap.add_argument("--dims", default="2,4", help="one shape per run gives a kernel profile of that shape")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F = a.batch, 39
    print("tile budget: FX_FFM_TILE_KB=%s" % os.environ.get("FX_FFM_TILE_KB", "unset (80)"))
    for mode in a.modes.split(","):
        for D in (int(d) for d in a.dims.split(",")):
            torch.manual_seed(0)
            C = ops.ffm_slots(mode, F)
            emb = torch.randn(B, F, C * D, device=dev).requires_grad_(True)
            add = torch.randn(B, 1, device=dev) if mode == "ffm" else None
            g = torch.randn(B, ops.ffm_out_floats(mode, F, D), device=dev)
            ref = torch_ops(mode, F, D, dev)

            def native_fwd():
                with torch.no_grad():
                    return layers.field_aware_interaction(emb, F, D, mode, add)

            def native_both():
                return torch.autograd.grad(layers.field_aware_interaction(emb, F, D, mode, add), [emb], g)

            def torch_fwd():
                with torch.no_grad():
                    return ref(emb, add)

            def torch_both():
                return torch.autograd.grad(ref(emb, add), [emb], g)
            yn, yt = native_fwd(), torch_fwd()
            err = float((yn - yt).abs().max() / yt.abs().max())
            gerr = float((native_both()[0] - torch_both()[0]).abs().max() / torch_both()[0].abs().max())
            print("%s B %d F %d D %d  tile %d samples   max |native - torch| / max |torch|: out %.2e, dX %.2e   %d timed "
                  "calls x 5 rounds" % (mode, B, F, D, ops.ffm_tile_rows(mode, F, D), err, gerr, a.iters))
            names = ["native forward", "torch forward", "native forward + backward", "torch forward + backward"]
            rows = dict(zip(names, timed([native_fwd, torch_fwd, native_both, torch_both], a.iters)))
            for name in names:
                print("%-32s median %9.1f us   min %9.1f   max %9.1f" % ((name,) + rows[name]))
            t = dict((k, v[0]) for k, v in rows.items())
            print("speed-up forward %.2f x, forward + backward %.2f x" % (t[names[1]] / t[names[0]],
                                                                         t[names[3]] / t[names[2]]))
            x_bytes = 4.0 * B * F * C * D
            for name, floor_bytes in ((names[0], x_bytes), (names[2], 3.0 * x_bytes)):
                floor = 1e6 * floor_bytes / HBM_PEAK
                print("%s: HBM floor (%.1f MB at %.1f TB/s) %.2f us: %.1f %% of it achieved"
                      % (name, floor_bytes / 1e6, HBM_PEAK / 1e12, floor, 100.0 * floor / t[name]))


if __name__ == "__main__":
    main()
