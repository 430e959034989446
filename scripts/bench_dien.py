"""A/B of DIEN's native interest block (csrc/fx_gru.hip: GRU, bilinear soft-max scores, AUGRU; three launches forward)
against the same mathematics composed from torch on the same GPU: nn.GRU over the padded history, the scores as
matmuls and a masked soft-max, then the reference-style per-step AUGRU cell loop over padded tensors
(model_zoo/DIEN/src/DIEN.py:241-294, 342-370, 426-448, without its host read of the lengths and its packing, so the
torch side is not charged for them).  B 4096, L 50, H 32 (two fields of D 16).

    python scripts/bench_dien.py [--batch 4096] [--iters 50]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up, five rounds, median and
spread reported.  Prints a table for profiles/dien_ab.txt."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

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


class TorchBlock(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.gru = nn.GRU(H, H, batch_first=True)
        self.W = nn.Parameter(torch.eye(H))
        self.x2h, self.h2h = nn.Linear(H, 3 * H), nn.Linear(H, 3 * H)
        self.H = H

    def forward(self, seqs, tgts, ids):
        x, target = torch.cat(seqs, dim=-1), torch.cat(tgts, dim=-1)
        mask = (ids != 0).float()
        lens = mask.sum(dim=1)
        L = x.shape[1]
        live = (torch.arange(L, device=x.device).unsqueeze(0) < lens.unsqueeze(1)).float()
        interest = self.gru(x)[0] * live.unsqueeze(-1)          # (post-padded ids: the first len positions)
        s = ((interest @ self.W) @ target.unsqueeze(-1)).squeeze(-1) * mask
        a = torch.softmax(s + -1.e9 * (1 - mask), dim=-1)
        h = torch.zeros(x.shape[0], self.H, device=x.device)
        for t in range(L):                                       # DynamicGRU's loop of AUGRU cells
            i_u, i_r, i_n = self.x2h(interest[:, t]).chunk(3, 1)
            h_u, h_r, h_n = self.h2h(h).chunk(3, 1)
            u = torch.sigmoid(i_u + h_u) * a[:, t:t + 1]
            n = torch.tanh(i_n + torch.sigmoid(i_r + h_r) * h_n)
            h = torch.where(live[:, t:t + 1] > 0, h + u * (n - h), h)
        return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B, L, D, n = a.batch, 50, 16, 2
    H = D * n
    seqs = [(torch.randn(B, L, D, device=dev) * 0.5).requires_grad_(True) for _ in range(n)]
    tgts = [(torch.randn(B, D, device=dev) * 0.5).requires_grad_(True) for _ in range(n)]
    lens = torch.randint(1, L + 1, (B,), device=dev)
    ids = (torch.arange(L, device=dev).unsqueeze(0) < lens.unsqueeze(1)).to(torch.int32)
    ref = TorchBlock(H).to(dev)
    gru, att, evo = layers.GRU(H, H), layers.AttentionLayer(H), layers.DynamicGRU(H, H)
    with torch.no_grad():
        for dst, src in ((gru.weight_ih_l0, ref.gru.weight_ih_l0), (gru.weight_hh_l0, ref.gru.weight_hh_l0),
                         (gru.bias_ih_l0, ref.gru.bias_ih_l0), (gru.bias_hh_l0, ref.gru.bias_hh_l0),
                         (evo.gru_cell.x2h.weight, ref.x2h.weight), (evo.gru_cell.x2h.bias, ref.x2h.bias),
                         (evo.gru_cell.h2h.weight, ref.h2h.weight), (evo.gru_cell.h2h.bias, ref.h2h.bias)):
            dst.copy_(src)
    gy = torch.randn(B, H, device=dev)
    native_params = list(gru.parameters()) + list(att.parameters()) + list(evo.parameters())

    def native(seqs, tgts):
        interest, _ = gru.forward_parts(seqs, ids)
        return evo(interest, att.forward_parts(interest, tgts, ids), ids)[1]

    def native_fwd():
        with torch.no_grad():
            return native(seqs, tgts)

    def native_both():
        torch.autograd.grad(native(seqs, tgts), seqs + tgts + native_params, gy)

    def torch_fwd():
        with torch.no_grad():
            return ref(seqs, tgts, ids)

    def torch_both():
        torch.autograd.grad(ref(seqs, tgts, ids), seqs + tgts + list(ref.parameters()), gy)
    err = float((native_fwd() - torch_fwd()).abs().max())
    print("B %d L %d parts %d D %d H %d   max |native - torch| final state %.2e" % (B, L, n, D, H, err))
    rows = [("native forward (3 launches)", timed(native_fwd, a.iters)),
            ("native forward + backward", timed(native_both, a.iters)),
            ("torch forward", timed(torch_fwd, max(a.iters // 5, 5))),
            ("torch forward + backward", timed(torch_both, max(a.iters // 5, 5)))]
    for name, (med, lo, hi) in rows:
        print("%-32s median %9.1f us   min %9.1f   max %9.1f" % (name, med, lo, hi))
    t = dict((k, v[0]) for k, v in rows)
    print("speed-up forward %.2f x, forward + backward %.2f x" % (
        t["torch forward"] / t["native forward (3 launches)"],
        t["torch forward + backward"] / t["native forward + backward"]))


if __name__ == "__main__":
    main()
