"""A/B of the fused BST transformer block (csrc/fx_bst.hip) against the reference's composition in plain torch on the
same GPU: nn.MultiheadAttention with the [B * H, L1, L1] bool mask, LayerNorm, FFN, masked mean pooling
(model_zoo/BST/src/BST.py:183-229, 345-366).  B 4096, L 50, two parts of D 16 + position_emb (dm 48), H 2, one block.

    python scripts/bench_bst.py [--batch 4096] [--iters 200]

Each side is timed over `iters` back-to-back calls between one event pair after warm-up, five rounds, median and
spread reported; the per-launch times of the fused side come from the same loop run on the forward and on the
backward launch alone.  Prints a table for profiles/bst_ab.txt."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fuxictr_amd import ops  # noqa: E402

PEAK_FP32_TFLOPS = 157.3      # MI355X vector fp32 FMA rate (256 CUs x 128 lanes x 2 flops x 2.4 GHz)


def timed(fn, iters, rounds=5):
    for _ in range(10):
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
    def __init__(self, dm, H):
        super().__init__()
        self.attention = nn.MultiheadAttention(dm, num_heads=H, batch_first=True)
        self.ffn = nn.Sequential(nn.Linear(dm, dm), nn.LeakyReLU(), nn.Linear(dm, dm))
        self.ln1, self.ln2 = nn.LayerNorm(dm), nn.LayerNorm(dm)
        self.H = H

    def forward(self, seqs, tgts, pos, ids):
        B = ids.shape[0]
        x = torch.cat([torch.cat(seqs, dim=-1), torch.cat(tgts, dim=-1).unsqueeze(1)], dim=1)
        x = torch.cat([x, pos.unsqueeze(0).repeat(B, 1, 1)], dim=-1)
        pad = torch.cat([ids == 0, torch.zeros(B, 1, dtype=torch.bool, device=ids.device)], dim=-1)
        L1 = pad.shape[1]
        mask = pad.unsqueeze(1).repeat(1, L1, 1) & ~torch.eye(L1, device=ids.device).bool().unsqueeze(0)
        mask = mask.unsqueeze(1).repeat(1, self.H, 1, 1).flatten(end_dim=1)
        attn, _ = self.attention(x, x, x, attn_mask=mask)
        s = self.ln1(attn + x)
        out = self.ln2(self.ffn(s) + s)
        keep = (1 - pad.float()).unsqueeze(-1)
        return (out * keep).sum(dim=1) / (keep.sum(dim=1) + 1e-12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B, L, D, H, n = a.batch, 50, 16, 2, 2
    L1, dm = L + 1, D * (n + 1)
    seqs = [torch.randn(B, L, D, device=dev) * 0.5 for _ in range(n)]
    tgts = [torch.randn(B, D, device=dev) * 0.5 for _ in range(n)]
    pos = torch.randn(L1, D, device=dev) * 0.7
    lens = torch.randint(0, L + 1, (B,), device=dev)
    ids = (torch.arange(L, device=dev).unsqueeze(0) < lens.unsqueeze(1)).to(torch.int32)
    ref = TorchBlock(dm, H).to(dev)
    w = (ref.attention.in_proj_weight, ref.attention.in_proj_bias, ref.attention.out_proj.weight,
         ref.attention.out_proj.bias, ref.ffn[0].weight, ref.ffn[0].bias, ref.ffn[2].weight, ref.ffn[2].bias,
         ref.ln1.weight, ref.ln1.bias, ref.ln2.weight, ref.ln2.bias)
    w = tuple(t.detach().contiguous() for t in w)
    y = torch.empty(B, dm, device=dev)
    gy = torch.randn(B, dm, device=dev)
    dseqs, dtgts = [torch.empty_like(t) for t in seqs], [torch.empty_like(t) for t in tgts]
    grads = torch.empty(ops.bst_grad_floats(L1, dm, D), device=dev)
    ws = torch.empty(ops.bst_workspace_floats(B, L1, dm, D), device=dev)
    cfg = (H, True, True, False, "mean")

    def fused_fwd():
        ops.bst_block_fwd(seqs, tgts, pos, ids, w, *cfg, y)

    def fused_bwd():
        ops.bst_block_bwd(seqs, tgts, pos, ids, w, *cfg, gy, dseqs, dtgts, grads, ws)

    def fused_both():
        fused_fwd()
        fused_bwd()
    leaves = [t.clone().requires_grad_(True) for t in seqs + tgts]
    pos_leaf = pos.clone().requires_grad_(True)

    def torch_fwd():
        with torch.no_grad():
            return ref(seqs, tgts, pos, ids)

    def torch_both():
        out = ref(leaves[:n], leaves[n:], pos_leaf, ids)
        torch.autograd.grad(out, leaves + [pos_leaf] + list(ref.parameters()), gy)
    with torch.no_grad():
        fused_fwd()
        err = float((y - ref(seqs, tgts, pos, ids)).abs().max())
    print("B %d L %d parts %d D %d H %d dm %d   max |fused - torch| forward %.2e" % (B, L, n, D, H, dm, err))
    rows = [("fused forward (1 launch)", timed(fused_fwd, a.iters)),
            ("fused backward (1 launch + fx_colsum's 2)", timed(fused_bwd, a.iters)),
            ("fused forward + backward", timed(fused_both, a.iters)),
            ("torch forward", timed(torch_fwd, max(a.iters // 4, 10))),
            ("torch forward + backward", timed(torch_both, max(a.iters // 4, 10)))]
    for name, (med, lo, hi) in rows:
        print("%-44s median %9.1f us   min %9.1f   max %9.1f" % (name, med, lo, hi))
    t = dict((k, v[0]) for k, v in rows)
    print("speed-up forward %.2f x, forward + backward %.2f x" % (
        t["torch forward"] / t["fused forward (1 launch)"],
        t["torch forward + backward"] / t["fused forward + backward"]))
    for name, key, back in (("forward", "fused forward (1 launch)", False),
                            ("backward", "fused backward (1 launch + fx_colsum's 2)", True)):
        fl = ops.bst_flops(B, L1, dm, backward=back)
        print("%s: %.3f MFLOP/sample, %.2f TFLOP/s = %.1f %% of the %.1f TFLOP/s fp32-FMA rate" % (
            name, fl / B / 1e6, fl / t[key] / 1e6, 100.0 * fl / t[key] / 1e6 / PEAK_FP32_TFLOPS, PEAK_FP32_TFLOPS))


if __name__ == "__main__":
    main()
