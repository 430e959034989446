"""Outputs of the fused DIN attention passes (fx_din_attn.hip) for one small shape per instantiation
family, fixed seeds, every output array into one .npz: run it on two builds and compare to the bit.
usage: python scripts/din_attn_dump.py OUT.npz"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fuxictr_amd import ops  # noqa: E402

# (B, L, E, H): general formulation <NB, FB, EC>, then q split <NB, EC>
SHAPES = [(7, 3, 4, 16), (6, 5, 12, 20), (40, 6, 8, 16), (300, 20, 16, 32),          # NB = 1
          (5, 3, 4, 33), (5, 1, 10, 64), (9, 4, 8, 40), (37, 9, 16, 64),             # NB = 2
          (3, 32, 8, 7), (50, 32, 16, 32), (33, 50, 8, 36), (19, 33, 16, 64)]        # q split

dev = torch.device("cuda", 0)
arrays = {}
for B, L, E, H in SHAPES:
    g = torch.Generator(device="cpu").manual_seed(B + L + E + H)
    q = torch.randn(B, E, generator=g).to(dev)
    K = torch.randn(B, L, E, generator=g).to(dev)
    W1 = (torch.randn(H, 4 * E, generator=g) * 0.3).to(dev)
    b1 = torch.randn(H, generator=g).to(dev)
    alpha = (torch.rand(H, generator=g) - 0.5).to(dev)
    W2 = torch.randn(H, generator=g).to(dev)
    b2 = torch.randn(1, generator=g).to(dev)
    mask = (torch.rand(B, L, generator=g) > 0.3).to(torch.int32).to(dev)
    dout = torch.randn(B, E, generator=g).to(dev)
    rm, rv = torch.zeros(H, device=dev), torch.ones(H, device=dev)
    ws = torch.zeros(ops.din_attn_workspace_floats(B, L, E, H), device=dev)
    sums = torch.zeros(2 * H + 1, device=dev)
    stats = torch.zeros(2 * H, device=dev)
    a = torch.zeros(B, L, device=dev)
    out = torch.zeros(B, E, device=dev)
    da = torch.zeros(B, L, device=dev)
    sums5 = torch.zeros(5 * H, device=dev)
    dq = torch.zeros(B, E, device=dev)
    dK = torch.zeros(B, L, E, device=dev)
    dW = torch.zeros(H * 4 * E + H, device=dev)
    rm1, rv1, stats1 = torch.zeros(H, device=dev), torch.ones(H, device=dev), torch.zeros(2 * H, device=dev)
    ops.din_attn_stats(q, K, W1, b1, sums, ws, stats1, 0.01, rm1, rv1)     # statistics in the same launch
    ops.dice_stats_from_sums(sums, H, B * L, 0.01, True, rm, rv, stats)
    ops.din_attn_fwd(q, K, W1, b1, alpha, 1e-9, stats, W2, b2, mask, a, out)
    ops.din_attn_bwd_sums(q, K, W1, b1, alpha, 1e-9, stats, W2, mask, dout, da, sums5, ws)
    ops.din_attn_bwd(q, K, W1, b1, alpha, 1e-9, True, stats, W2, mask, a, dout, da, sums5, B * L, dq, dK, dW, ws)
    torch.cuda.synchronize()
    for name, t in (("sums", sums[:2 * H]), ("stats1", stats1), ("rm1", rm1), ("rv1", rv1),
                    ("stats", stats), ("rm", rm), ("rv", rv), ("a", a), ("out", out),
                    ("da", da), ("sums5", sums5), ("dq", dq), ("dK", dK), ("dW", dW)):
        arrays["%dx%dx%dx%d/%s" % (B, L, E, H, name)] = t.cpu().numpy()
np.savez(sys.argv[1], **arrays)
print("wrote %d arrays to %s" % (len(arrays), sys.argv[1]))
