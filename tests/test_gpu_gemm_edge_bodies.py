"""The k-loop body selection of the pipelined GEMM (fx_gemm_tile.hip, fx_gemm_pipe_tile) must not change a
single bit: tiles on the M / N edge on the unmasked bodies (FX_GEMM_EDGE_PLAIN=1, the round-4 default)
against the masked bodies wherever an edge is near (=0, rounds 1-3).  The switch is read once per
process: one subprocess per setting, the outputs compared bit for bit — on the shapes where edges matter (the 624-wide record:
first tower layer, CrossNetV2 layer; ragged M; K with and without a tail; K slabs).  Two settings wrong in the
same way would still agree: the parent also holds every output of the base run to float64, element by element."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, %r)
from fuxictr_amd import ops
dev = torch.device("cuda:0")
g = torch.Generator(device="cpu").manual_seed(7)
def rnd(*s):
    return torch.randn(*s, generator=g).to(dev)
out = {}
# (M, N_out, K_in): forward y = x W^T + b (K tail when K_in %% 32), then dW + dX pair
for tag, (M, N, K) in %r:
    x, W, b, dz = rnd(M, K), rnd(N, K), rnd(N), rnd(M, N)
    y = torch.empty(M, N, device=dev)
    ops.gemm(x, W, y, transb=True, bias=b, act=1)
    out[tag + "/y"] = y.cpu().numpy()
    for sk in (1, 8):
        dW, dx, rs = torch.empty(N, K, device=dev), torch.empty(M, K, device=dev), torch.empty(N, device=dev)
        ws = torch.empty(ops.gemm_workspace_floats(N, K, sk), device=dev)
        ops.gemm_dw_dx(dz, x, W, dW, dx, split_k=sk, workspace=ws, rowsum=rs)
        out["%%s/dW%%d" %% (tag, sk)] = dW.cpu().numpy()
        out["%%s/dx%%d" %% (tag, sk)] = dx.cpu().numpy()
        out["%%s/db%%d" %% (tag, sk)] = rs.cpu().numpy()
        dW2 = torch.empty(N, K, device=dev)
        ops.gemm(dz, x, dW2, transa=True, split_k=sk, workspace=ws)
        out["%%s/dWsingle%%d" %% (tag, sk)] = dW2.cpu().numpy()
np.savez(sys.argv[1], **out)
"""

# (M, N_out, K_in) of the script, in its order: the parent draws the same operands from the same generator
SHAPES = (("first", (4096, 1024, 624)), ("cross", (4096, 624, 624)), ("ragged", (1000, 520, 136)),
          ("small", (332, 260, 72)), ("tower", (2048, 512, 1024)), ("one_tile", (64, 64, 64)),
          ("two_tiles", (128, 64, 64)))
_ref = {}


def _reference():
    """float64 of every product of the script with its bound max(|A| @ |B|), computed once."""
    if not _ref:
        g = torch.Generator(device="cpu").manual_seed(7)
        for tag, (M, N, K) in SHAPES:
            x, W, b, dz = (torch.randn(*s, generator=g).double() for s in ((M, K), (N, K), (N,), (M, N)))
            _ref[tag] = {"y": (x @ W.t() + b, (x.abs() @ W.abs().t()).max().item()),
                         "dx": (dz @ W, (dz.abs() @ W.abs()).max().item()),
                         "dW": (dz.t() @ x, (dz.abs().t() @ x.abs()).max().item()),
                         "db": (dz.sum(0), dz.abs().sum(0).max().item())}
    return _ref


def _check_against_float64(z):
    """Every output of one run against float64, per element, with the bounds the project states for the fp32-MFMA
    kernels: 2e-6 x max(|A| @ |B|) without a K split (plus one ulp of the biased sum the epilogue rounds), 3e-6 x
    the same for the weight gradients that may be K-split, 1e-5 x the largest column sum of |dz| for the fused
    bias gradient."""
    for tag, r in _reference().items():
        zy, bound = r["y"]
        err = (torch.from_numpy(z[tag + "/y"]).double() - zy.clamp(min=0)).abs()
        assert bool((err <= 2e-6 * bound + 2.0 ** -23 * zy.abs()).all()), (tag, "y", err.max().item(), bound)
        for sk in (1, 8):
            for key, what, f in (("dx%d" % sk, "dx", 2e-6), ("dW%d" % sk, "dW", 2e-6 if sk == 1 else 3e-6),
                                 ("dWsingle%d" % sk, "dW", 2e-6 if sk == 1 else 3e-6), ("db%d" % sk, "db", 1e-5)):
                ref, bound = r[what]
                err = (torch.from_numpy(z["%s/%s" % (tag, key)]).double() - ref).abs().max().item()
                assert err <= f * bound, (tag, key, err, f * bound)     # (a NaN fails the comparison)


def _run(mode, tmp_path, var="FX_GEMM_EDGE_PLAIN"):
    out = str(tmp_path / ("%s_%s.npz" % (var, mode)))
    env = dict(os.environ)
    env["FX_GEMM_BF16X6"] = "0"       # these switches select among the fp32-MFMA kernels' forms
    env[var] = mode
    p = subprocess.run([sys.executable, "-c", SCRIPT % (ROOT, SHAPES), out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out)


def test_body_selection_is_bit_identical(tmp_path):
    base = _run("0", tmp_path)
    _check_against_float64(base)
    for mode in ("1",):
        z = _run(mode, tmp_path)
        assert sorted(z.files) == sorted(base.files)
        for k in base.files:
            assert np.array_equal(z[k].view(np.uint32), base[k].view(np.uint32)), (mode, k)


def test_vector_slab_reduce_is_bit_identical(tmp_path):
    """k_splitk_reduce_v4 (16-byte loads, all slabs of a vector in flight) adds the slabs in the order of
    the 4-byte kernel it replaces (FX_SPLITK_V4=0): weight gradients and bias gradients bit for bit."""
    base = _run("0", tmp_path, var="FX_SPLITK_V4")
    _check_against_float64(base)
    z = _run("1", tmp_path, var="FX_SPLITK_V4")
    for k in base.files:
        assert np.array_equal(z[k].view(np.uint32), base[k].view(np.uint32)), k
