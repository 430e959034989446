"""fx_crossmix_fwd / _bwd alone, through ops, on a real MI355X against the fp64 torch-autograd run of the reference's
formulas (cross_net.py:158-201), written per expert as the reference writes them.

Yardstick (that of tests/test_gpu_fignn_kernel.py and tests/test_gpu_gatecross.py): per compared tensor e32 = max |the
same formulas in fp32 torch on the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  The observed
err / bound is printed per tensor.  Every output and the workspace are pre-filled with NaN and every element is
compared; tanh and the soft-max have no kinks, so no sample is left out.  The saturated case scales V and C so that
both pre-activations reach |a| ~ 50: tanh is +-1 there, its derivative 0, and everything must stay finite."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402

DEV = torch.device("cuda", 0)


def shapes():
    """(B, W, r, E, L, layout): the smallest shapes that reach each arm, tile sizes from the limits query."""
    lim = ops.crossmix_limits()
    tile, r_max, er = lim["tile_rows"], lim["r_max"], lim["Er_max"]
    return [(1, 4, 1, 1, 1, "dense"),                            # soft-max = 1, gate gradient 0
            (7, 6, 3, 2, 2, "dense"),                            # W % 4, r % 4 != 0, the gate shared by two layers
            (17, 390, 32, 4, 3, "dense"),                        # Criteo at D = 10
            (2 * tile + 1, 624, 32, 4, 3, "dense"),              # Criteo at D = 16: two tiles and a ragged one
            (tile + 1, lim["W_max"], r_max, er // r_max, 1, "dense"),    # the widest W at the largest E r
            (tile + 1, 64, r_max, 1, 2, "dense"),
            (9, 24, 8, 2, 2, "strided"), (9, 24, 8, 2, 2, "misaligned"),
            (lim["workgroups_max"] * tile + 3, 8, 4, 2, 2, "dense"),     # more tiles than workgroups
            (9, 24, 8, 2, 2, "saturated")]


def make_case(shape, seed):
    B, W, r, E, L, layout = shape
    g = torch.Generator().manual_seed(seed)

    def rnd(*s, std=1.0):
        return torch.randn(*s, generator=g, dtype=torch.float64) * std
    big = 100.0 if layout == "saturated" else 1.0           # |V^T x| ~ 0.5 * big, |C tanh| ~ sqrt(r) / sqrt(r) * big
    return dict(x=rnd(B, W, std=0.5), d_out=rnd(B, W),
                U=[rnd(E, W, r, std=r ** -0.5) for _ in range(L)],
                V=[rnd(E, W, r, std=big * W ** -0.5) for _ in range(L)],
                C=[rnd(E, r, r, std=big * r ** -0.5) for _ in range(L)],
                bias=[rnd(W, 1, std=0.2) for _ in range(L)], gate=[rnd(1, W, std=W ** -0.5) for _ in range(E)])


def reference(case, dtype):
    def leaves(ts):
        return [t.to(dtype).clone().requires_grad_(True) for t in ts]
    x, = leaves([case["x"]])
    U, V, Cs, bias, gate = (leaves(case[k]) for k in ("U", "V", "C", "bias", "gate"))
    x0 = x.unsqueeze(2)
    xl, kept = x0, []
    for l in range(len(U)):
        outs, scores = [], []
        for e in range(len(gate)):
            scores.append(xl.squeeze(2) @ gate[e].t())
            v = torch.tanh(Cs[l][e] @ torch.tanh(V[l][e].t() @ xl))
            outs.append((x0 * (U[l][e] @ v + bias[l])).squeeze(2))
        xl = torch.stack(outs, 2) @ torch.stack(scores, 1).softmax(1) + xl
        kept.append(xl.squeeze(2))
    got = torch.autograd.grad(kept[-1], [x] + U + V + Cs + bias + gate, case["d_out"].to(dtype), allow_unused=True)
    L, E, at = len(U), len(gate), iter(got)
    out = {"out": kept[-1].detach(), "dX": next(at)}
    for l in range(L - 1):
        out["x%d" % (l + 1)] = kept[l].detach()
    for name in ("dU", "dV", "dC"):
        out[name] = torch.stack([next(at) for _ in range(L)])
    out["dbias"] = torch.stack([next(at).view(-1) for _ in range(L)])
    out["dgating"] = torch.stack([next(at).view(-1) for _ in range(E)])
    return out


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def place(x, layout):
    B, n = x.shape
    if layout == "strided":
        buf = nan(B, n + 4)
        buf[:, :n] = x.float().to(DEV)
        return buf[:, :n]
    if layout == "misaligned":
        view = nan(B * n + 1)[1:].view(B, n)
        view.copy_(x.float().to(DEV))
        assert view.data_ptr() % 16 == 4
        return view
    return x.float().to(DEV).contiguous()


def hip(case, shape):
    B, W, r, E, L, layout = shape

    def d(ts):
        return [t.float().to(DEV).contiguous() for t in ts]
    x, d_out = place(case["x"], layout), place(case["d_out"], layout)
    U, V, Cs, bias, gate = (d(case[k]) for k in ("U", "V", "C", "bias", "gate"))
    out, dX = place(torch.full((B, W), float("nan")), layout), place(torch.full((B, W), float("nan")), layout)
    xs = nan(L - 1, B, W) if L > 1 else None
    zs = nan(L, B, E * r + E)
    ops.crossmix_fwd(x, U, V, Cs, bias, gate, out, xs, zs)
    ws = nan(ops.crossmix_workspace_floats(B, W, r, E, L))
    dU, dV, dC, dbias, dgate = ops.crossmix_bwd(d_out, x, U, V, Cs, bias, gate, xs, zs, dX, ws)
    torch.cuda.synchronize()
    got = {"out": out, "dX": dX, "dU": dU, "dV": dV, "dC": dC, "dbias": dbias, "dgating": dgate}
    for l in range(L - 1):
        got["x%d" % (l + 1)] = xs[l]
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("index", range(10))
def test_crossmix_against_fp64(index):
    shape = shapes()[index]
    case = make_case(shape, 300 + index)
    r64, r32 = reference(case, torch.float64), reference(case, torch.float32)
    got = hip(case, shape)
    tag = "B%d W%d r%d E%d L%d %s" % shape
    assert sorted(got) == sorted(r64)
    failed = []
    for name in sorted(r64):
        assert got[name].shape == r64[name].shape, (tag, name, got[name].shape, r64[name].shape)
        assert torch.isfinite(got[name]).all(), (tag, name)
        e32 = float((r32[name].double() - r64[name]).abs().max())
        bound = 4.0 * e32 + 1e-6 * float(r64[name].abs().max())
        err = float((got[name].double() - r64[name]).abs().max())
        print("%s %-8s err %.3e bound %.3e ratio %.3f" % (tag, name, err, bound, err / bound if bound else 0.0))
        if err > bound:
            failed.append((name, err, bound))
    assert not failed, (tag, failed)
