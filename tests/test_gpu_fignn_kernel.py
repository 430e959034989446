"""fx_fignn_fwd / _bwd and fx_fignn_head_fwd / _bwd alone, through ops, on a real MI355X against the fp64 torch-autograd
run of the restatement in tests/test_fignn_host.py (fignn_layer, attn_prediction; no nn.GRUCell).

Yardstick (that of tests/test_gpu_dien_kernel.py and tests/test_gpu_bst_kernel.py): per compared tensor e32 = max |the
same formulas in fp32 torch on the CPU - fp64|; the HIP result must lie within 4 * e32 + 1e-6 * max|ref|.  The observed
err / bound is printed per tensor.  Every output (and the workspace) is pre-filled with NaN; dX and the gradients are
compared element by element.

The LeakyReLU of the graph has a kink at 0 (the rule of tests/test_gpu_bst_kernel.py): a sample whose fp64
pre-activation w_src . x_i + w_dst . x_j (i != j) has an element within 1e-5 of zero gets an all-zero upstream
gradient, so it drops out of every gradient (samples are independent); at most 10 % of a case's samples may go that way
(asserted).  The forward is continuous across the kink: no sample is left out of the forward comparison.  Sigmoid and
tanh have no kinks.  Inputs of std 0.5 and W_attn of std 1 / sqrt(2 D) give the pre-activation a std of about 0.5, i.e.
about 1.6e-5 per element.  The data of a shape do not depend on the flag set, so one count holds for all four.  The
seed of a shape is the first of 100 + shape index, + 10, .. whose count is under the cap; samples dropped with it
(of B, with the forward tile rows of the library at the time of writing: 8 at F 39 / D 16, 8 at 26 / 40, 2 at 64 / 32,
16 at 4 / 64 and 3 / 8):
    shape 0 (1, 2, 4, 1): 0      shape 1 (7, 3, 8, 2): 0       shape 2 (33, 5, 10, 3): 0
    shape 3 (17, 39, 16, 3): 0   shape 4 (17, 26, 40, 2): 0    shape 5 (3, 64, 32, 1): 0
    shape 6 (17, 4, 64, 2): 0    shape 7 (9, 6, 8, 2) strided: 0       shape 8 (9, 6, 8, 2) misaligned: 0
    shape 9 (4099, 3, 8, 2): 0
every one with its first seed (100 + index)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_fignn_host import GRU, RES, REUSE, attn_prediction, fignn_layer, graph_preactivation, split_packed  # noqa: E402

DEV = torch.device("cuda", 0)
FLAG_SETS = [GRU | RES, GRU | REUSE, RES, REUSE]
KINK = 1e-5
SEEDS = [100, 101, 102, 103, 104, 105, 106, 107, 108, 109]


def shapes():
    """(B, F, D, layers, layout): the smallest shapes that reach each arm.  VEC = 1 at D = 10; the Criteo shape and
    the reference's default D = 40 with two full tiles and a ragged one; the F * D limit and the D limit with B just
    past one tile; x as a row-strided view; a base that is 4-byte but not 16-byte aligned at D % 4 == 0; more tiles
    than workgroups (256), so that a workgroup adds a second tile's sums to its row of partial gradients."""
    lim = ops.fignn_limits()

    def tile(F, D):
        return ops.fignn_tile_rows(F, D, GRU | RES)
    Fl, Dl = lim["F_max"], lim["FD_max"] // lim["F_max"]
    return [(1, 2, 4, 1, "dense"), (7, 3, 8, 2, "dense"), (33, 5, 10, 3, "dense"),
            (2 * tile(39, 16) + 1, 39, 16, 3, "dense"), (2 * tile(26, 40) + 1, 26, 40, 2, "dense"),
            (tile(Fl, Dl) + 1, Fl, Dl, 1, "dense"), (tile(4, lim["D_max"]) + 1, 4, lim["D_max"], 2, "dense"),
            (9, 6, 8, 2, "strided"), (9, 6, 8, 2, "misaligned"),
            (256 * ops.fignn_tile_rows(3, 8, GRU | RES, backward=True) + 3, 3, 8, 2, "dense")]


def make_case(shape, flags, seed):
    """fp64 data of a case; x and w_attn come first, so they (and the kink count) do not depend on the flags"""
    B, F, D, L, _ = shape
    g = torch.Generator().manual_seed(seed)

    def rnd(*s, std=1.0):
        return torch.randn(*s, generator=g, dtype=torch.float64) * std
    x, w_attn = rnd(B, F, D, std=0.5), rnd(2 * D, std=(2 * D) ** -0.5)
    d_h = rnd(B, F, D)
    LW = 1 if flags & REUSE else L
    W = torch.cat([rnd(LW, F * D * D, std=D ** -0.5), rnd(LW, F * D * D, std=D ** -0.5), rnd(LW, D, std=0.2)], dim=1)
    u = D ** -0.5
    gru = (rnd(3 * D, D, std=u), rnd(3 * D, D, std=u), rnd(3 * D, std=0.2), rnd(3 * D, std=0.2)) if flags & GRU else None
    pre = graph_preactivation(x, w_attn).abs()
    pre = pre + torch.eye(F, dtype=torch.float64) * 1e9                # (the diagonal is masked: no kink there)
    near = (pre < KINK).flatten(start_dim=1).any(dim=1)
    d_h[near] = 0.0
    return dict(x=x, w_attn=w_attn, d_h=d_h, W=W.contiguous(), gru=gru, dropped=int(near.sum()))


def reference(case, shape, flags, dtype):
    B, F, D, L, _ = shape

    def leaf(t):
        return t.to(dtype).clone().requires_grad_(True)
    x, W, wa = leaf(case["x"]), leaf(case["W"]), leaf(case["w_attn"])
    gru = tuple(leaf(t) for t in case["gru"]) if case["gru"] else None
    W_in, W_out, bias_p = split_packed(W, F, D)
    h = fignn_layer(x, W_in, W_out, bias_p, gru, wa, L, flags)
    leaves = [x, W] + list(gru or ()) + [wa]
    got = torch.autograd.grad(h, leaves, case["d_h"].to(dtype))
    n = F * D * D
    dW = got[1].detach().reshape(-1, 2 * n + D)
    out = {"h_out": h.detach(), "dX": got[0].detach(), "dW_in": dW[:, :n], "dW_out": dW[:, n:2 * n],
           "dbias_p": dW[:, 2 * n:], "dW_attn": got[-1].detach()}
    if gru:
        out.update(zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), [t.detach() for t in got[2:6]]))
    return out


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def place(x2d, layout):
    """x [B, F * D] on the device as the layout asks"""
    B, n = x2d.shape
    x2d = x2d.float()
    if layout == "strided":
        buf = nan(B, n + 4)
        buf[:, :n] = x2d.to(DEV)
        return buf[:, :n]
    if layout == "misaligned":
        buf = nan(B * n + 1)
        view = buf[1:].view(B, n)
        view.copy_(x2d.to(DEV))
        assert view.data_ptr() % 16 == 4
        return view
    return x2d.to(DEV).contiguous()


def hip(case, shape, flags):
    B, F, D, L, layout = shape

    def d(t):
        return t.float().to(DEV).contiguous()
    x = place(case["x"].reshape(B, F * D), layout)
    W, wa = d(case["W"]), d(case["w_attn"])
    gru = tuple(d(t) for t in case["gru"]) if case["gru"] else None
    h_out = nan(B, F * D)
    hs = nan(L - 1, B, F * D) if L > 1 else None
    ops.fignn_fwd(x, F, D, L, flags, W, gru, wa, h_out, hs)
    drec, grads = nan(B, F * D), nan(ops.fignn_grad_floats(F, D, L, flags))
    ws = nan(ops.fignn_workspace_floats(B, F, D, L, flags))
    ops.fignn_bwd(d(case["d_h"].reshape(B, F * D)), x, F, D, L, flags, W, gru, wa, hs, drec, grads, ws)
    torch.cuda.synchronize()
    n = F * D * D
    LW = 1 if flags & REUSE else L
    dW = grads[:LW * (2 * n + D)].view(LW, 2 * n + D)
    rest = grads[LW * (2 * n + D):]
    out = {"h_out": h_out.view(B, F, D), "dX": drec.view(B, F, D), "dW_in": dW[:, :n], "dW_out": dW[:, n:2 * n],
           "dbias_p": dW[:, 2 * n:], "dW_attn": rest[-2 * D:]}
    if gru:
        DD = 3 * D * D
        out.update({"dw_ih": rest[:DD].view(3 * D, D), "dw_hh": rest[DD:2 * DD].view(3 * D, D),
                    "db_ih": rest[2 * DD:2 * DD + 3 * D], "db_hh": rest[2 * DD + 3 * D:2 * DD + 6 * D]})
    return {k: v.cpu() for k, v in out.items()}


def bound_check(tag, name, got, r64, r32):
    assert got.shape == r64.shape, (tag, name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), (tag, name)
    e32 = float((r32.double() - r64).abs().max())
    bound = 4.0 * e32 + 1e-6 * float(r64.abs().max())
    err = float((got.double() - r64).abs().max())
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print("%s %-8s err %.3e bound %.3e ratio %.3f" % (tag, name, err, bound, ratio))
    assert err <= bound, (tag, name, err, bound)


_REFS = {}


def references(index, flags):
    """the fp64 and fp32 CPU runs of a case, computed once"""
    key = (index, flags)
    if key not in _REFS:
        shape = shapes()[index]
        case = make_case(shape, flags, SEEDS[index])
        _REFS[key] = (shape, case, reference(case, shape, flags, torch.float64),
                      reference(case, shape, flags, torch.float32))
    return _REFS[key]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["gru_res", "gru_reuse", "res", "reuse"])
@pytest.mark.parametrize("index", range(10))
def test_fignn_layer_against_fp64(index, flags):
    shape, case, r64, r32 = references(index, flags)
    B, F, D, L, layout = shape
    tag = "B%d F%d D%d L%d %s flags%d" % (B, F, D, L, layout, flags)
    print(tag, "dropped at the kink: %d of %d" % (case["dropped"], B))
    assert case["dropped"] <= 0.1 * B, (tag, case["dropped"])
    got = hip(case, shape, flags)
    assert sorted(got) == sorted(r64)
    for name in r64:
        bound_check(tag, name, got[name], r64[name], r32[name])


@pytest.mark.parametrize("index", range(10))
def test_fignn_head_against_fp64(index):
    B, F, D, L, _ = shapes()[index]
    gen = torch.Generator().manual_seed(SEEDS[index] + 1000)

    def rnd(*s, std=1.0):
        return torch.randn(*s, generator=gen, dtype=torch.float64) * std
    h, Z, w1, g = rnd(B, F, D, std=0.5), rnd(B, F), rnd(1, D, std=D ** -0.5), rnd(B, 1)
    refs = []
    for dtype in (torch.float64, torch.float32):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (h, Z, w1)]
        out = attn_prediction(*leaves)
        gr = torch.autograd.grad(out, leaves, g.to(dtype))
        refs.append({"logit": out.detach(), "dH": gr[0], "dZ": gr[1], "dw1": gr[2]})

    def d(t):
        return t.float().to(DEV).contiguous()
    H, Zd, wd = d(h.reshape(B, F * D)), d(Z), d(w1.reshape(-1))
    logit = nan(B, 1)
    ops.fignn_head_fwd(H, Zd, wd, F, D, logit)
    dH, dZ, dw1 = nan(B, F * D), nan(B, F), nan(D)
    ops.fignn_head_bwd(d(g), H, Zd, wd, F, D, dH, dZ, dw1, nan(ops.fignn_workspace_floats(B, F, D, L, 0)))
    torch.cuda.synchronize()
    got = {"logit": logit.cpu(), "dH": dH.view(B, F, D).cpu(), "dZ": dZ.cpu(), "dw1": dw1.view(1, D).cpu()}
    tag = "head B%d F%d D%d" % (B, F, D)
    for name in refs[0]:
        bound_check(tag, name, got[name], refs[0][name], refs[1][name])
    # more samples than one workgroup pass of the backward (256 workgroups x 4 waves): the grid-stride arm
    if index == 1:
        B2 = 256 * 4 + 3
        h2, Z2, g2 = rnd(B2, F, D, std=0.5), rnd(B2, F), rnd(B2, 1)
        leaves = [t.clone().requires_grad_(True) for t in (h2, Z2, w1)]
        r64 = torch.autograd.grad(attn_prediction(*leaves), leaves, g2)
        leaves32 = [t.float().clone().requires_grad_(True) for t in (h2, Z2, w1)]
        r32 = torch.autograd.grad(attn_prediction(*leaves32), leaves32, g2.float())
        H2, Z2d = d(h2.reshape(B2, F * D)), d(Z2)
        dH2, dZ2, dw2 = nan(B2, F * D), nan(B2, F), nan(D)
        ops.fignn_head_bwd(d(g2), H2, Z2d, wd, F, D, dH2, dZ2, dw2, nan(ops.fignn_workspace_floats(B2, F, D, L, 0)))
        torch.cuda.synchronize()
        bound_check(tag + " B%d" % B2, "dw1", dw2.view(1, D).cpu(), r64[2], r32[2])
        bound_check(tag + " B%d" % B2, "dH", dH2.view(B2, F, D).cpu(), r64[0], r32[0])
