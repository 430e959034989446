"""FiGNN on the native layers, host side (no GPU): zoo.FiGNN + layers.FiGNN_Layer / AttentionalPrediction wired end to
end with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the four fx_fignn_*
wrappers emulated here from the formulas of include/fxctr.h in plain torch ops (no nn.GRUCell), their backwards derived
by torch autograd — against fixtures recorded from the REAL reference's model_zoo.FiGNN
(tests/golden/make_golden_fignn.py).  Checks the parameter names, the fused node (one fignn_fwd per forward and one
fignn_bwd per backward whatever gnn_layers is) and the messages for the shapes outside the envelope; the HIP kernels
themselves are held to the fp64 run of the same restatement in tests/test_gpu_fignn_kernel.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, pred atol 2e-5, losses 1e-4 per step, trained
weights through conftest.assert_weights_close."""
import contextlib

import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

FIGNN_CASES = ["fignn_zoo_test", "fignn_adam", "fignn_reuse_d10_sgd", "fignn_nogru_nores", "fignn_two_fields"]
GRU, RES, REUSE = 1, 2, 4


# ---- the formulas, in the dtype of the arguments ----------------------------------------------------------
def fignn_layer(x, W_in, W_out, bias_p, gru, w_attn, layers, flags):
    """FiGNN.py:128-172, 200-203: x [B, F, D]; W_in / W_out [LW, F, D, D], bias_p [LW, D] (LW = 1 with REUSE);
    gru = (w_ih [3D, D], w_hh [3D, D], b_ih [3D], b_hh [3D]) or None; w_attn [2 D] -> h_out [B, F, D]"""
    B, F, D = x.shape
    w_src, w_dst = w_attn.reshape(-1)[:D], w_attn.reshape(-1)[D:]
    pre = (x @ w_src).unsqueeze(2) + (x @ w_dst).unsqueeze(1)                     # [B, i, j]
    alpha = torch.where(pre > 0, pre, 0.01 * pre)
    alpha = alpha.masked_fill(torch.eye(F, dtype=torch.bool), float("-inf"))
    g = torch.softmax(alpha, dim=-1)
    h = x
    for l in range(layers):
        k = 0 if flags & REUSE else l
        o = torch.einsum("fed,bfd->bfe", W_out[k], h)
        aggr = torch.bmm(g, o)
        a = torch.einsum("fed,bfd->bfe", W_in[k], aggr) + bias_p[k]
        if flags & GRU:
            w_ih, w_hh, b_ih, b_hh = gru
            gi = a @ w_ih.t() + b_ih
            gh = h @ w_hh.t() + b_hh
            r = torch.sigmoid(gi[..., :D] + gh[..., :D])
            z = torch.sigmoid(gi[..., D:2 * D] + gh[..., D:2 * D])
            n = torch.tanh(gi[..., 2 * D:] + r * gh[..., 2 * D:])
            h = (1 - z) * n + z * h
        else:
            h = a + h
        if flags & RES:
            h = h + x
    return h


def graph_preactivation(x, w_attn):
    """w_src . x_i + w_dst . x_j [B, F, F]: where the LeakyReLU of the graph has its kink (the kernel test's rule)"""
    D = x.shape[2]
    w = w_attn.reshape(-1)
    return (x @ w[:D]).unsqueeze(2) + (x @ w[D:]).unsqueeze(1)


def attn_prediction(h, Z, w1):
    """FiGNN.py:228-231 after the mlp2 product Z [B, F]: -> logit [B, 1]"""
    score = h @ w1.reshape(-1)
    return (torch.sigmoid(Z) * score).sum(dim=1, keepdim=True)


def split_packed(W, F, D):
    """the packed graph weights [LW, 2 F D D + D] -> W_in, W_out [LW, F, D, D], bias_p [LW, D]"""
    n = F * D * D
    W = W.reshape(-1, 2 * n + D)
    return W[:, :n].reshape(-1, F, D, D), W[:, n:2 * n].reshape(-1, F, D, D), W[:, 2 * n:]


def fignn_layer_grads(d_h, x, W, gru, w_attn, layers, flags):
    """autograd of fignn_layer -> dx [B, F, D], grads in the order of fx_fignn_bwd (flat)"""
    B, F, D = x.shape
    with torch.enable_grad():
        xs = x.detach().clone().requires_grad_(True)
        Ws = W.detach().clone().requires_grad_(True)
        gs = tuple(t.detach().clone().requires_grad_(True) for t in gru) if flags & GRU else None
        ws = w_attn.detach().clone().requires_grad_(True)
        W_in, W_out, bias_p = split_packed(Ws, F, D)
        out = fignn_layer(xs, W_in, W_out, bias_p, gs, ws, layers, flags)
        leaves = [xs, Ws] + list(gs or ()) + [ws]
        got = torch.autograd.grad(out, leaves, d_h.reshape(B, F, D), allow_unused=True)
    got = [torch.zeros_like(t) if v is None else v for v, t in zip(got, leaves)]
    return got[0], torch.cat([v.reshape(-1) for v in got[1:]])


# ---- emulations of the four ops -----------------------------------------------------------------------------
CALLS = {"fignn_fwd": 0, "fignn_bwd": 0, "fignn_head_fwd": 0, "fignn_head_bwd": 0}


def _emul_fignn_fwd(rec, F, D, layers, flags, W, gru, w_attn, h_out, hs):
    CALLS["fignn_fwd"] += 1
    from fuxictr_amd import ops
    ops.fignn_check(F, D, layers)
    with torch.no_grad():
        B = rec.shape[0]
        W_in, W_out, bias_p = split_packed(W, F, D)
        h_out.copy_(fignn_layer(rec.reshape(B, F, D), W_in, W_out, bias_p, gru, w_attn, layers, flags)
                    .reshape(B, F * D))
    return h_out


def _emul_fignn_bwd(d_h_out, rec, F, D, layers, flags, W, gru, w_attn, hs, drec, grads, workspace):
    CALLS["fignn_bwd"] += 1
    B = rec.shape[0]
    dx, gr = fignn_layer_grads(d_h_out, rec.reshape(B, F, D), W, gru, w_attn, layers, flags)
    drec.copy_(dx.reshape(B, F * D))
    grads.copy_(gr)
    return drec, grads


def _emul_head_fwd(H, Z, w1, F, D, logit):
    CALLS["fignn_head_fwd"] += 1
    with torch.no_grad():
        logit.copy_(attn_prediction(H.reshape(-1, F, D), Z, w1).reshape(logit.shape))
    return logit


def _emul_head_bwd(g, H, Z, w1, F, D, dH, dZ, dw1, workspace):
    CALLS["fignn_head_bwd"] += 1
    with torch.enable_grad():
        leaves = [t.detach().clone().requires_grad_(True) for t in (H, Z, w1)]
        out = attn_prediction(leaves[0].reshape(-1, F, D), leaves[1], leaves[2])
        a, b, c = torch.autograd.grad(out, leaves, g.reshape(out.shape))
    dH.copy_(a)
    dZ.copy_(b)
    dw1.copy_(c)
    return dH, dZ, dw1


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "fignn_fwd", _emul_fignn_fwd)
    monkeypatch.setattr(ops, "fignn_bwd", _emul_fignn_bwd)
    monkeypatch.setattr(ops, "fignn_head_fwd", _emul_head_fwd)
    monkeypatch.setattr(ops, "fignn_head_bwd", _emul_head_bwd)
    monkeypatch.setattr(ops, "fignn_workspace_floats", lambda B, F, D, layers, flags: 4)
    for k in CALLS:
        CALLS[k] = 0


def build_fignn(model_cls, g, tmp_path, gpu=-1, **extra):
    """zoo.FiGNN (or the reference's class) with a fixture's hyper-parameters and initial weights (shared with
    tests/test_gpu_fignn.py and tests/test_dropin_reference_fignn.py)."""
    return build_from_golden(model_cls, g, tmp_path, gpu=gpu, **fignn_keywords(g), **extra)


def fignn_keywords(g):
    m = g.meta
    return dict(gnn_layers=m["gnn_layers"], use_gru=m["use_gru"], use_residual=m["use_residual"],
                reuse_graph_layer=m["reuse_graph_layer"])


def _build(g, tmp_path, monkeypatch, **extra):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_fignn(zoo.FiGNN, g, tmp_path, **extra)


@contextlib.contextmanager
def _launches(fwd, bwd):
    """the launch counters over the block move by exactly (fwd, bwd), for the layer and for the head"""
    before = dict(CALLS)
    yield
    moved = {k: CALLS[k] - before[k] for k in CALLS}
    assert moved == {"fignn_fwd": fwd, "fignn_bwd": bwd, "fignn_head_fwd": fwd, "fignn_head_bwd": bwd}, moved


@pytest.mark.parametrize("flags", [GRU | RES, GRU | REUSE, RES, REUSE, 0])
def test_restatement_is_the_reference_composition(flags):
    """fignn_layer / attn_prediction against the reference's modules as they are written (nn.GRUCell, the [F^2, 2 D]
    concat, torch.matmul with the broadcast weights), rebuilt here from torch modules in fp64."""
    from itertools import product
    gen = torch.Generator().manual_seed(5)
    B, F, D, L = 5, 4, 6, 3
    LW = 1 if flags & REUSE else L

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64) * 0.5
    x, W_in, W_out, bias_p, w_attn = rnd(B, F, D), rnd(LW, F, D, D), rnd(LW, F, D, D), rnd(LW, D), rnd(1, 2 * D)
    cell = torch.nn.GRUCell(D, D).double() if flags & GRU else None
    gru = tuple(p.detach() for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)) if cell else None
    src, dst = zip(*list(product(range(F), repeat=2)))
    with torch.no_grad():
        cat = torch.cat([x[:, src, :], x[:, dst, :]], dim=-1)
        alpha = torch.nn.functional.leaky_relu(cat @ w_attn.t(), 0.01).view(-1, F, F)
        g = torch.softmax(alpha.masked_fill(torch.eye(F).bool(), float("-inf")), dim=-1)
        h = x
        for l in range(L):
            k = 0 if flags & REUSE else l
            o = torch.matmul(W_out[k], h.unsqueeze(-1)).squeeze(-1)
            a = torch.matmul(W_in[k], torch.bmm(g, o).unsqueeze(-1)).squeeze(-1) + bias_p[k]
            h = cell(a.view(-1, D), h.reshape(-1, D)).view(-1, F, D) if cell else a + h
            if flags & RES:
                h = h + x
        got = fignn_layer(x, W_in, W_out, bias_p, gru, w_attn, L, flags)
    assert torch.allclose(got, h, atol=1e-12), (got - h).abs().max()
    mlp1, mlp2 = rnd(1, D), rnd(F, F * D)
    want = (torch.sigmoid(h.flatten(start_dim=1) @ mlp2.t()) * (h @ mlp1.t()).squeeze(-1)).sum(dim=1, keepdim=True)
    assert torch.allclose(attn_prediction(h, h.flatten(start_dim=1) @ mlp2.t(), mlp1), want, atol=1e-12)


@pytest.mark.parametrize("case", FIGNN_CASES)
def test_state_dict_keys_are_the_references(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (build_from_golden asserts keys, shapes and dtypes)
    keys = set(model.state_dict().keys())
    gnn = ["fignn.gnn."] if g.meta["reuse_graph_layer"] else ["fignn.gnn.%d." % i for i in range(g.meta["gnn_layers"])]
    want = {p + n for p in gnn for n in ("W_in", "W_out", "bias_p")} | {"fignn.W_attn.weight", "fc.mlp1.weight",
                                                                         "fc.mlp2.0.weight"}
    if g.meta["use_gru"]:
        want |= {"fignn.gru." + n for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    assert {k for k in keys if not k.startswith("embedding_layer.")} == want
    # the graph layers' Parameters are views of the one packed storage the kernel reads, and stay so when moved
    model.double().float()
    layer = model.fignn
    first = layer._graph_layers()[0]
    assert first.W_in.data_ptr() == layer._packed.data_ptr()
    assert first.bias_p.data_ptr() == layer._packed[0, 2 * first.W_in.numel():].data_ptr()


@pytest.mark.parametrize("case", FIGNN_CASES)
def test_forward_logits_match_reference(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)
    with _launches(1, 0):
        check_forward(model, g, "0")


@pytest.mark.parametrize("case", FIGNN_CASES)
def test_training_trajectory_matches_reference(case, tmp_path, monkeypatch):
    """One fignn_fwd and one fignn_bwd per step, whatever gnn_layers is."""
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)
    check_trajectory(model, g, per_step=lambda i: _launches(1, 1))


def test_limits_are_the_librarys_and_every_shape_outside_them_raises(monkeypatch):
    from fuxictr_amd import layers, ops
    lim = ops.fignn_limits()
    assert lim["F_min"] == 2 and lim["D_max"] >= 40 and lim["FD_max"] >= 39 * 40 and lim["layers_max"] >= 3
    ops.fignn_check(2, 1, 1)
    ops.fignn_check(lim["FD_max"] // lim["D_max"], lim["D_max"], lim["layers_max"])
    bad = [(1, 8, 1), (lim["F_max"] + 1, 1, 1), (2, lim["D_max"] + 1, 1), (2, 0, 1),
           (lim["FD_max"] // 16 + 1, 16, 1), (4, 8, 0), (4, 8, lim["layers_max"] + 1)]
    for F, D, L in bad:
        with pytest.raises(NotImplementedError, match="limit"):
            ops.fignn_check(F, D, L)
        with pytest.raises(NotImplementedError, match="limit"):
            layers.FiGNN_Layer(F, D, gnn_layers=L)
    # the wrappers themselves ask before anything is launched
    monkeypatch.setattr(ops, "_need_cuda", lambda t, name: None)
    x = torch.zeros(3, 8)
    W = torch.zeros(ops.fignn_layer_floats(1, 8))
    with pytest.raises(NotImplementedError, match="F=1"):
        ops.fignn_fwd(x, 1, 8, 1, 0, W, None, torch.zeros(16), torch.zeros(3, 8), None)
    with pytest.raises(NotImplementedError, match="F=1"):
        ops.fignn_bwd(x, x, 1, 8, 1, 0, W, None, torch.zeros(16), None, torch.zeros(3, 8), torch.zeros(1),
                      torch.zeros(4))
    assert ops.fignn_tile_rows(1, 8) == 0 and ops.fignn_tile_rows(39, 16) >= 1
    assert ops.fignn_grad_floats(39, 16, 3, GRU | RES) == 3 * (2 * 39 * 256 + 16) + 6 * 256 + 96 + 32
    assert ops.fignn_grad_floats(39, 16, 3, GRU | REUSE) == (2 * 39 * 256 + 16) + 6 * 256 + 96 + 32
    assert ops.fignn_grad_floats(39, 16, 3, RES) == 3 * (2 * 39 * 256 + 16) + 32
