"""BST on the native layers, host side (no GPU): zoo.BST + layers.BehaviorTransformer / TransformerBlock wired end to
end with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the two fx_bst_block_*
wrappers emulated here from the block's formulas — against fixtures recorded from the REAL reference's model_zoo.BST
(tests/golden/make_golden_bst.py).  Checks the parameter names, the forward composition (parts read in place, ids as
the mask, pooling, the concatenation in front of the DNN), the autograd node's plumbing and the optimizer protocol;
the HIP kernels themselves are held to an fp64 restatement in tests/test_gpu_bst_kernel.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close (position_emb is trained, so it is among them).

The two Adam fixtures train under a clip that is reached (max_norm 1e-3): the K third of in_proj_bias has a gradient
that is zero in exact arithmetic, and at the default clip Adam turned its rounding residue into the reference's own
trajectory (tests/golden/make_golden_bst.py says so at length)."""
import numpy as np
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import LOGIT_TOL, allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

BST_CASES = ["bst_pair_adam", "bst_zoo_test", "bst_single_causal_sgd", "bst_concat_two_layers", "bst_plain"]
POOLS = {"none": 0, "concat": 0, "mean": 1, "sum": 2, "target": 3}


def bst_block(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool, ffn_pre=None):
    """One block in plain torch ops, from its formulas (any dtype): -> Y [B, L1, dm] or [B, dm].
    ffn_pre: a list that receives the FFN's pre-activation [B, L1, dm]."""
    in_w, in_b, out_w, out_b, w1, b1, w2, b2, g1, be1, g2, be2 = w
    B = tgts[0].shape[0]
    L = seqs[0].shape[1]
    L1 = L + 1
    parts = [torch.cat([s, t.unsqueeze(1)], dim=1) for s, t in zip(seqs, tgts)]
    if pos is not None:
        parts.append(pos.unsqueeze(0).expand(B, L1, pos.shape[1]))
    X = torch.cat(parts, dim=-1)
    dm = X.shape[-1]
    hd = dm // H
    pad = torch.zeros(B, L1, dtype=torch.bool)
    if ids is not None and L > 0:
        pad[:, :L] = ids.cpu() == 0
    eye = torch.eye(L1, dtype=torch.bool)
    masked = pad.unsqueeze(1) & ~eye.unsqueeze(0)                                # [B, L1 (i), L1 (j)]
    if causal:
        masked = masked | torch.triu(torch.ones(L1, L1, dtype=torch.bool), 1).unsqueeze(0)
    QKV = X @ in_w.t() + in_b

    def heads(t):
        return t.reshape(B, L1, H, hd).permute(0, 2, 1, 3)
    Q, K, V = (heads(t) for t in QKV.split(dm, dim=-1))
    S = (Q @ K.transpose(-1, -2)) / hd ** 0.5
    S = S.masked_fill(masked.unsqueeze(1), float("-inf"))
    P = torch.softmax(S, dim=-1)
    A = (P @ V).permute(0, 2, 1, 3).reshape(B, L1, dm) @ out_w.t() + out_b

    def norm(t, g, be):
        mu = t.mean(dim=-1, keepdim=True)
        var = ((t - mu) ** 2).mean(dim=-1, keepdim=True)
        return (t - mu) / torch.sqrt(var + 1e-5) * g + be
    s = A + X if residual else A
    if layer_norm:
        s = norm(s, g1, be1)
    z = s @ w1.t() + b1
    if ffn_pre is not None:
        ffn_pre.append(z.detach())
    f = torch.where(z > 0, z, 0.01 * z) @ w2.t() + b2
    out = f + s if residual else f
    if layer_norm:
        out = norm(out, g2, be2)
    keep = (~pad).to(out.dtype).unsqueeze(-1)
    if pool == "mean":
        return (out * keep).sum(dim=1) / (keep.sum(dim=1) + 1e-12)
    if pool == "sum":
        return (out * keep).sum(dim=1)
    if pool == "target":
        return out[:, -1, :]
    return out


def _emul_fwd(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool, Y):
    with torch.no_grad():
        Y.copy_(bst_block(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool).reshape(Y.shape))
    return Y


def _emul_bwd(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool, dY, dseqs, dtgts, grads, workspace,
              dx_accumulate=False):
    n = len(tgts)
    with torch.enable_grad():
        leaves = [t.detach().clone().requires_grad_(True) for t in list(seqs) + list(tgts)]
        wl = [None if t is None else t.detach().clone().requires_grad_(True) for t in w]
        pl = None if pos is None else pos.detach().clone().requires_grad_(True)
        y = bst_block(leaves[:n], leaves[n:], pl, ids, wl, H, layer_norm, residual, causal, pool)
        wanted = leaves + [t for t in wl if t is not None] + ([pl] if pl is not None else [])
        got = torch.autograd.grad(y, wanted, dY.reshape(y.shape), allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, wanted)]
    with torch.no_grad():
        for dst, g in zip(list(dseqs) + list(dtgts), got[:2 * n]):
            if dst is not None:
                dst.add_(g) if dx_accumulate else dst.copy_(g)
        by_name = dict(zip(["in_w", "in_b", "out_w", "out_b", "w1", "b1", "w2", "b2", "ln1_w", "ln1_b", "ln2_w",
                            "ln2_b"][:len([t for t in wl if t is not None])], got[2 * n:]))
        dm = w[0].shape[1]
        off = 0
        for name, size in (("in_w", 3 * dm * dm), ("out_w", dm * dm), ("w1", dm * dm), ("w2", dm * dm),
                           ("in_b", 3 * dm), ("out_b", dm), ("b1", dm), ("b2", dm), ("ln1_w", dm), ("ln1_b", dm),
                           ("ln2_w", dm), ("ln2_b", dm)):
            if name in by_name:
                grads[off:off + size].copy_(by_name[name].reshape(-1))
            else:
                grads[off:off + size].zero_()
            off += size
        if pl is not None:
            grads[off:].copy_(got[-1].reshape(-1))
    return grads


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "bst_block_fwd", _emul_fwd)
    monkeypatch.setattr(ops, "bst_block_bwd", _emul_bwd)
    monkeypatch.setattr(ops, "bst_workspace_floats", lambda B, L1, dm, pos_D: 1)


def _field(f):
    return tuple(f) if isinstance(f, list) else f


def build_bst(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.BST with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_bst.py)."""
    m = g.meta
    return build_from_golden(zoo.BST, g, tmp_path, gpu=gpu, dnn_hidden_units=m["hidden"], dnn_activations="relu",
                             num_heads=m["heads"], stacked_transformer_layers=m["layers"], layer_norm=m["layer_norm"],
                             use_residual=m["use_residual"], bst_target_field=[_field(f) for f in m["bst_target"]],
                             bst_sequence_field=[_field(f) for f in m["bst_sequence"]], seq_pooling_type=m["pooling"],
                             use_position_emb=m["use_position_emb"], use_causal_mask=m["causal"], **extra)


def _build(g, tmp_path, monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_bst(zoo, g, tmp_path)


def test_zoo_bst_is_importable():
    from fuxictr_amd import layers, ops, zoo
    assert callable(zoo.BST) and ops.BST_MAX == 64
    assert hasattr(layers, "TransformerBlock") and hasattr(layers, "BehaviorTransformer")


@pytest.mark.parametrize("case", BST_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    assert "transformer_encoders.0.transformer_blocks.0.attention.in_proj_weight" in g.state0
    assert "transformer_encoders.0.transformer_blocks.0.attention.out_proj.bias" in g.state0
    assert "transformer_encoders.0.transformer_blocks.0.ffn.2.weight" in g.state0
    assert ("transformer_encoders.0.position_emb" in g.state0) == g.meta["use_position_emb"]
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", BST_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)
    if g.meta["use_position_emb"]:
        k = "transformer_encoders.0.position_emb"
        assert np.abs(g.state1[k] - g.state0[k]).max() > 0           # trained in the reference ...
    check_trajectory(model, g)                                        # ... and held here with every other weight


def test_fixtures_exercise_softmax_lrelu_and_padding():
    """What make_golden_bst.py asserted when it wrote the fixtures, re-read from their meta and batches."""
    for case in BST_CASES:
        g = Golden(case)
        m = g.meta
        assert 0.05 <= m["attention_peak_median"] <= 0.5 and m["attention_rows"] >= 32, (case, m)
        assert 0.1 <= m["lrelu_negative_share"] <= 0.9, (case, m)
        first = m["bst_sequence"][0]
        first = first[0] if isinstance(first, list) else first
        for b in g.batches:
            lens = (np.asarray(b[first]) != 0).sum(axis=1)
            L = np.asarray(b[first]).shape[1]
            assert (lens == 0).any() and (lens == L).any() and ((lens > 0) & (lens < L)).any(), case


def test_reset_parameters_gives_the_sinusoid(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    enc = layers.BehaviorTransformer(seq_len=7, model_dim=16, num_heads=2, position_dim=8)
    pos = torch.arange(7).float().unsqueeze(1)
    div = torch.exp(torch.arange(0, 8, 2).float() * (-np.log(10000.0) / 8))
    assert torch.allclose(enc.position_emb[:, 0::2], torch.sin(pos * div), atol=1e-6)
    assert torch.allclose(enc.position_emb[:, 1::2], torch.cos(pos * div), atol=1e-6)
    att = enc.transformer_blocks[0].attention
    assert float(att.in_proj_bias.abs().max()) == 0 and float(att.out_proj.bias.abs().max()) == 0
    assert float(att.in_proj_weight.abs().max()) <= (6.0 / (4 * 16)) ** 0.5 + 1e-6      # xavier-uniform bound
    with pytest.raises(NotImplementedError):
        att(torch.zeros(1, 7, 16))                       # a container: nothing to call


def test_limits_and_unsupported_options_raise(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers, ops
    with pytest.raises(NotImplementedError, match="L1 <= 64"):
        ops.bst_check(65, 48, 2)
    with pytest.raises(NotImplementedError, match="dm <= 64"):
        ops.bst_check(51, 96, 2)
    with pytest.raises(NotImplementedError, match="does not divide"):
        ops.bst_check(51, 48, 5)
    with pytest.raises(NotImplementedError, match="at most 4 times"):
        ops.bst_check(51, 60, 2, 10)
    ops.bst_check(51, 48, 2, 16)                         # the reference Taobao config fits
    with pytest.raises(NotImplementedError, match="dm <= 64"):      # ... with embedding_dim = 32 it does not
        layers.BehaviorTransformer(seq_len=51, model_dim=96, num_heads=2, position_dim=32)
    with pytest.raises(NotImplementedError, match="dropout"):
        layers.TransformerBlock(16, 16, 2, attn_dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        layers.BehaviorTransformer(seq_len=5, model_dim=16, num_heads=2, net_dropout=0.2, position_dim=8)
    with pytest.raises(NotImplementedError, match="ffn_dim"):
        layers.TransformerBlock(16, 32, 2)
    blk = layers.TransformerBlock(16, 16, 2)
    with pytest.raises(NotImplementedError, match="attn_mask"):
        blk(torch.zeros(2, 5, 16), attn_mask=torch.zeros(4, 5, 5, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="L1 <= 64"):
        blk(torch.zeros(2, 65, 16))


def test_entry_points_are_declared_and_validate_before_the_device():
    import ctypes
    from fuxictr_amd import _lib
    for name in ("fx_bst_block_fwd", "fx_bst_block_bwd", "fx_bst_workspace_floats", "fx_bst_grad_floats",
                 "fx_bst_limits"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    inp, w = _lib.SeqParts(), _lib.BstWeights()
    inp.n_parts, inp.D = 2, 16

    def fwd(L1, dm, H):
        return lib.fx_bst_block_fwd(ctypes.byref(inp), None, 0, 4, L1, dm, H, ctypes.byref(w), 1, 1, 0, 1, None, None)
    assert fwd(65, 48, 2) == 1 and b"L1 <= 64" in lib.fx_last_error()
    assert fwd(51, 96, 2) == 1 and b"dm <= 64" in lib.fx_last_error()
    assert fwd(51, 48, 5) == 1 and b"does not divide" in lib.fx_last_error()
    assert fwd(51, 48, 2) == 1 and b"is not (n_parts=2" in lib.fx_last_error()      # 48 != 2 * 16 without pos
    assert lib.fx_bst_grad_floats(51, 48, 16) == 6 * 48 * 48 + 10 * 48 + 51 * 16
    n4 = (6 * 48 * 48 + 10 * 48 + 51 * 16 + 3) // 4 * 4
    assert lib.fx_bst_workspace_floats(4096, 51, 48, 16) == (256 + 64) * n4


def test_the_batch_dict_order_does_not_change_the_logits(tmp_path, monkeypatch):
    """The DNN's input is assembled in the feature map's order.  A captured step's static batch lists its features by
    packed matrix (ids first, numerics behind them), not in the loader's order; built on the dict's own order the
    replayed step fed the tower permuted columns (loss 0.7032 against the eager 0.5830)."""
    g = Golden("bst_pair_adam")
    model = _build(g, tmp_path, monkeypatch)
    model.eval()
    batch = tb(g.batches[-1])
    shuffled = {k: batch[k] for k in reversed(list(batch.keys()))}
    with torch.no_grad():
        a = model.forward(batch)["y_pred"]._fx_logit.reshape(-1).numpy()
        b = model.forward(shuffled)["y_pred"]._fx_logit.reshape(-1).numpy()
    assert np.abs(a - g.expect["logit0"]).max() <= LOGIT_TOL
    assert np.abs(b - g.expect["logit0"]).max() <= LOGIT_TOL


def test_frozen_inputs_get_no_gradient_and_in_place_changes_are_noticed(monkeypatch):
    _install(monkeypatch)
    from fuxictr_amd import layers
    torch.manual_seed(0)
    enc = layers.BehaviorTransformer(seq_len=5, model_dim=16, num_heads=2, position_dim=8)
    blk = enc.transformer_blocks[0]
    blk.ffn[0].weight.requires_grad_(False)
    seq, tgt = torch.randn(3, 4, 8, requires_grad=True), torch.randn(3, 8)          # the target is not differentiated
    ids = torch.tensor([[1, 2, 0, 0], [0, 0, 0, 0], [3, 4, 5, 6]], dtype=torch.int32)
    out = enc.forward_parts([seq], [tgt], ids=ids, pool="mean")
    out.sum().backward()
    assert seq.grad is not None and tgt.grad is None and blk.ffn[0].weight.grad is None
    assert blk.ffn[2].weight.grad is not None and enc.position_emb.grad is not None
    out = enc.forward_parts([seq], [tgt], ids=ids, pool="mean")
    with torch.no_grad():
        blk.ffn[2].weight.mul_(2.0)                     # between forward and backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    with pytest.raises(NotImplementedError, match="at most 4 times"):        # four parts + position_emb
        layers.BehaviorTransformer(seq_len=5, model_dim=40, num_heads=2, position_dim=8)


def test_fixtures_record_the_clip_and_the_zero_gradient_residue():
    """The Adam fixtures say in their meta that they train under a reached clip instead of fit()'s default of 10, and
    every fixture records the reference's own gradient of in_proj_bias: its K third is rounding residue (below 1e-4
    of the Q third; the generator asserts it)."""
    for case in BST_CASES:
        m = Golden(case).meta
        assert m["max_norm_default"] == 10.0
        assert m["max_norm_reached"] == (m["optimizer"] == "adam") == (m["max_norm"] < 10.0), case
        k_res, q_max = m["k_bias_grad_residue"]
        assert 0 <= k_res <= 1e-4 * q_max, (case, k_res, q_max)
