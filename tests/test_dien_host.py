"""DIEN on the native layers, host side (no GPU): zoo.DIEN + layers.GRU / DynamicGRU / AttentionLayer wired end to end
with the kernels replaced by torch-CPU emulations — tests/_cpu_emul.py for the existing ops, the four fx_gru_seq_* /
fx_seq_score_* wrappers emulated here from the layers' formulas (`gru_seq`, `seq_score`: plain torch ops of any
dtype, no nn.GRU, no packing) — against fixtures recorded from the REAL reference's model_zoo.DIEN
(tests/golden/make_golden_dien.py).  Checks the parameter names, the forward composition (parts read in place, the ids
as lengths and mask, the concatenation in front of the DNN), the autograd nodes' plumbing and the optimizer protocol;
the HIP kernels themselves are held to the same restatement in fp64 in tests/test_gpu_dien_kernel.py.

Stated tolerances (those of tests/test_gpu_models.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close.  The two Adam fixtures train under a clip that is reached (max_norm 1e-4), recorded in
their meta (tests/golden/make_golden_dien.py says why)."""
import numpy as np
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import LOGIT_TOL, allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory, tb

DIEN_CASES = ["dien_augru_pair_adam", "dien_zoo_test", "dien_agru_dot_sgd", "dien_gru_sumpool_sgd",
              "dien_neg_fields_present"]


def gru_seq(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh):
    """One recurrent layer in plain torch ops, from its formulas (any dtype) -> (states [B, L, H], final [B, H]).
    Positions 0 .. len-1 run, len = the number of non-zero ids; chunks (r, z, n) for "GRU", (u, r, n) otherwise."""
    x = torch.cat(list(parts), dim=-1)
    B, L, H = x.shape
    lens = (ids != 0).sum(dim=1)
    h = torch.zeros(B, H, dtype=x.dtype)
    states = []
    for t in range(L):
        live = (lens > t).unsqueeze(1)
        gx, gh = x[:, t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
        a, b, c = gx.split(H, dim=1)
        ha, hb, hc = gh.split(H, dim=1)
        if mode == "GRU":
            r, g = torch.sigmoid(a + ha), 1 - torch.sigmoid(b + hb)
        else:
            r = torch.sigmoid(b + hb)
            g = scores[:, t:t + 1].expand(B, H) if mode == "AGRU" else torch.sigmoid(a + ha) * scores[:, t:t + 1]
        n = torch.tanh(c + r * hc)
        h = torch.where(live, h + g * (n - h), h)
        states.append(torch.where(live, h, torch.zeros_like(h)))
    return torch.stack(states, dim=1), h


def seq_score(interest, tgts, ids, W, softmax):
    """The attention scores in plain torch ops (any dtype) -> [B, L]; a row without an open position gives zeros."""
    target = torch.cat(list(tgts), dim=-1)
    mask = (ids != 0).to(interest.dtype)
    v = target if W is None else target @ W.t()
    s = (interest * v.unsqueeze(1)).sum(dim=-1) * mask
    if softmax:
        s = torch.softmax(s + -1.e9 * (1 - mask), dim=-1) * (mask.sum(dim=1, keepdim=True) > 0).to(interest.dtype)
    return s


def _leaf(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


def _emul_gru_fwd(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh, states, final):
    with torch.no_grad():
        s, f = gru_seq(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh)
        states.copy_(s)
        final.copy_(f)
    return states, final


def _emul_gru_bwd(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh, states, d_states, d_final, dparts, d_scores,
                  grads, workspace):
    with torch.enable_grad():
        lp, la = [_leaf(t) for t in parts], _leaf(scores)
        lw = [_leaf(t) for t in (w_ih, w_hh, b_ih, b_hh)]
        s, f = gru_seq(lp, ids, la, mode, *lw)
        out = 0
        if d_states is not None:
            out = out + (s * d_states).sum()
        if d_final is not None:
            out = out + (f * d_final).sum()
        wanted = lp + lw + ([la] if la is not None else [])
        got = torch.autograd.grad(out, wanted, allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, wanted)]
    with torch.no_grad():
        for dst, g in zip(dparts, got[:len(lp)]):
            if dst is not None:
                dst.copy_(g)
        grads.copy_(torch.cat([g.reshape(-1) for g in got[len(lp):len(lp) + 4]]))
        if la is not None:
            d_scores.copy_(got[-1])
    return grads


def _emul_score_fwd(interest, tgts, ids, W, softmax, scores):
    with torch.no_grad():
        scores.copy_(seq_score(interest, tgts, ids, W, softmax))
    return scores


def _emul_score_bwd(interest, tgts, ids, W, softmax, scores, d_scores, d_interest, dtgts, dW, workspace):
    with torch.enable_grad():
        li, lt, lw = _leaf(interest), [_leaf(t) for t in tgts], _leaf(W)
        wanted = [li] + lt + ([lw] if lw is not None else [])
        got = torch.autograd.grad(seq_score(li, lt, ids, lw, softmax), wanted, d_scores, allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, wanted)]
    with torch.no_grad():
        if d_interest is not None:
            d_interest.copy_(got[0])
        for dst, g in zip(dtgts, got[1:1 + len(lt)]):
            if dst is not None:
                dst.copy_(g)
        if lw is not None:
            dW.copy_(got[-1])
    return dW


def _install(monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops
    monkeypatch.setattr(ops, "gru_seq_fwd", _emul_gru_fwd)
    monkeypatch.setattr(ops, "gru_seq_bwd", _emul_gru_bwd)
    monkeypatch.setattr(ops, "seq_score_fwd", _emul_score_fwd)
    monkeypatch.setattr(ops, "seq_score_bwd", _emul_score_bwd)
    monkeypatch.setattr(ops, "gru_workspace_floats", lambda B, H: 1)
    monkeypatch.setattr(ops, "seq_score_workspace_floats", lambda B, H: 1)


def _field(f):
    return tuple(f) if isinstance(f, list) else f


def build_dien(model_cls, g, tmp_path, gpu=-1, **extra):
    """DIEN with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_dien.py and the
    drop-in test)."""
    m = g.meta
    return build_from_golden(model_cls, g, tmp_path, gpu=gpu, dnn_hidden_units=m["hidden"],
                             dnn_activations=m["dnn_activations"], batch_norm=m["batch_norm"],
                             dien_target_field=[_field(f) for f in m["dien_target"]],
                             dien_sequence_field=[_field(f) for f in m["dien_sequence"]],
                             dien_neg_seq_field=[_field(f) for f in m["dien_neg"]], gru_type=m["gru_type"],
                             enable_sum_pooling=m["sum_pooling"], attention_type=m["attention_type"],
                             use_attention_softmax=m["use_softmax"], aux_loss_alpha=0, **extra)


def _build(g, tmp_path, monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_dien(zoo.DIEN, g, tmp_path)


def test_zoo_dien_is_importable():
    from fuxictr_amd import layers, ops, zoo
    assert callable(zoo.DIEN) and ops.GRU_MAX_H == 64 and ops.GRU_MAX_L == 256
    assert all(hasattr(layers, n) for n in ("GRU", "DynamicGRU", "AttentionLayer"))


@pytest.mark.parametrize("case", DIEN_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    assert "extraction_modules.0.weight_ih_l0" in g.state0 and "extraction_modules.0.bias_hh_l0" in g.state0
    if g.meta["gru_type"] == "GRU":
        assert "evolving_modules.0.weight_hh_l0" in g.state0
        assert not any(k.startswith("attention_modules") for k in g.state0)
    else:
        assert "evolving_modules.0.gru_cell.x2h.weight" in g.state0
        assert "evolving_modules.0.gru_cell.h2h.bias" in g.state0
        assert ("attention_modules.0.W_kernel" in g.state0) == (g.meta["attention_type"] == "bilinear_attention")
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", DIEN_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)
    k = "extraction_modules.0.weight_hh_l0"
    assert np.abs(g.state1[k] - g.state0[k]).max() > 0               # trained in the reference ...
    check_trajectory(model, g)                                        # ... and held here with every other weight


def test_forward_returns_the_five_keys(tmp_path, monkeypatch):
    g = Golden("dien_augru_pair_adam")
    model = _build(g, tmp_path, monkeypatch)
    model.eval()
    batch = tb(g.batches[-1])
    with torch.no_grad():
        out = model.forward(batch)
    B, L = batch["click_sequence"].shape
    H = 2 * g.meta["embedding_dim"]
    assert sorted(out.keys()) == ["interest_emb", "neg_emb", "pad_mask", "pos_emb", "y_pred"]
    assert tuple(out["y_pred"].shape) == (B, 1) and out["neg_emb"] is None
    assert tuple(out["interest_emb"].shape) == (B, L, H) and tuple(out["pos_emb"].shape) == (B, L, H)
    assert out["pad_mask"].dtype == torch.bool and tuple(out["pad_mask"].shape) == (B, L)
    assert torch.equal(out["pad_mask"], batch["click_sequence"] != 0)
    lens = (batch["click_sequence"] != 0).sum(dim=1)
    past = torch.arange(L).unsqueeze(0) >= lens.unsqueeze(1)
    assert float(out["interest_emb"][past].abs().max()) == 0          # zero past len, and in the empty rows
    assert float(out["interest_emb"][0].abs().max()) == 0 and int(lens[0]) == 0


def test_the_unused_u_chunk_has_exactly_zero_gradients_under_agru(tmp_path, monkeypatch):
    g = Golden("dien_agru_dot_sgd")
    assert g.meta["agru_u_chunk_grad"][0] == 0.0 and g.meta["agru_u_chunk_grad"][1] > 0      # the reference's own
    model = _build(g, tmp_path, monkeypatch)
    cell = model.evolving_modules[0].gru_cell
    before = [p.detach().clone() for p in (cell.x2h.weight, cell.h2h.weight, cell.x2h.bias, cell.h2h.bias)]
    model.train()
    model.train_step(tb(g.batches[0]))
    H = cell.h2h.weight.shape[1]
    for p, b in zip((cell.x2h.weight, cell.h2h.weight, cell.x2h.bias, cell.h2h.bias), before):
        assert torch.equal(p[:H], b[:H])                 # untouched to the bit: the gradient was an exact zero
    assert not torch.equal(cell.x2h.weight[H:], before[0][H:])


def test_limits_and_unsupported_options_raise(tmp_path, monkeypatch):
    _install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import layers, ops, zoo
    with pytest.raises(NotImplementedError, match="H % 4 == 0"):
        ops.gru_check(6)
    with pytest.raises(NotImplementedError, match="4 <= H <= 64"):
        ops.gru_check(68)
    with pytest.raises(NotImplementedError, match="1 <= L <= 256"):
        ops.gru_check(32, 257)
    ops.gru_check(32, 50)                                # the Taobao shape fits
    with pytest.raises(NotImplementedError, match="4 <= H <= 64"):
        layers.GRU(128, 128)
    with pytest.raises(NotImplementedError, match="one width"):
        layers.GRU(8, 16)
    with pytest.raises(NotImplementedError, match="AGRU and AUGRU"):
        layers.DynamicGRU(8, 8, gru_type="AIGRU")
    with pytest.raises(NotImplementedError, match="4 <= H <= 64"):
        layers.DynamicGRU(2, 2)
    with pytest.raises(NotImplementedError, match="din_attention"):
        layers.AttentionLayer(8, attention_type="din_attention")
    with pytest.raises(NotImplementedError, match="parts"):
        layers.GRU(8, 8).forward_parts([torch.zeros(2, 3, 4)], torch.ones(2, 3, dtype=torch.int32))
    g = Golden("dien_augru_pair_adam")
    from fuxictr_amd.features import FeatureMap
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": 8})
    kw = dict(gpu=-1, embedding_dim=8, optimizer="adam", loss="binary_crossentropy", task="binary_classification",
              metrics=["logloss"], verbose=0, model_root=str(tmp_path), dien_target_field=[("adgroup_id", "cate_id")],
              dien_sequence_field=[("click_sequence", "cate_sequence")])
    with pytest.raises(NotImplementedError, match=r"DIEN\.py:228"):
        zoo.DIEN(fmap, dien_neg_seq_field=[], aux_loss_alpha=0.5, **kw)
    with pytest.raises(NotImplementedError, match=r"DIEN\.py:283"):
        zoo.DIEN(fmap, dien_neg_seq_field=[], gru_type="AIGRU", **kw)
    with pytest.raises(NotImplementedError, match="din_attention"):
        zoo.DIEN(fmap, dien_neg_seq_field=[], attention_type="din_attention", **kw)
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):       # the default neg fields, absent
        zoo.DIEN(fmap, **kw)
    with pytest.raises(NotImplementedError, match="4 <= H <= 64"):
        zoo.DIEN(fmap, dien_neg_seq_field=[], **dict(kw, embedding_dim=40))
    model = zoo.DIEN(fmap, dien_neg_seq_field=[], **kw)       # ... and the width follows DIEN.py:112-138
    assert model.dnn.mlp[0].in_features == fmap.sum_emb_out_dim()


def test_entry_points_are_declared_and_validate_before_the_device():
    import ctypes
    from fuxictr_amd import _lib
    for name in ("fx_gru_seq_fwd", "fx_gru_seq_bwd", "fx_gru_workspace_floats", "fx_gru_grad_floats",
                 "fx_gru_limits", "fx_gru_tile_rows", "fx_seq_score_fwd", "fx_seq_score_bwd",
                 "fx_seq_score_workspace_floats"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    x, tgt = _lib.SeqParts(), _lib.SeqParts()
    x.n_parts, x.D = 2, 16
    tgt.n_parts, tgt.D = 2, 16

    def fwd(L, H, mode=0):
        return lib.fx_gru_seq_fwd(ctypes.byref(x), None, 0, None, 4, L, H, mode, None, None, None, None, None, None,
                                  None)
    assert fwd(50, 68) == 1 and b"4 <= H <= 64" in lib.fx_last_error()
    assert fwd(50, 30) == 1 and b"H % 4 == 0" in lib.fx_last_error()
    assert fwd(257, 32) == 1 and b"1 <= L <= 256" in lib.fx_last_error()
    assert fwd(50, 32, 3) == 1 and b"mode=3" in lib.fx_last_error()
    assert fwd(50, 48) == 1 and b"is not n_parts=2" in lib.fx_last_error()
    assert fwd(50, 32) == 1 and b"null part 0" in lib.fx_last_error()

    def score(L, H):
        return lib.fx_seq_score_fwd(None, ctypes.byref(tgt), None, 0, 4, L, H, None, 1, None, None)
    assert score(50, 68) == 1 and b"4 <= H <= 64" in lib.fx_last_error()
    assert score(0, 32) == 1 and b"1 <= L <= 256" in lib.fx_last_error()
    assert score(50, 32) == 1 and b"interest is null" in lib.fx_last_error()
    assert lib.fx_gru_grad_floats(32) == 6 * 32 * 32 + 6 * 32
    assert lib.fx_gru_tile_rows(32) == 16 and lib.fx_gru_tile_rows(64) == 8 and lib.fx_gru_tile_rows(24) == 20
    assert lib.fx_gru_workspace_floats(4096, 32) == 256 * (6 * 32 * 32 + 6 * 32)
    assert lib.fx_seq_score_workspace_floats(4096, 32) == 256 * 32 * 32
    lim = (ctypes.c_int32 * 4)()
    lib.fx_gru_limits(lim)
    assert list(lim)[:2] == [64, 256]


def _packed(d):
    """The pointer and stride fields of a packed struct fx_seq_parts as plain tuples (a null pointer reads as None)."""
    return {"seq": tuple(d.seq), "seq_ld": tuple(d.seq_ld), "seq_row_ld": tuple(d.seq_row_ld), "tgt": tuple(d.tgt),
            "tgt_ld": tuple(d.tgt_ld), "n_parts": d.n_parts, "D": d.D}


def test_the_one_packer_gives_the_fields_of_the_three_it_replaced():
    """ops._seq_parts on the layouts the three earlier packers met: contiguous tensors, column slices of a wider
    record, and B = 1 / L = 1, where the stride of the axis of extent 1 is replaced by the dense one.  The expected
    fields are written out from data_ptr() and stride()."""
    from fuxictr_amd import ops
    B, L, D = 5, 4, 3
    none3, zero3 = (None,) * 3, (0,) * 3
    # contiguous history and target, two parts (BST's input: both sides)
    s = [torch.zeros(B, L, D), torch.zeros(B, L, D)]
    t = [torch.zeros(B, D), torch.zeros(B, D)]
    assert _packed(ops._seq_parts(s, t, "t")) == {
        "seq": (s[0].data_ptr(), s[1].data_ptr(), None), "seq_ld": (L * D, L * D, 0), "seq_row_ld": (D, D, 0),
        "tgt": (t[0].data_ptr(), t[1].data_ptr(), None), "tgt_ld": (D, D, 0), "n_parts": 2, "D": D}
    # views of a wider record [B, L + 3, D + 3] at slot and column offsets of their own
    rec = torch.zeros(B, L + 3, D + 3)
    W, R = D + 3, (L + 3) * (D + 3)
    s = [rec[:, 1:1 + L, :D], rec[:, 2:2 + L, 2:2 + D]]
    t = [rec[:, 0, :D], rec[:, L + 2, 3:3 + D]]
    base = rec.data_ptr()
    assert s[1].stride() == (R, W, 1) and t[1].stride() == (R, 1)
    want_seq = (base + 4 * W, base + 4 * (2 * W + 2), None)
    want_tgt = (base, base + 4 * ((L + 2) * W + 3), None)
    assert _packed(ops._seq_parts(s, t, "t")) == {
        "seq": want_seq, "seq_ld": (R, R, 0), "seq_row_ld": (W, W, 0), "tgt": want_tgt, "tgt_ld": (R, R, 0),
        "n_parts": 2, "D": D}
    # the GRU input has no target side, the scores' target no sequence side; three parts fill the struct
    assert _packed(ops._seq_parts(s, None, "t")) == {
        "seq": want_seq, "seq_ld": (R, R, 0), "seq_row_ld": (W, W, 0), "tgt": none3, "tgt_ld": zero3, "n_parts": 2,
        "D": D}
    assert _packed(ops._seq_parts(None, t, "t")) == {
        "seq": none3, "seq_ld": zero3, "seq_row_ld": zero3, "tgt": want_tgt, "tgt_ld": (R, R, 0), "n_parts": 2, "D": D}
    t3 = [rec[:, i, :D] for i in range(3)]
    assert _packed(ops._seq_parts(None, t3, "t"))["tgt"] == (base, base + 4 * W, base + 8 * W)
    # a gradient description: a part nobody wants stays null, D comes from the caller
    g = torch.zeros(B, L, D)
    assert _packed(ops._seq_parts([None, g], None, "t", D)) == {
        "seq": (None, g.data_ptr(), None), "seq_ld": (0, L * D, 0), "seq_row_ld": (0, D, 0), "tgt": none3,
        "tgt_ld": zero3, "n_parts": 2, "D": D}
    assert _packed(ops._seq_parts([None], [None], "t", D)) == {
        "seq": none3, "seq_ld": zero3, "seq_row_ld": zero3, "tgt": none3, "tgt_ld": zero3, "n_parts": 1, "D": D}
    # B = 1: the sample stride of a view is whatever the slicing left; the packer hands on the dense one
    one = rec[2:3]
    s1, t1 = one[:, 1:1 + L, :D], one[:, 0, 1:1 + D]
    assert s1.stride(0) == R and t1.stride(0) == R
    assert _packed(ops._seq_parts([s1], [t1], "t")) == {
        "seq": (s1.data_ptr(), None, None), "seq_ld": (L * W, 0, 0), "seq_row_ld": (W, 0, 0),
        "tgt": (t1.data_ptr(), None, None), "tgt_ld": (D, 0, 0), "n_parts": 1, "D": D}
    # L = 1: the position stride likewise; an empty history (BST with L1 = 1) leaves the sequence side null
    sl = rec[:, 3:4, 1:1 + D]
    assert sl.stride(1) == W
    assert _packed(ops._seq_parts([sl], None, "t")) == {
        "seq": (sl.data_ptr(), None, None), "seq_ld": (R, 0, 0), "seq_row_ld": (D, 0, 0), "tgt": none3,
        "tgt_ld": zero3, "n_parts": 1, "D": D}
    s11 = rec[1:2, 3:4, :D]
    assert _packed(ops._seq_parts([s11], None, "t"))["seq_ld"] == (D, 0, 0)
    assert _packed(ops._seq_parts([rec[:, :0, :D]], [rec[:, 0, :D]], "t"))["seq"] == none3
    # the ids of the first sequence field: own row stride, the dense one at B = 1, null only where the caller allows
    ids = torch.zeros(B, L + 2, dtype=torch.int32)[:, :L]
    p, ld = ops._seq_ids(ids, B, L)
    assert (p.value, ld) == (ids.data_ptr(), L + 2)
    assert ops._seq_ids(ids[:1], 1, L)[1] == L
    p, ld = ops._seq_ids(None, B, L, nullable=True)
    assert (p.value, ld) == (None, 0)
    with pytest.raises((AssertionError, AttributeError)):
        ops._seq_ids(None, B, L)


def test_the_batch_dict_order_does_not_change_the_logits(tmp_path, monkeypatch):
    """The DNN's input is assembled in the feature map's order: a captured step's static batch lists its features by
    packed matrix (ids first, numerics behind them), not in the loader's order."""
    g = Golden("dien_augru_pair_adam")
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
    gru, att, evo = layers.GRU(8, 8), layers.AttentionLayer(8), layers.DynamicGRU(8, 8)
    evo.gru_cell.h2h.weight.requires_grad_(False)
    seq, tgt = torch.randn(3, 4, 8, requires_grad=True), torch.randn(3, 8)          # the target is not differentiated
    ids = torch.tensor([[1, 2, 0, 0], [0, 0, 0, 0], [3, 4, 5, 6]], dtype=torch.int32)

    def run():
        interest, _ = gru.forward_parts([seq], ids)
        return evo(interest, att(interest, tgt, ids), ids)[1]
    run().sum().backward()
    assert seq.grad is not None and tgt.grad is None and evo.gru_cell.h2h.weight.grad is None
    assert evo.gru_cell.x2h.weight.grad is not None and att.W_kernel.grad is not None
    assert gru.weight_hh_l0.grad is not None and float(seq.grad[1].abs().max()) == 0      # the empty history
    out = run()
    with torch.no_grad():
        gru.weight_ih_l0.mul_(2.0)                      # between forward and backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


def test_fixtures_meta_figures_are_within_their_bands():
    """What make_golden_dien.py asserted when it wrote the fixtures, re-read from their meta and batches."""
    for case in DIEN_CASES:
        g = Golden(case)
        m = g.meta
        assert m["candidate_saturated_share"] < 0.1 and 0.1 <= m["gate_mid_share"] <= 0.9, (case, m)
        assert m["recurrence_median"] > 1e-2 and m["long_rows"] >= 16, (case, m)
        if m["gru_type"] != "GRU" and m["use_softmax"]:
            assert 0.05 <= m["attention_peak_median"] <= 0.5, (case, m)
        assert m["max_norm_default"] == 10.0
        assert m["max_norm_reached"] == (m["optimizer"] == "adam") == (m["max_norm"] < 10.0), case
        if m["batch_norm"]:          # the reference's own gradient of a bias in front of a BatchNorm1d is residue
            b_res, w_max = m["bn_bias_grad_residue"]
            assert 0 <= b_res <= 1e-4 * w_max, (case, b_res, w_max)
        first = m["dien_sequence"][0]
        first = first[0] if isinstance(first, list) else first
        for b in g.batches:
            ids = np.asarray(b[first])
            lens = (ids != 0).sum(axis=1)
            L = ids.shape[1]
            assert lens[0] == 0 and lens[1] == 1 and lens[2] == L and lens[3] == L - 2 and ids[3, 1] == 0, case
