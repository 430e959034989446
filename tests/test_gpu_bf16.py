"""Opt-in bf16 table storage (`emb_dtype: bf16`, BASELINE north_star "vectorised fp32/bf16 gathers") on
a real MI355X: rows are read as bf16 and widened, every sum, the Adam moments and the update arithmetic
stay fp32, updated rows are rounded to nearest-even.
  kernels   bf16 tables give exactly what the fp32 kernels give on the widened table (forward), and the
            fp32 result rounded once (catch-up, update)
  model     at the c2 shapes: same (bf16-representable) weights -> logits within 1e-4 of the oracle;
            after 10 training steps the deviation from the fp32 oracle is REPORTED and bounded loosely —
            it is the price of 8-bit mantissas in the table, not an implementation error."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import baseline_shapes as BS  # noqa: E402
from fuxictr_amd import _lib, ops, zoo  # noqa: E402
from oracle import ctr_oracle as O  # noqa: E402
from test_gpu_fused import DEV, _dev, _ids, _schema, _tables  # noqa: E402


def test_bf16_gather_equals_fp32_gather_of_the_widened_table():
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(5)
    D, B = 16, 1500
    vocabs = [50, 3, 1000, 7, 20011]
    bases, R = _schema(vocabs)
    C, Fd = len(vocabs), 3
    table16 = torch.randn(R, D, generator=g).bfloat16()
    num_w = torch.randn(Fd, D, generator=g)
    table1, num_w1 = torch.randn(R, 1, generator=g), torch.randn(Fd, 1, generator=g)
    ids = _ids(rng, B, vocabs, "power")
    dense = torch.rand(B, Fd, generator=g)
    F = C + Fd
    off_c = _dev([(Fd + c) * D for c in range(C)], torch.int64)
    off_n = _dev([j * D for j in range(Fd)], torch.int64)
    scal = ops.new_scalars(DEV)
    outs = []
    for tab in (table16.to(DEV), table16.float().to(DEV)):
        rec = torch.empty(B, F * D, device=DEV)
        lr = torch.empty(B, 1, device=DEV)
        fm = torch.empty(B, 1, device=DEV)
        S = torch.empty(B, D, device=DEV)
        ops.emb_fm_fwd(tab, D, _dev(ids, torch.int32), _dev(bases, torch.int64),
                       _dev(vocabs, torch.int32), off_c, _dev(dense), _dev(num_w), off_n, rec, scal,
                       table1=_dev(table1), num_w1=_dev(num_w1), lr_out=lr, fm_out=fm, S=S)
        outs.append((rec, lr, fm, S))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_bf16_catchup_and_update_round_the_fp32_result_once(kind):
    rng = np.random.default_rng(9)
    vocabs = [5, 40, 3000]
    bases, R = _schema(vocabs)
    B, C, D = 900, 3, 16
    ids = _ids(rng, B, vocabs, "power")
    ws = torch.empty(ops.dedup_workspace_bytes(B * C), dtype=torch.uint8, device=DEV)
    t, m, v = _tables(rng, R, D)
    t = t.bfloat16()
    last = torch.from_numpy(rng.integers(0, 5, R).astype(np.int32))
    G = torch.randn(B * C, D)
    res = {}
    for name, tab in (("bf16", t.clone()), ("fp32", t.float())):
        scal = ops.new_scalars(DEV, lr=0.01)
        scal.view(torch.int32)[_lib.SC_STEP] = 6
        st = ops.RowState(tab.to(DEV), m.clone().to(DEV) if kind == "adam" else None,
                          v.clone().to(DEV) if kind == "adam" else None, last.clone().to(DEV), D)
        dd = ops.dedup_catchup(_dev(ids, torch.int32), _dev(bases, torch.int64),
                               _dev(vocabs, torch.int32), _dev([0, 0, 0], torch.int32), ws,
                               [st] if kind == "adam" else [], scal, begin_scal=scal)
        mid = st.table.clone()
        st.G = G.to(DEV)
        ops.sparse_update_multi(kind, [st], dd, scal)
        torch.cuda.synchronize()
        res[name] = (mid, st.table.clone(), st.m, st.v)
    # catch-up: the fp32 replay rounded once
    assert torch.equal(res["bf16"][0].float(), res["fp32"][0].bfloat16().float())
    # update on top of it: start both from the bf16 catch-up result for a like-for-like comparison
    nu = int(dd.n_unique.item())
    rows = dd.uniq_row[:nu].long()
    scal = ops.new_scalars(DEV, lr=0.01)
    scal.view(torch.int32)[_lib.SC_STEP] = 7
    ops.opt_begin_step(scal)
    base = res["bf16"][0]
    outs = []
    for tab in (base.clone(), base.float()):
        st = ops.RowState(tab, torch.zeros(R, D, device=DEV) if kind == "adam" else None,
                          torch.zeros(R, D, device=DEV) if kind == "adam" else None,
                          torch.zeros(R, dtype=torch.int32, device=DEV), D, G=G.to(DEV))
        ops.sparse_update_multi(kind, [st], dd, scal)
        outs.append(st.table)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][rows].float(), outs[1][rows].bfloat16().float())


def test_bf16_model_error_report_at_c2_shapes(tmp_path):
    case, dist = "c2_deepfm", "powerlaw"
    model, features, cfg, spec, cards = BS.build(case, zoo, 0, tmp_path, emb_dtype="bf16")
    grp = model.embedding_layer.embedding_layer.table_groups()[0]
    assert grp.table.dtype == torch.bfloat16 and grp.m.dtype == torch.float32
    state0 = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    tr = O.OracleTrainer(cfg, state0, features, lr=1e-3, max_norm=10.0)      # fp32 everywhere
    teacher = BS.Teacher(features)
    rng = np.random.default_rng(11)
    train = BS.make_batches(case, spec, cards, rng, 4096, 10, dist, teacher)
    test = BS.make_batches(case, spec, cards, rng, 4096, 8, dist, teacher)
    model.eval()
    lg, _ = BS.logits_of(model, BS.tb(train[0]))
    d0 = float(np.abs(lg - tr.logits(BS.tb(train[0])).numpy()).max())
    assert d0 <= 1e-4, d0                                    # same (bf16-representable) weights
    model.train()
    model._max_gradient_norm = 10.0
    ln, lo = [], []
    for b in train:
        t = BS.tb(b)
        ln.append(float(model.train_step(t).item()))
        lo.append(tr.train_step(t, t["label"])[0])
    model.eval()
    from sklearn.metrics import log_loss, roc_auc_score
    y = np.concatenate([b["label"] for b in test]).astype(np.float64)
    lgn = np.concatenate([BS.logits_of(model, BS.tb(b))[0] for b in test])
    lgo = np.concatenate([tr.logits(BS.tb(b)).numpy() for b in test])
    pn, po = 1 / (1 + np.exp(-lgn.astype(np.float64))), 1 / (1 + np.exp(-lgo.astype(np.float64)))
    rep = {"logit0": d0, "loss_max_diff": float(np.abs(np.asarray(ln) - np.asarray(lo)).max()),
           "logit_max": float(np.abs(lgn - lgo).max()), "logit_mean": float(np.abs(lgn - lgo).mean()),
           "auc": (float(roc_auc_score(y, pn)), float(roc_auc_score(y, po))),
           "logloss": (float(log_loss(y, pn)), float(log_loss(y, po)))}
    print("[bf16 tables vs fp32 oracle, c2 shapes, 10 steps] " + json.dumps(rep))
    out = os.environ.get("FX_PARITY_REPORT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"case": "c2_deepfm_bf16_tables", **rep}) + "\n")
    assert rep["loss_max_diff"] < 5e-3 and abs(rep["auc"][0] - rep["auc"][1]) < 5e-3
    model.optimizer.check_errors()


@pytest.mark.parametrize("case,B", [("c2_deepfm", 8448), ("c4_din", 2048)])
def test_bf16_tables_on_the_generic_dedup_path(case, B, tmp_path):
    """outside the column fast path — B > 8192, or sequence columns that alias a
    table (DIN) — the exact-mode catch-up and the row update of a bf16 table go through the same
    dtype-aware kernels (fx_adam_catchup_rows / fx_sparse_adam_multi); a kernel that took the table for
    fp32 would write 4-byte floats into the 2-byte table.  Checked: rows no batch touched are bit-identical
    to their initial value after training (a stray fp32 write lands in other rows), the losses follow
    the fp32 oracle within the bf16 storage error, nothing is flagged."""
    dist = "powerlaw"
    model, features, cfg, spec, cards = BS.build(case, zoo, 0, tmp_path, emb_dtype="bf16")
    from fuxictr_amd.layers import FeatureEmbeddingDict
    groups = [g for mod in model.modules() if isinstance(mod, FeatureEmbeddingDict)
              for g in mod.table_groups()]
    main = [g for g in groups if g.table is not None and g.D > 1]
    assert main and all(g.table.dtype == torch.bfloat16 for g in main)
    before = [g.table.clone() for g in main]
    state0 = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    tr = O.OracleTrainer(cfg, state0, features, lr=1e-3, max_norm=10.0)
    teacher = BS.Teacher(features)
    rng = np.random.default_rng(3)
    train = BS.make_batches(case, spec, cards, rng, B, 4, dist, teacher)
    model.train()
    model._max_gradient_norm = 10.0
    ln, lo = [], []
    for b in train:
        t = BS.tb(b)
        ln.append(float(model.train_step(t).item()))
        lo.append(tr.train_step(t, t["label"])[0])
    torch.cuda.synchronize()
    model.optimizer.check_errors()
    assert np.abs(np.asarray(ln) - np.asarray(lo)).max() < 5e-3, (ln, lo)
    for g, b0 in zip(main, before):
        never = g.last_step == 0                               # never read by any batch
        assert int(never.sum()) > 0
        assert torch.equal(g.table[never].view(torch.int16), b0[never].view(torch.int16))
        assert torch.isfinite(g.table.float()).all()
