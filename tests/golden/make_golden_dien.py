"""Golden vectors of DIEN from the REAL reference (model_zoo.DIEN of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_dien.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

Every batch holds, in rows 0 .. 3 of every sequence feature, an empty history, one of length 1, a full one and one
with a padding id inside its first `len` positions (len counts the non-zero ids; pack_padded_sequence keeps the first
len positions, so that row feeds the recurrence a padding embedding in the middle).

A fixture must exercise the soft-max, the gates and the recurrence, so the generator asserts on the first recorded
forward and records in `meta`:
  * `attention_peak_median`: over the rows with len >= 3, the median of max_t a_t - 1 / len lies in [0.05, 0.5]
    (soft-max cases; neither uniform nor one-hot);
  * `candidate_saturated_share`: fewer than 10 % of the candidate-gate values have |n| > 0.99;
  * `gate_mid_share`: between 10 % and 90 % of the reset- and update-gate values of the extraction layer lie in
    (0.1, 0.9).  (`evolution_gate_mid_share` is recorded beside it and not held to the band: that layer's inputs are
    the extraction layer's states, inside (-1, 1) whatever the tables' scale.);
  * `recurrence_median`: over the rows with len >= 3, the median |state after position len-1 - state after position
    0| of the interest extraction layer is above 1e-2 (the recurrence matters).
The gates are those of the extraction layer, from a plain restatement of torch.nn.GRU's cell over the padded history
(checked against the module's own interests to 1e-5), and those of the evolution cells (AGRU / AUGRU) from a forward
hook.  The tables are rescaled (`emb_scale`) for that, never the weights.

The Adam cases train under a clip that is reached (max_norm 1e-4, recorded in `meta`), as BST's do.  With batch_norm
the bias of every Linear in front of a BatchNorm1d has a gradient that is zero in exact arithmetic (the norm takes
the batch mean off again); what the reference computes there is the rounding residue of its own sums, and under Adam
such an entry moves by lr * residue / (|residue| + eps), which no other summation order reproduces: at max_norm 1e-3
the HIP kernels missed conftest.assert_weights_close in `dnn.mlp.3.bias` alone (2 of 16 entries, 2.3e-5 against 2e-5;
the entries themselves are ~1e-5).  The smaller clip scales the residue further below eps; every real entry stays far
above it, and Adam's step does not depend on the scale of such a gradient.  `finish` shows the residue on the
reference's own last gradient (`bn_bias_grad_residue`), and the AGRU fixture's exactly-zero gradient of the unused u
chunk.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, pair_seq_spec, probing, record_case, small_seq_spec  # noqa: E402

ADAM_CLIP = 1e-4
_BASE = dict(model="DIEN", B=64, steps=3, lr=1e-2, max_norm=10.0, seed=11, emb_scale=2.5e4, optimizer="adam",
             schema="pair_seq", embedding_dim=8, hidden=[32, 16], dnn_activations="relu", batch_norm=True,
             gru_type="AUGRU", attention_type="bilinear_attention", use_softmax=True, sum_pooling=False,
             neg_fields=False)
CASES = [
    # two aligned histories: H = 2 * 8 = 16, L = 5; the defaults otherwise
    dict(_BASE, name="dien_augru_pair_adam", max_norm=ADAM_CLIP),
    # the hyper-parameters of the zoo's own DIEN_test (model_zoo/DIEN/config/model_config.yaml)
    dict(_BASE, name="dien_zoo_test", schema="small_seq", embedding_dim=4, hidden=[64, 32], dnn_activations="Dice",
         lr=1e-3, max_norm=ADAM_CLIP, emb_scale=3e4),
    dict(_BASE, name="dien_agru_dot_sgd", schema="small_seq", gru_type="AGRU", attention_type="dot_attention",
         use_softmax=False, batch_norm=False, optimizer="SGD", lr=2e-3),
    dict(_BASE, name="dien_gru_sumpool_sgd", gru_type="GRU", sum_pooling=True, optimizer="SGD", lr=5e-2, emb_scale=3e4),
    # (one target field, H = 4: at H = 8 and 16 no scale met the soft-max band and the gate band at once)
    dict(_BASE, name="dien_neg_fields_present", schema="small_seq", embedding_dim=4, neg_fields=True,
         optimizer="SGD", lr=5e-2, emb_scale=3e4),
]


def fields_of(case):
    neg = [["neg_click_sequence", "neg_cate_sequence"]] if case["neg_fields"] else []
    if case["schema"] == "pair_seq":
        return [["adgroup_id", "cate_id"]], [["click_sequence", "cate_sequence"]], neg
    return ["adgroup_id"], ["click_sequence"], neg


def make_spec(case):
    spec = pair_seq_spec(case["name"]) if case["schema"] == "pair_seq" else small_seq_spec(case["name"])
    if case["neg_fields"]:
        L = 5
        for name, share, vocab in (("neg_click_sequence", "adgroup_id", 97), ("neg_cate_sequence", "cate_id", 23)):
            spec["features"].append({name: {"source": "user", "type": "sequence", "feature_encoder": None,
                                            "share_embedding": share, "padding_idx": 0, "vocab_size": vocab,
                                            "max_len": L}})
        spec["num_fields"] = len(spec["features"])
    return spec


def build_reference(case, fmap):
    from model_zoo import DIEN
    target, sequence, neg = fields_of(case)
    as_field = lambda f: tuple(f) if isinstance(f, list) else f      # noqa: E731
    return DIEN(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=0, net_regularizer=0,
                dnn_hidden_units=case["hidden"], dnn_activations=case["dnn_activations"],
                batch_norm=case["batch_norm"], dien_target_field=[as_field(f) for f in target],
                dien_sequence_field=[as_field(f) for f in sequence], dien_neg_seq_field=[as_field(f) for f in neg],
                gru_type=case["gru_type"], enable_sum_pooling=case["sum_pooling"],
                attention_type=case["attention_type"], use_attention_softmax=case["use_softmax"], aux_loss_alpha=0)


def edit_batches(batches, spec, case):
    import numpy as np
    seq_names = [n for item in spec["features"] for n, fs in item.items() if fs["type"] == "sequence"]
    for b in batches:
        for n in seq_names:
            L = b[n].shape[1]
            fill = 1 + (np.arange(L) % 5)
            b[n][0, :] = 0                                           # empty
            b[n][1, :] = 0
            b[n][1, 0] = fill[0]                                     # length 1
            b[n][2, :] = np.where(b[n][2] == 0, fill, b[n][2])       # full
            b[n][3, :] = fill
            b[n][3, 1] = 0                                           # a padding id inside the first len = L - 2
            b[n][3, L - 1] = 0
        first = b["click_sequence"]
        lens = (first != 0).sum(axis=1)
        L = first.shape[1]
        assert lens[0] == 0 and lens[1] == 1 and lens[2] == L and lens[3] == L - 2 and first[3, 1] == 0, case["name"]


def gru_restated(gru, x, lens):
    """torch.nn.GRU's cell over the padded x [B, L, H] for the positions below lens -> (states, r, z, n at those)."""
    import torch
    w_ih, w_hh, b_ih, b_hh = gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0
    B, L, H = x.shape
    h = torch.zeros(B, H)
    states = torch.zeros(B, L, H)
    gates = [[], [], []]
    for t in range(L):
        live = lens > t
        gx, gh = x[:, t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
        r = torch.sigmoid(gx[:, :H] + gh[:, :H])
        z = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:])
        h = torch.where(live.unsqueeze(1), (1 - z) * n + z * h, h)
        states[:, t] = h * live.unsqueeze(1)
        for acc, v in zip(gates, (r, z, n)):
            acc.append(v[live].reshape(-1))
    return (states,) + tuple(torch.cat(g) for g in gates)


def probe(model, batch, case):
    import torch
    name, seen = case["name"], {"u": [], "r": [], "n": []}
    handles = []
    if case["gru_type"] != "GRU":
        def attention_hook(module, args, result):
            seen.setdefault("a", result.detach().clone())

        def cell_hook(module, args, result):
            x, hx = args[0], args[1]
            i_u, i_r, i_n = module.x2h(x).chunk(3, 1)
            h_u, h_r, h_n = module.h2h(hx).chunk(3, 1)
            r = torch.sigmoid(i_r + h_r)
            seen["r"].append(r.reshape(-1))
            seen["n"].append(torch.tanh(i_n + r * h_n).reshape(-1))
            if case["gru_type"] == "AUGRU":
                seen["u"].append(torch.sigmoid(i_u + h_u).reshape(-1))
        handles = [model.attention_modules[0].register_forward_hook(attention_hook),
                   model.evolving_modules[0].gru_cell.register_forward_hook(cell_hook)]
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        out = model.forward(batch)
    for h in handles:
        h.remove()
    # the fixture is not vacuous
    interest, mask, x = out["interest_emb"], out["pad_mask"], out["pos_emb"]
    lens = mask.sum(dim=1)
    with torch.no_grad():
        states, r, z, n = gru_restated(model.extraction_modules[0], x, lens)
    assert float((states - interest).abs().max()) <= 1e-5, (name, float((states - interest).abs().max()))
    long_rows = lens >= 3
    assert int(long_rows.sum()) >= 16, (name, int(long_rows.sum()))
    idx = torch.arange(len(lens))[long_rows]
    last = interest[idx, lens[long_rows] - 1]
    recurrence = float((last - interest[idx, 0]).abs().median())
    def mid_share(vals):
        vals = torch.cat(vals)
        return float(((vals > 0.1) & (vals < 0.9)).float().mean())
    cand = torch.cat([n] + ([torch.cat(seen["n"])] if seen["n"] else []))
    mid = mid_share([r, z])
    saturated = float((cand.abs() > 0.99).float().mean())
    shares = {"candidate_saturated_share": saturated, "gate_mid_share": mid, "recurrence_median": recurrence,
              "long_rows": int(long_rows.sum())}
    if seen["r"]:
        shares["evolution_gate_mid_share"] = mid_share(seen["u"] + seen["r"])
    if case["gru_type"] != "GRU" and case["use_softmax"]:
        nz = lens[lens > 0]
        shares["attention_peak_median"] = float((seen["a"].max(dim=-1).values - 1.0 / nz.float())[nz >= 3].median())
    print(name, shares)
    assert saturated < 0.1, (name, saturated)
    assert 0.1 <= mid <= 0.9, (name, mid)
    assert recurrence > 1e-2, (name, recurrence)
    if case["gru_type"] != "GRU" and case["use_softmax"]:
        peak = shares["attention_peak_median"]          # (the hook saw the non-empty rows, [rows, L])
        assert 0.05 <= peak <= 0.5, (name, peak)
    return logit0, p0, shares


def finish(out, model, case, fmap):
    target, sequence, neg = fields_of(case)
    extra = {"dien_target": target, "dien_sequence": sequence, "dien_neg": neg, "max_norm_default": 10.0,
             "max_norm_reached": bool(case["max_norm"] < 10.0)}
    if case["batch_norm"]:
        # the residue claim above: the bias in front of the first BatchNorm1d against its weight
        lin = model.dnn.mlp[0]
        b_res, w_max = float(lin.bias.grad.abs().max()), float(lin.weight.grad.abs().max())
        assert b_res <= 1e-4 * w_max, (case["name"], b_res, w_max)
        extra["bn_bias_grad_residue"] = [b_res, w_max]
    if case["gru_type"] == "AGRU":
        # the u chunk is computed and unused (DIEN.py:402-407): the reference's own gradient there is exactly zero
        cell = model.evolving_modules[0].gru_cell
        H = cell.h2h.weight.shape[1]
        u_max = max(float(t.grad[:H].abs().max()) for t in (cell.x2h.weight, cell.h2h.weight, cell.x2h.bias,
                                                              cell.h2h.bias))
        rest = float(cell.x2h.weight.grad[H:].abs().max())
        assert u_max == 0.0 and rest > 0.0, (case["name"], u_max, rest)
        extra["agru_u_chunk_grad"] = [u_max, rest]
    return extra


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True, finish, make_spec=make_spec,
                edit_batches=edit_batches)


if __name__ == "__main__":
    main(CASES, run_case)
