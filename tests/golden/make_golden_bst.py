"""Golden vectors of BST from the REAL reference (model_zoo.BST of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_bst.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must exercise the masked soft-max, the LeakyReLU and the padding, so the generator asserts on the first
recorded forward and records in `meta`:
  * block 0, over the rows of unpadded queries with at least 3 open keys: the median of max_k P - 1 / (open keys)
    lies in [0.05, 0.5] (neither uniform nor one-hot).  P comes from a forward hook that calls the attention once
    more with need_weights (the model's own call discards it);
  * block 0: between 10 % and 90 % of the LeakyReLU's inputs are negative;
  * every batch holds an all-padding history, a full one and one with padding (rows 0 and 1 are overwritten).
The tables are rescaled (`emb_scale`) for that, never the weights.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, pair_seq_spec, probing, record_case, small_seq_spec  # noqa: E402

_BASE = dict(model="BST", B=64, steps=3, lr=1e-2, max_norm=10.0, seed=7, emb_scale=3e4, optimizer="adam",
             schema="small_seq", embedding_dim=8, heads=2, layers=1, pooling="mean", causal=False, layer_norm=True,
             use_residual=True, use_position_emb=True, hidden=[32, 16])
# The K third of attention.in_proj_bias has a gradient that is zero in exact arithmetic (a constant added to every key's
# score leaves the soft-max alone), and the K rows' entries at position columns that hardly vary nearly so.  What the
# reference computes there is the rounding residue of its own sums, ~1e-10, far below Adam's eps = 1e-8, where Adam's
# step is lr * g / eps: at the default clip (max_norm 10, never reached) three steps move such an entry by up to
# ~0.06 lr of pure rounding noise, which no other order of the same sums reproduces (the torch-CPU emulation of
# tests/test_bst_host.py and the HIP kernels both missed conftest.assert_weights_close in exactly those entries, and
# nowhere else).  The Adam cases therefore train under a clip that IS reached: max_norm 1e-3 scales every gradient
# by c = 1e-3 / |g| before Adam sees it.  Adam's step does not depend on the scale of a gradient that stays above
# eps, so every real entry trains as before (and the clip coefficient is now part of what the fixtures check); the
# residue entries move c times as far, below the tolerance.
ADAM_CLIP = 1e-3
CASES = [
    # two aligned histories: dm = 3 * 8 = 24, L1 = 6
    dict(_BASE, name="bst_pair_adam", schema="pair_seq", max_norm=ADAM_CLIP),
    # the hyper-parameters of the zoo's own BST_test (model_zoo/BST/config/model_config.yaml)
    dict(_BASE, name="bst_zoo_test", embedding_dim=4, heads=4, hidden=[64, 32], lr=1e-3, max_norm=ADAM_CLIP),
    dict(_BASE, name="bst_single_causal_sgd", causal=True, pooling="target", optimizer="SGD", lr=5e-2),
    # (the cases whose optimizer is free run SGD: the K third of in_proj_bias has a gradient that is zero in exact
    # arithmetic - a constant added to every key's score leaves the soft-max alone - and so have the K rows' entries
    # at position columns that hardly vary; under Adam such an entry moves by ~lr * noise / eps per step in the
    # reference itself, which no other summation order reproduces)
    dict(_BASE, name="bst_concat_two_layers", layers=2, pooling="concat", optimizer="SGD", lr=5e-2),
    dict(_BASE, name="bst_plain", schema="pair_seq", layer_norm=False, use_residual=False, use_position_emb=False,
         pooling="sum", heads=1, emb_scale=1.5e4, optimizer="SGD", lr=5e-2),      # (no position columns: the tables alone make the scores)
]


def fields_of(case):
    if case["schema"] == "pair_seq":
        return [["adgroup_id", "cate_id"]], [["click_sequence", "cate_sequence"]]
    return ["adgroup_id"], ["click_sequence"]


def build_reference(case, fmap):
    from model_zoo import BST
    target, sequence = fields_of(case)
    as_field = lambda f: tuple(f) if isinstance(f, list) else f      # noqa: E731
    return BST(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
               optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
               metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=0, net_regularizer=0,
               dnn_hidden_units=case["hidden"], dnn_activations="relu", num_heads=case["heads"],
               stacked_transformer_layers=case["layers"], layer_norm=case["layer_norm"],
               use_residual=case["use_residual"], bst_target_field=[as_field(f) for f in target],
               bst_sequence_field=[as_field(f) for f in sequence], seq_pooling_type=case["pooling"],
               use_position_emb=case["use_position_emb"], use_causal_mask=case["causal"])


def make_spec(case):
    return pair_seq_spec(case["name"]) if case["schema"] == "pair_seq" else small_seq_spec(case["name"])


def edit_batches(batches, spec, case):
    import numpy as np
    seq_names = [n for item in spec["features"] for n, fs in item.items() if fs["type"] == "sequence"]
    for b in batches:            # row 0: an all-padding history, row 1: a full one
        for n in seq_names:
            b[n][0, :] = 0
            b[n][1, :] = np.where(b[n][1] == 0, 1 + (np.arange(b[n].shape[1]) % 5), b[n][1])
        lens = (b["click_sequence"] != 0).sum(axis=1)
        L = b["click_sequence"].shape[1]
        assert (lens == 0).any() and (lens == L).any() and ((lens > 0) & (lens < L)).any(), case["name"]


def probe(model, batch, case):
    import torch
    name, seen = case["name"], {}
    block0 = model.transformer_encoders[0].transformer_blocks[0]

    def attention_hook(module, args, kwargs, result):
        if "P" in seen or seen.get("busy"):
            return None
        seen["busy"] = True
        with torch.no_grad():
            _, P = module(*args, attn_mask=kwargs["attn_mask"], need_weights=True, average_attn_weights=False)
        seen["busy"] = False
        seen["P"], seen["mask"] = P.detach().clone(), kwargs["attn_mask"].detach().clone()
        return None

    def lrelu_hook(module, inp):     # (returns None: a pre-hook's return value would replace the input)
        seen.setdefault("neg", float((inp[0] < 0).float().mean()))
    handles = [block0.attention.register_forward_hook(attention_hook, with_kwargs=True),
               block0.ffn[1].register_forward_pre_hook(lrelu_hook)]
    with probing(model, batch) as forward:
        logit0, p0 = forward()
    for h in handles:
        h.remove()
    # the fixture is not vacuous
    H = case["heads"]
    P, mask = seen["P"], seen["mask"]                       # [B, H, L1, L1], [B * H, L1, L1] (True = masked)
    B, L1 = P.shape[0], P.shape[-1]
    open_keys = (~mask).view(B, H, L1, L1).sum(dim=-1)      # [B, H, L1]
    pad = torch.cat([batch["click_sequence"] == 0, torch.zeros(B, 1, dtype=torch.bool)], dim=1)
    rows = (~pad).unsqueeze(1).expand(B, H, L1) & (open_keys >= 3)
    peak = float((P.max(dim=-1).values - 1.0 / open_keys.float())[rows].median())
    assert int(rows.sum()) >= 32, (name, int(rows.sum()))
    assert 0.05 <= peak <= 0.5, (name, peak)
    assert 0.1 <= seen["neg"] <= 0.9, (name, seen["neg"])
    return logit0, p0, {"attention_peak_median": peak, "attention_rows": int(rows.sum()),
                        "lrelu_negative_share": seen["neg"]}


def finish(out, model, case, fmap):
    # the residue claim above, shown on the reference's own last gradient (as clipped; the ratio does not depend on
    # the clip): the K third of in_proj_bias against the Q third
    bias_grad = model.transformer_encoders[0].transformer_blocks[0].attention.in_proj_bias.grad
    third = bias_grad.numel() // 3
    k_res, q_max = float(bias_grad[third:2 * third].abs().max()), float(bias_grad[:third].abs().max())
    assert k_res <= 1e-4 * q_max, (case["name"], k_res, q_max)
    target, sequence = fields_of(case)
    # what departs from the reference's defaults, spelled out: fit()'s clip is 10
    return {"bst_target": target, "bst_sequence": sequence, "max_norm_default": 10.0,
            "max_norm_reached": bool(case["max_norm"] < 10.0),
            "k_bias_grad_residue": [k_res, q_max]}         # max |grad| of in_proj_bias's K third, of its Q third


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True, finish, make_spec=make_spec, edit_batches=edit_batches)


if __name__ == "__main__":
    main(CASES, run_case)
