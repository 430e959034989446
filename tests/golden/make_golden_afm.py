"""Golden vectors of AFM from the REAL reference (model_zoo.AFM of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_afm.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

The reference's tables start at std 1e-4: every pair product is ~1e-8, every score equal, the attention uniform and
the fixture vacuous.  The tables are rescaled (`emb_scale`, doubled until the assertions hold, at most
`emb_scale_max`), never the weights; the scale that was used and the measured shares are kept in `meta`.  Asserted
on the first recorded forward and the recorded steps, for a case with attention over more than one pair:
  * in at least half of the samples the largest attention weight is at least twice the smallest (`att_ratio_share`);
  * replacing the attention by the uniform 1 / P moves the logits by at least 5 % of their largest magnitude
    (`att_share`);
  * zeroing `weight_p` moves the logits by at least 5 % of their largest magnitude (`wp_share`);
  * consecutive losses differ;
  * attention.0.weight, attention.0.bias, attention.2.weight and weight_p.weight differ between state0 and state1.
`afm_two_fields` has one pair: its softmax is 1 whatever the score and the attention's three parameters get a zero
gradient, so of these only the `weight_p` share, the losses and weight_p's change can hold and are asserted.
`afm_noatt` does not run the attention: there the pair sum itself must matter (zeroing the tables' second-order
part is the `pair_share`) and the losses differ.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="AFM", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=23, emb_scale=2e3,
             emb_scale_max=1e6, optimizer="adam", use_attention=True)
CASES = [
    dict(_BASE, name="afm_adam", embedding_dim=8, attention_dim=8),
    # the reference's defaults D = 10, A = 10 over 9 fields (7 sparse + 2 dense): F * D = 90, no multiple of 4: the
    # kernels' scalar arm; SGD with a net regularizer
    dict(_BASE, name="afm_d10_sgd", embedding_dim=10, attention_dim=10, n_dense=2, optimizer="SGD", lr=5e-2,
         net_reg=1e-4),
    dict(_BASE, name="afm_noatt", embedding_dim=8, attention_dim=8, use_attention=False),
    # two fields: one pair, a softmax over a single score
    dict(_BASE, name="afm_two_fields", embedding_dim=8, attention_dim=8, n_dense=0, cards=[37, 211]),
    # the hyper-parameters of the zoo's own AFM_test (model_zoo/AFM/config/model_config.yaml)
    dict(_BASE, name="afm_zoo_test", embedding_dim=4, attention_dim=8, emb_reg=1e-8, lr=1e-3),
]
ATT_KEYS = ["attention.0.weight", "attention.0.bias", "attention.2.weight", "weight_p.weight"]


def build_reference(case, fmap):
    from model_zoo.AFM.src.AFM import AFM
    return AFM(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
               optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
               metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=case.get("emb_reg", 0),
               net_regularizer=case.get("net_reg", 0), attention_dim=case["attention_dim"],
               attention_dropout=[0, 0], use_attention=case["use_attention"])


def probe(model, batch, case):
    import torch
    att, shares = [], {}
    with probing(model, batch) as forward:
        h_att = model.attention.register_forward_hook(lambda m, i, r: att.append(r.detach().clone()))
        logit0, p0 = forward()
        h_att.remove()
        if case["use_attention"]:
            a = att[-1].squeeze(-1)                                     # [B, P]
            if a.shape[1] > 1:
                ratio = a.max(dim=1).values / a.min(dim=1).values
                shares["att_ratio_share"] = float((ratio >= 2.0).float().mean())
                h_uni = model.attention.register_forward_hook(lambda m, i, r: torch.full_like(r, 1.0 / r.shape[1]))
                shares["att_share"] = logit_share(forward()[0], logit0)
                h_uni.remove()
            kept = model.weight_p.weight.detach().clone()
            model.weight_p.weight.zero_()
            shares["wp_share"] = logit_share(forward()[0], logit0)
            model.weight_p.weight.copy_(kept)
        else:
            # without the pair sum: the linear part alone
            shares["pair_share"] = logit_share(model.lr_layer(model.get_inputs(batch)), logit0)
    return logit0, p0, shares


def accept(shares, case):
    floors = {"att_ratio_share": 0.5, "att_share": 0.05, "wp_share": 0.05, "pair_share": 0.05}
    return all(v >= floors[k] for k, v in shares.items())


def finish(out, model, case, fmap):
    import numpy as np
    n_pairs = fmap.num_fields * (fmap.num_fields - 1) // 2
    moved = [k for k in ATT_KEYS if not np.array_equal(out["state1/" + k], out["state0/" + k])]
    if case["use_attention"]:
        want = ATT_KEYS if n_pairs > 1 else ["weight_p.weight"]
        assert all(k in moved for k in want), (case["name"], moved)
    return {"n_pairs": n_pairs, "moved": moved}


def run_case(case):
    record_case(case, build_reference, probe, accept, finish)


if __name__ == "__main__":
    main(CASES, run_case)
