"""Golden vectors of DCNv2 with `use_low_rank_mixture=True` (CrossNetMix) from the REAL reference (model_zoo.DCNv2 of
reczoo/FuxiCTR), next to those of make_golden.py and in the same layout (`state0/`, `batchN/`,
`expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_dcnv2_mix.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

The reference's tables start at std 1e-4, where x_0 * (..) vanishes and a fixture that ignores the cross network
would still pass.  The embedding tables are rescaled (`emb_scale`, doubled until the assertions hold, at most
`emb_scale_max`), never the weights; the scale that was used is kept in `meta`.  Asserted per case, on the first
recorded forward and the recorded steps:
  * zeroing every U (the experts' outputs) moves the logits by at least 2 % of their largest magnitude (`u_share`:
    200 times the 1e-4 the logits are held to.  Not more: xavier_normal_ on [E, W, r] gives U a std of ~0.03, and tables
    scaled until U carries 5 % put every tanh into saturation, where V and C receive gradients that are rounding
    residue, which Adam's m / sqrt(v) turns into steps of +-lr: no fp32 run reproduces those);
  * zeroing the gating weights (a uniform mixture) moves them at all where there is more than one expert
    (`gate_share` > 0; with one expert the soft-max is 1 whatever the gate holds: the share is recorded as 0);
  * consecutive losses differ;
  * every parameter of `crossnet.` differs between state0 and state1, except the gate of a single expert (its
    gradient is exactly 0).
`finish` records whether the reference's last step reached the default clip of 10 (`max_norm_reached`, from the norm
of the clipped gradients, `last_grad_norm`): no case does at its last step (0.81, 1.71, 0.93 and 0.36), so the clip
of these fixtures is the identity there; the norms of the earlier steps are not recorded.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 150, 90, 11, 5, 211]
_BASE = dict(model="DCNv2", n_dense=1, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=31, emb_scale=1e3,
             emb_scale_max=1e6, optimizer="adam", emb_reg=0, net_reg=0, low_rank=32, num_experts=4, n_cross=2,
             stacked=[], hidden=[])
CASES = [
    # the reference's defaults r 32 / E 4 next to a deep tower; 8 fields of D = 8: W = 64
    dict(_BASE, name="dcnv2_mix_parallel_adam", structure="parallel", embedding_dim=8, hidden=[32, 16]),
    # D = 10 over 9 fields: W = 90 is no multiple of 4 (the kernels' k tails); three layers, r = 16, SGD
    dict(_BASE, name="dcnv2_mix_crossonly_d10_sgd", structure="crossnet_only", embedding_dim=10, n_dense=2, n_cross=3,
         low_rank=16, optimizer="SGD", lr=5e-2),
    # one expert (the soft-max is 1, the gate gets no gradient) and one layer (layer 0 is also the last)
    dict(_BASE, name="dcnv2_mix_stacked_e1", structure="stacked", embedding_dim=8, n_cross=1, num_experts=1,
         stacked=[32, 16]),
    # r = 8 and E = 3: E r + E = 27 columns of the down product, no multiple of 4 or 16
    dict(_BASE, name="dcnv2_mix_sp_r8_e3", structure="stacked_parallel", embedding_dim=8, low_rank=8, num_experts=3,
         stacked=[24], hidden=[32, 16]),
]


def build_reference(case, fmap):
    from model_zoo import DCNv2
    return DCNv2(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                 optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                 metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=case["emb_reg"],
                 net_regularizer=case["net_reg"], model_structure=case["structure"], use_low_rank_mixture=True,
                 low_rank=case["low_rank"], num_experts=case["num_experts"], num_cross_layers=case["n_cross"],
                 stacked_dnn_hidden_units=case["stacked"], parallel_dnn_hidden_units=case["hidden"],
                 dnn_activations="relu")


def _zeroed_share(params, forward, logit0):
    kept = [p.detach().clone() for p in params]
    for p in params:
        p.zero_()
    share = logit_share(forward()[0], logit0)
    for p, k in zip(params, kept):
        p.copy_(k)
    return share


def probe(model, batch, case):
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        u_share = _zeroed_share(list(model.crossnet.U_list), forward, logit0)
        gate_share = _zeroed_share([g.weight for g in model.crossnet.gating], forward, logit0)
    return logit0, p0, {"u_share": u_share, "gate_share": gate_share}


def accept(shares, case):
    return shares["u_share"] >= 0.02 and (case["num_experts"] == 1 or shares["gate_share"] > 0.0)


def finish(out, model, case, fmap):
    import numpy as np
    one = case["num_experts"] == 1
    want = [k[7:] for k in out if k.startswith("state1/crossnet.") and not (one and ".gating." in k)]
    moved = [k for k in want if not np.array_equal(out["state1/" + k], out["state0/" + k])]
    assert moved == want, (case["name"], sorted(set(want) - set(moved)))
    norm = float(sum(float(p.grad.pow(2).sum()) for p in model.parameters() if p.grad is not None) ** 0.5)
    return {"last_grad_norm": norm, "max_norm_reached": bool(norm >= case["max_norm"] * (1.0 - 1e-5))}


def run_case(case):
    record_case(case, build_reference, probe, accept, finish, is_table=lambda k: k.startswith("embedding_layer."))


if __name__ == "__main__":
    main(CASES, run_case)
