"""Golden vectors of FwFM and FmFM from the REAL reference (model_zoo.FwFM, model_zoo.FmFM of reczoo/FuxiCTR), next to
those of make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`,
`state1/`, `meta`), so that conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_pairfm.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

The reference's tables start at std 1e-4: every pair term is ~1e-8 and a fixture that ignores the interaction weight
would still pass.  The main embedding tables are rescaled (`emb_scale`, doubled until the assertions hold, at most
`emb_scale_max`), never the weights; the scale that was used is kept in `meta`.  Asserted per case, on the first
recorded forward and the recorded steps:
  * zeroing the interaction weight moves the logits by at least 5 % of their largest magnitude (`pair_share`);
  * consecutive losses differ;
  * the interaction weight differs between state0 and state1; for FwFM so do interaction_weight.bias and the linear
    part's parameters.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=23, emb_scale=1e3,
             emb_scale_max=1e6, optimizer="adam", regularizer=0)
_FMFM = dict(_BASE, model="FmFM", field_interaction_type="matrixed")
_FWFM = dict(_BASE, model="FwFM", linear_type="FiLV")
CASES = [
    dict(_FMFM, name="fmfm_matrixed_adam", embedding_dim=8),
    # the reference's default D = 10 over 9 fields (7 sparse + 2 dense): the kernels' 4-byte arm; SGD with a
    # regularizer, which reaches the bare Parameter as a net parameter
    dict(_FMFM, name="fmfm_matrixed_d10_sgd", embedding_dim=10, n_dense=2, optimizer="SGD", lr=5e-2,
         regularizer=1e-4),
    dict(_FMFM, name="fmfm_vectorized", embedding_dim=8, field_interaction_type="vectorized"),
    # two fields: one pair
    dict(_FMFM, name="fmfm_two_fields", embedding_dim=8, n_dense=0, cards=[37, 211]),
    dict(_FWFM, name="fwfm_filv_adam", embedding_dim=8),
    dict(_FWFM, name="fwfm_felv_sgd", embedding_dim=10, linear_type="FeLV", optimizer="SGD", lr=5e-2),
    dict(_FWFM, name="fwfm_lw", embedding_dim=8, linear_type="LW"),
    # the hyper-parameters of the zoo's own FmFM_test / FwFM_test (model_zoo/F{m,w}FM/config/model_config.yaml)
    dict(_FMFM, name="fmfm_zoo_test", embedding_dim=4, lr=1e-3),
    dict(_FWFM, name="fwfm_zoo_test", embedding_dim=4, regularizer=1e-8, lr=1e-3),
]


def build_reference(case, fmap):
    kw = dict(model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
              optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
              metrics=["logloss", "AUC"], verbose=0, model_root=TMP, regularizer=case["regularizer"])
    if case["model"] == "FmFM":
        from model_zoo.FmFM.src.FmFM import FmFM
        return FmFM(fmap, field_interaction_type=case["field_interaction_type"], **kw)
    from model_zoo.FwFM.src.FwFM import FwFM
    return FwFM(fmap, linear_type=case["linear_type"], **kw)


def interaction_weight(model, case):
    return model.interaction_weight if case["model"] == "FmFM" else model.interaction_weight.weight


def must_move(case, keys):
    """state_dict keys that have to differ between state0 and state1"""
    if case["model"] == "FmFM":
        return ["interaction_weight"]
    return ["interaction_weight.weight", "interaction_weight.bias"] + \
        [k for k in keys if k.startswith("linear_weight_layer.")]


def probe(model, batch, case):
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        w = interaction_weight(model, case)
        kept = w.detach().clone()
        w.zero_()
        share = logit_share(forward()[0], logit0)
        w.copy_(kept)
    return logit0, p0, {"pair_share": share}


def finish(out, model, case, fmap):
    import numpy as np
    want = must_move(case, [k[7:] for k in out if k.startswith("state1/")])
    moved = [k for k in want if not np.array_equal(out["state1/" + k], out["state0/" + k])]
    assert moved == want, (case["name"], want, moved)
    return {"n_pairs": fmap.num_fields * (fmap.num_fields - 1) // 2, "moved": moved}


def run_case(case):
    # the interaction's tables alone: FwFM's FeLV keeps a second set of [V, D] tables under linear_weight_layer, which
    # counts as a weight and keeps its scale
    record_case(case, build_reference, probe, lambda shares, case: shares["pair_share"] >= 0.05, finish,
                is_table=lambda k: k.startswith("embedding_layer."))


if __name__ == "__main__":
    main(CASES, run_case)
