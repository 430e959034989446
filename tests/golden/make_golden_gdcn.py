"""Golden vectors of GDCN and GDCNP from the REAL reference (model_zoo.GDCN of reczoo/FuxiCTR), next to those of
make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`,
`meta`), so that conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_gdcn.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must exercise the gates and the cross weights, so the generator asserts on the first recorded forward:
  * sigmoid(Wg x) of every layer spans at least 0.2 over the batch (max - min over all its elements);
  * the gates matter: with every gate replaced by 0.5 the logits move by at least 5 % of their largest magnitude;
  * the cross weights matter: with every `w` zeroed the logits move by at least 5 % of their largest magnitude;
  * consecutive losses differ;
  * every `b.<i>` of `state1` differs from that of `state0`.
The tables are rescaled (`emb_scale`, doubled until the assertions hold, at most `emb_scale_max`) for that, never
the weights; the scale that was used is kept in `meta`.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="GDCN", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=17, emb_scale=2e3,
             emb_scale_max=1e6, optimizer="adam")
CASES = [
    dict(_BASE, name="gdcn_adam", embedding_dim=8, n_cross=3, dnn=[32, 16]),
    dict(_BASE, name="gdcnp_adam", model="GDCNP", embedding_dim=8, n_cross=2, dnn=[32, 24]),
    # D = 10 over 9 fields (7 sparse + 2 dense): F * D = 90, no multiple of 4: the kernels' scalar arm; SGD with a net
    # regularizer, which the reference applies to every parameter outside the tables, `b.<i>` included; smaller tables
    # (three [180, 90] pairs of cross weights already fill most of the size allowed to a fixture)
    dict(_BASE, name="gdcn_d10_sgd", embedding_dim=10, n_dense=2, cards=[37, 13, 300, 200, 11, 5, 101], n_cross=3,
         dnn=[32, 16], optimizer="SGD", lr=5e-2, net_reg=1e-4),
    # one cross layer: layer 0 is also the last
    dict(_BASE, name="gdcnp_one_layer", model="GDCNP", embedding_dim=8, n_cross=1, dnn=[32, 24]),
    # the hyper-parameters of the zoo's own GDCNP_test (model_zoo/GDCN/config/model_config.yaml; its `crossing_layers`
    # is no keyword of the class, so the default of 3 layers holds)
    dict(_BASE, name="gdcnp_zoo_test", model="GDCNP", embedding_dim=4, n_cross=3, dnn=[64, 32], emb_reg=1e-8, lr=1e-3),
]


def build_reference(case, fmap):
    from model_zoo.GDCN.src.GDCN import GDCN, GDCNP
    cls = GDCNP if case["model"] == "GDCNP" else GDCN
    return cls(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
               optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
               metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=case.get("emb_reg", 0),
               net_regularizer=case.get("net_reg", 0), dnn_hidden_units=case["dnn"], dnn_activations="relu",
               num_cross_layers=case["n_cross"])


def probe(model, batch, case):
    import torch
    gates = []
    with probing(model, batch) as forward:
        h_gate = model.cross_net.activation.register_forward_hook(lambda m, i, r: gates.append(r.detach().clone()))
        logit0, p0 = forward()
        h_gate.remove()
        spread = [float(g.max() - g.min()) for g in gates[:case["n_cross"]]]
        assert len(spread) == case["n_cross"], (case["name"], spread)
        # the same forward with every gate replaced by 0.5
        h_half = model.cross_net.activation.register_forward_hook(lambda m, i, r: torch.full_like(r, 0.5))
        gate_share = logit_share(forward()[0], logit0)
        h_half.remove()
        # ... and with every cross weight zeroed
        kept = [lin.weight.detach().clone() for lin in model.cross_net.w]
        for lin in model.cross_net.w:
            lin.weight.zero_()
        w_share = logit_share(forward()[0], logit0)
        for lin, k in zip(model.cross_net.w, kept):
            lin.weight.copy_(k)
    return logit0, p0, {"gate_spread": spread, "gate_share": gate_share, "w_share": w_share}


def accept(shares, case):
    return min(shares["gate_spread"]) >= 0.2 and shares["gate_share"] >= 0.05 and shares["w_share"] >= 0.05


def finish(out, model, case, fmap):
    import numpy as np
    for k in [k[7:] for k in out if k.startswith("state1/cross_net.b.")]:
        assert not np.array_equal(out["state1/" + k], out["state0/" + k]), (case["name"], k)
    return {}


def run_case(case):
    record_case(case, build_reference, probe, accept, finish)


if __name__ == "__main__":
    main(CASES, run_case)
