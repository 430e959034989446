"""Golden vectors of DCN from the REAL reference (model_zoo.DCN of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_dcn.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

A fixture must exercise the cross weights, so the generator asserts on the first recorded forward:
  * the cross weights matter: with every cross `weight` zeroed the logits move by at least 5 % of their largest
    magnitude;
  * consecutive losses differ;
  * every cross `bias` and `weight` of `state1` differs from that of `state0`.
The tables are rescaled (`emb_scale`, doubled until the assertion holds, at most `emb_scale_max`) for that, never
the weights; the scale that was used is kept in `meta`.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="DCN", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=23, emb_scale=2e3,
             emb_scale_max=1e6, optimizer="adam", embedding_dim=8, n_cross=3, dnn=[32, 16])
CASES = [
    dict(_BASE, name="dcn_adam"),
    # D = 10 over 9 fields (7 sparse + 2 dense): F * D = 90, no multiple of 4: the kernels' scalar arm; SGD with a net
    # regularizer, which the reference applies to every parameter outside the tables, the cross biases included
    dict(_BASE, name="dcn_d10_sgd", embedding_dim=10, n_dense=2, optimizer="SGD", lr=5e-2, net_reg=1e-4),
    # no tower: `dnn` is None and `fc` sits over the cross width alone
    dict(_BASE, name="dcn_cross_only", dnn=[]),
    # one cross layer: layer 0 is also the last
    dict(_BASE, name="dcn_one_layer", n_cross=1),
    # the hyper-parameters of the zoo's own DCN_test (model_zoo/DCN/DCN_torch/config/model_config.yaml; its
    # `crossing_layers` is no keyword of the class, so the default of 3 layers holds)
    dict(_BASE, name="dcn_zoo_test", embedding_dim=4, n_cross=3, dnn=[64, 32], emb_reg=1e-8, lr=1e-3),
]


def build_reference(case, fmap):
    from model_zoo.DCN.DCN_torch.src.DCN import DCN
    model = DCN(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=case.get("emb_reg", 0),
                net_regularizer=case.get("net_reg", 0), dnn_hidden_units=case["dnn"], dnn_activations="relu",
                num_cross_layers=case["n_cross"])
    assert (model.dnn is None) == (not case["dnn"])
    return model


def probe(model, batch, case):
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        # the same forward with every cross weight zeroed
        kept = [layer.weight.weight.detach().clone() for layer in model.crossnet.cross_net]
        for layer in model.crossnet.cross_net:
            layer.weight.weight.zero_()
        w_share = logit_share(forward()[0], logit0)
        for layer, k in zip(model.crossnet.cross_net, kept):
            layer.weight.weight.copy_(k)
    return logit0, p0, {"w_share": w_share}


def finish(out, model, case, fmap):
    import numpy as np
    cross = [k[7:] for k in out if k.startswith("state1/crossnet.cross_net.")]
    assert len(cross) == 2 * case["n_cross"], (case["name"], cross)
    for k in cross:
        assert not np.array_equal(out["state1/" + k], out["state0/" + k]), (case["name"], k)
    return {}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: shares["w_share"] >= 0.05, finish)


if __name__ == "__main__":
    main(CASES, run_case)
