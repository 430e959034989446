"""Golden vectors of AOANet from the REAL reference (model_zoo.AOANet of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout, so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_aoanet.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

The interaction stack is a polynomial of degree layers + 1 in the embeddings: at the default 1e-4 initialisation it
contributes nothing, at large embeddings it swamps the sigmoid.  The probe asserts, on the REFERENCE's forward, that
max |gin(feat_emb)| is at most 10, and record_case doubles the tables from `emb_scale` until it is at least 1e-2 (it
asserts when `emb_scale_max` is used up); the value is kept in `meta["gin_absmax"]`.  One numeric field only: a numeric
field's embedding is its value times a weight of order 1, and three of them alone push the degree-4 stack past the
window; `emb_scale` 500 puts the tables at 0.05, next to it.  W starts as the identity, alpha and
h as all ones, which would hide an indexing error: the case moves them off (+ 0.1 randn) before state0 is taken.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
WINDOW = (1e-2, 10.0)
_BASE = dict(model="AOANet", n_dense=1, cards=CARDS, B=64, steps=3, lr=1e-3, max_norm=10.0, seed=7, emb_scale=500.0,
             emb_scale_max=64e3, optimizer="adam", dnn_hidden_units=[64, 64, 64], num_interaction_layers=3,
             num_subspaces=4)
CASES = [
    # the hyper-parameters of the zoo's own AOANet_test (model_zoo/AOANet/config/model_config.yaml)
    dict(_BASE, name="aoanet_zoo_test", embedding_dim=4, seed=2022),
    dict(_BASE, name="aoanet_adam", embedding_dim=8, num_subspaces=3, num_interaction_layers=2, lr=1e-2, seed=11,
         dnn_hidden_units=[32, 16]),
    dict(_BASE, name="aoanet_one_layer_sgd", embedding_dim=6, num_subspaces=5, num_interaction_layers=1, lr=5e-2,
         seed=17, optimizer="SGD", dnn_hidden_units=[32]),
]


def build_reference(case, fmap):
    import torch
    from model_zoo import AOANet
    model = AOANet(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                   optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                   metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                   embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                   dnn_hidden_units=case["dnn_hidden_units"], dnn_hidden_activations="ReLU",
                   num_interaction_layers=case["num_interaction_layers"], num_subspaces=case["num_subspaces"],
                   net_dropout=0, batch_norm=False)
    with torch.no_grad():
        for layer in model.gin.layers:
            for p in (layer.W, layer.alpha, layer.h):
                p.add_(0.1 * torch.randn_like(p))
    return model


def probe(model, batch, case):
    seen = []
    handle = model.gin.register_forward_hook(lambda m, inp, out: seen.append(float(out.detach().abs().max())))
    with probing(model, batch) as forward:
        logit0, p0 = forward()
    handle.remove()
    assert seen[-1] <= WINDOW[1], (case["name"], seen[-1])
    return logit0, p0, {"gin_absmax": seen[-1]}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: shares["gin_absmax"] >= WINDOW[0])


if __name__ == "__main__":
    main(CASES, run_case)
