"""Golden vectors of SAM (interaction_type SAM2A / SAM2E) from the REAL reference (model_zoo.SAM of reczoo/FuxiCTR), next
to those of make_golden.py and in the same layout, so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_sam.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

SAM is a pure polynomial of the embeddings (degree 4 for SAM2A / SAM2E, up to 3^layers for SAM3A / SAM3E): at the default 1e-4 initialisation the block
contributes nothing, at large embeddings it swamps the sigmoid.  The probe therefore asserts, on the REFERENCE's forward,
that max |logit - fc.bias| is at most 10, and record_case doubles the tables from `emb_scale` until it is at least 1e-2
(it asserts when `emb_scale_max` is used up); the value is kept in `meta["block_absmax"]`.  SAM2A's W starts at all ones, which would hide an indexing error: the case moves it
off them (1 + 0.1 randn) before state0 is taken.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
WINDOW = (1e-2, 10.0)
SCALE_3A, SCALE_3E = 500.0, 2700.0
_BASE = dict(model="SAM", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-3, max_norm=10.0, seed=7, emb_scale=1e3,
             emb_scale_max=64e3, optimizer="adam", aggregation="concat", num_interaction_layers=2, use_residual=False)
# (num_interaction_layers 2 and use_residual False are SAM_test's own values; SAM2A / SAM2E ignore both)
CASES = [
    # the hyper-parameters of the zoo's own SAM_test (model_zoo/SAM/config/model_config.yaml) with a larger
    # embedding_dim
    dict(_BASE, name="sam_zoo_test", interaction_type="SAM2E", embedding_dim=10, seed=2022),
    dict(_BASE, name="sam_2a_adam", interaction_type="SAM2A", embedding_dim=8, lr=1e-2, seed=11),
    # stacked layers are a polynomial of degree 3^layers: one doubling moves the logit by 2^9 / 2^27, so these cases
    # name the scale that lands in the window instead of searching for it
    dict(_BASE, name="sam_3a_weighted_res_adam", interaction_type="SAM3A", embedding_dim=8, lr=1e-2, seed=13,
         aggregation="weighted_pooling", use_residual=True, emb_scale=SCALE_3A, emb_scale_max=SCALE_3A),
    dict(_BASE, name="sam_3e_concat_sgd", interaction_type="SAM3E", embedding_dim=6, lr=5e-2, seed=17, optimizer="SGD",
         num_interaction_layers=3, emb_scale=SCALE_3E, emb_scale_max=SCALE_3E),
]


def build_reference(case, fmap):
    import torch
    from model_zoo import SAM
    model = SAM(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                interaction_type=case["interaction_type"], aggregation=case["aggregation"],
                num_interaction_layers=case["num_interaction_layers"], use_residual=case["use_residual"],
                net_dropout=0)
    with torch.no_grad():
        for layer in model.block.layers:
            if hasattr(layer, "W"):
                layer.W.add_(0.1 * torch.randn_like(layer.W))
    return model


def probe(model, batch, case):
    with probing(model, batch) as forward:
        logit0, p0 = forward()
    block = float((logit0 - model.fc.bias.detach()).abs().max())
    assert block <= WINDOW[1], (case["name"], block)
    if case["emb_scale_max"] == case["emb_scale"]:      # no search: the named scale has to land in the window
        assert block >= WINDOW[0], (case["name"], block)
    return logit0, p0, {"block_absmax": block}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: shares["block_absmax"] >= WINDOW[0])


if __name__ == "__main__":
    main(CASES, run_case)
