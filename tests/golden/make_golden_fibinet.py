"""Golden vectors of FiBiNET from the REAL reference (model_zoo.FiBiNET of reczoo/FuxiCTR), next to those of
make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`,
`state1/`, `meta`), so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_fibinet.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must exercise both ReLUs of the excitation and the SENet branch, so the generator asserts on the first
recorded forward:
  * ReLU excitation: between 10 % and 90 % of the gates A are zero;
  * between 10 % and 90 % of the inner ReLU's outputs are zero;
  * the SENet branch matters: max |tower(comb) - tower(comb with the SENet half zeroed)| is at least 5 % of
    max |tower(comb)|.
The tables are rescaled (`emb_scale`) for that, never the weights.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="FiBiNET", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=11,
             emb_scale=2e4, optimizer="adam", bilinear_type="field_interaction", excitation="ReLU", ratio=3)
CASES = [
    dict(_BASE, name="fibinet_adam", embedding_dim=8, hidden=[32, 16]),
    # the hyper-parameters of the zoo's own FiBiNET_test (model_zoo/FiBiNET/config/model_config.yaml)
    dict(_BASE, name="fibinet_zoo_test", embedding_dim=4, hidden=[64, 32], lr=1e-3, emb_reg=1e-8),
    dict(_BASE, name="fibinet_each_sigmoid_sgd", embedding_dim=8, hidden=[32, 16], bilinear_type="field_each",
         excitation="Sigmoid", optimizer="SGD", lr=5e-2),
    dict(_BASE, name="fibinet_all_nodnn", embedding_dim=8, hidden=[], bilinear_type="field_all", emb_scale=4e4),
]


def build_reference(case, fmap):
    import torch
    from model_zoo import FiBiNET
    model = FiBiNET(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"],
                    learning_rate=case["lr"], optimizer=case["optimizer"], loss="binary_crossentropy",
                    task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                    embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                    hidden_units=case["hidden"], excitation_activation=case["excitation"],
                    reduction_ratio=case["ratio"], bilinear_type=case["bilinear_type"])
    with torch.no_grad():        # the linear part's one-column tables, which the rescaling leaves alone
        for k, p in model.named_parameters():
            if "lr_layer" in k and "embedding_layers" in k and p.shape[0] > 1:
                p.mul_(1000.0)
    return model


def probe(model, batch, case):
    name, seen = case["name"], {}

    def keep(key, pick):
        def hook(module, inp, result):      # (returns None: a hook's return value would replace the output)
            seen[key] = pick(inp, result).detach().clone()
        return hook
    handles = [model.senet_layer.excitation[1].register_forward_hook(keep("hidden", lambda i, r: r)),
               model.senet_layer.excitation.register_forward_hook(keep("gates", lambda i, r: r)),
               model.dnn.register_forward_hook(keep("comb", lambda i, r: i[0]))]
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        for h in handles:
            h.remove()
        comb = seen["comb"]
        half = comb.shape[1] // 2
        plain = comb.clone()
        plain[:, half:] = 0
        full_out = model.dnn(comb)
        share = float((full_out - model.dnn(plain)).abs().max() / full_out.abs().max())
    gate_zero = float((seen["gates"] == 0).float().mean())
    hidden_zero = float((seen["hidden"] == 0).float().mean())
    # the fixture is not vacuous
    if case["excitation"] == "ReLU":
        assert 0.1 <= gate_zero <= 0.9, (name, gate_zero)
    assert 0.1 <= hidden_zero <= 0.9, (name, hidden_zero)
    assert share >= 0.05, (name, share)
    return logit0, p0, {"gate_zero_share": gate_zero, "hidden_zero_share": hidden_zero, "senet_branch_share": share}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True)


if __name__ == "__main__":
    main(CASES, run_case)
