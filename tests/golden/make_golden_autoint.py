"""Golden vectors of AutoInt from the REAL reference (model_zoo.AutoInt of reczoo/FuxiCTR), next to those of
make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`,
`state1/`, `meta`), so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_autoint.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must exercise the soft-max and the ReLU, so the generator asserts on the first recorded forward:
  * layer 0: the median over (sample, head, query) of max_k P - 1/F lies in [0.05, 0.5] (neither uniform nor
    one-hot); every later layer: that median is >= 0.01;
  * per layer, between 10 % and 90 % of the outputs are zeroed by the ReLU.
The tables are rescaled (`emb_scale`) for that, never the weights.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="AutoInt", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=7,
             emb_scale=1e4, optimizer="adam", layers=3, heads=2, use_scale=False, use_wide=False,
             use_residual=True, layer_norm=False)
CASES = [
    # D != A: layer 0 has W_res, layers 1-2 an identity residual
    dict(_BASE, name="autoint_adam", embedding_dim=8, attention_dim=16, hidden=[32, 16]),
    # the hyper-parameters of the zoo's own AutoInt_test (model_zoo/AutoInt/config/model_config.yaml)
    dict(_BASE, name="autoint_zoo_test", embedding_dim=4, attention_dim=8, hidden=[64, 32], lr=1e-3,
         emb_reg=1e-8),
    dict(_BASE, name="autoint_scale_wide_sgd", embedding_dim=8, attention_dim=8, heads=1, layers=2,
         hidden=[32, 16], use_scale=True, use_wide=True, optimizer="SGD", lr=5e-2),
    # (without the residual the second layer's scores shrink: these tables are scaled a little further, so
    # that its attention stays away from uniform)
    dict(_BASE, name="autoint_nores_nodnn", embedding_dim=8, attention_dim=8, heads=4, layers=2,
         hidden=[], use_residual=False, emb_scale=1.6e4),
    dict(_BASE, name="autoint_layernorm", embedding_dim=8, attention_dim=8, layers=2, hidden=[32, 16],
         layer_norm=True),
]


def build_reference(case, fmap):
    import torch
    from model_zoo import AutoInt
    model = AutoInt(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"],
                    learning_rate=case["lr"], optimizer=case["optimizer"], loss="binary_crossentropy",
                    task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                    embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                    dnn_hidden_units=case["hidden"], attention_layers=case["layers"],
                    num_heads=case["heads"], attention_dim=case["attention_dim"],
                    layer_norm=case["layer_norm"], use_scale=case["use_scale"], use_wide=case["use_wide"],
                    use_residual=case["use_residual"])
    with torch.no_grad():        # the wide part's one-column tables, which the rescaling leaves alone
        for k, p in model.named_parameters():
            if "lr_layer" in k and "embedding_layers" in k and p.shape[0] > 1:
                p.mul_(1000.0)
    return model


def probe(model, batch, case):
    name, probs, outs, handles = case["name"], {}, {}, []

    def keep(store, i, pick):
        def hook(module, inp, result):      # (returns None: a hook's return value would replace the output)
            store[i] = pick(result).detach().clone()
        return hook
    for i, layer in enumerate(model.self_attention):
        handles.append(layer.dot_attention.register_forward_hook(keep(probs, i, lambda r: r[1])))
        handles.append(layer.register_forward_hook(keep(outs, i, lambda r: r)))
    with probing(model, batch) as forward:
        logit0, p0 = forward()
    for h in handles:
        h.remove()
    # the fixture is not vacuous: the attention is neither uniform nor one-hot, the ReLU cuts some outputs
    peaks, zeros = [], []
    for i in range(case["layers"]):
        F = probs[i].shape[-1]
        peak = float((probs[i].max(dim=-1).values - 1.0 / F).median())
        zero = float((outs[i] == 0).float().mean())
        peaks.append(peak)
        zeros.append(zero)
        if i == 0:
            assert 0.05 <= peak <= 0.5, (name, i, peak)
        else:
            assert peak >= 0.01, (name, i, peak)
        assert 0.1 <= zero <= 0.9, (name, i, zero)
    return logit0, p0, {"attention_peak_median": peaks, "relu_zero_share": zeros}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True)


if __name__ == "__main__":
    main(CASES, run_case)
