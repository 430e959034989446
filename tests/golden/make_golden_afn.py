"""Golden vectors of AFN from the REAL reference (model_zoo.AFN of reczoo/FuxiCTR), next to those of make_golden.py and
in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_afn.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fresh BatchNorm1d has running statistics (0, 1), under which the eval forward sees a = log|x| ~ -9.5 unnormalised and
exp(.) of it spans twenty orders of magnitude.  A fixture is therefore a checkpoint whose two logarithmic-net batch
norms have seen data: before `state0` is taken, the probe runs one training-mode forward of the probe batch with
momentum 1 (running statistics = that batch's), then puts momentum and the step counters back.

A fixture must not be degenerate, so the probe asserts on u = W . BN_log(log|x|) of that forward (the argument of exp):
0.05 <= std(u) <= 3 (exp neither constant nor saturating) and max |u| <= 20.  Xavier's coefficient_W gives std(u) ~ 1
and max |u| ~ 7, where a channel of c = exp(u) has a variance of several hundred and one fp32 ulp of
`exp_batch_norm.running_var` (6e-5 at 800) is already beyond conftest.assert_weights_close's absolute 2e-5.  The
generator therefore scales coefficient_W by `w_scale` = 0.3 (std(u) ~ 0.3, the variances O(1)); the tables are scaled by
`emb_scale` as everywhere.

`log_batch_norm.bias` has a gradient that is almost zero in exact arithmetic: a constant added to u[:, l, :] scales c,
and BN_exp takes that scale out again up to its eps.  What the reference computes there is mostly the rounding residue
of its own sums, where Adam's step is lr * g / (|g| + eps): noise that no other summation order reproduces.  As in
make_golden_bst.py and make_golden_destine.py, the Adam cases therefore train under a clip that IS reached
(max_norm 1e-3): Adam's step does not depend on the scale of a gradient that stays above eps, so every real entry
trains as before and the residue entries move c = 1e-3 / |g| times as far, below the tolerance.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
ADAM_CLIP = 1e-3
_BASE = dict(model="AFN", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=ADAM_CLIP, seed=7, emb_scale=1e4,
             w_scale=0.3, optimizer="adam", ensemble_dnn=False, batch_norm=False, dnn_hidden=[32, 16],
             afn_hidden=[32, 16])
CASES = [
    # the hyper-parameters of the zoo's own AFN_test (model_zoo/AFN/config/model_config.yaml): ensemble on
    dict(_BASE, name="afn_zoo_test", embedding_dim=4, neurons=8, lr=1e-3, ensemble_dnn=True, batch_norm=True),
    # (lr: the true gradient of log_batch_norm.bias is ~1e-4 of its neighbours' (BN_exp's eps / variance) and is
    # known to ~1e-3 of itself in fp32; where it still lies above Adam's eps after the clip, Adam turns that into
    # 1e-3 lr per step: at lr 1e-2 three steps of the HIP kernels ended 2.2e-5 from the reference's in 3 of 10 entries,
    # against conftest.assert_weights_close's 2e-5; at 1e-3 the same noise is 2e-6)
    dict(_BASE, name="afn_adam", embedding_dim=8, neurons=24, lr=1e-3),
    dict(_BASE, name="afn_sgd_bn", embedding_dim=8, neurons=16, optimizer="SGD", lr=5e-2, max_norm=10.0,
         batch_norm=True, ensemble_dnn=True),
    # L no multiple of 16, and the tables left at their initial 1e-4 scale: one value in fifteen lies under the clamp
    dict(_BASE, name="afn_l13_small", embedding_dim=8, neurons=13, emb_scale=1.0, optimizer="SGD", lr=5e-2,
         max_norm=10.0),
]


def build_reference(case, fmap):
    import torch
    from model_zoo import AFN
    model = AFN(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                ensemble_dnn=case["ensemble_dnn"], dnn_hidden_units=case["dnn_hidden"], dnn_dropout=0,
                afn_hidden_units=case["afn_hidden"], afn_dropout=0, logarithmic_neurons=case["neurons"],
                batch_norm=case["batch_norm"])
    with torch.no_grad():
        model.coefficient_W.weight.mul_(case["w_scale"])
    return model


def probe(model, batch, case):
    import torch
    norms = (model.log_batch_norm, model.exp_batch_norm)
    seen = []
    handle = model.coefficient_W.register_forward_hook(lambda m, inp, out: seen.append(out.detach().clone()))
    with torch.no_grad():                # the two batch norms see the probe batch once (see the module docstring)
        for bn in norms:
            bn.train()
            bn.momentum = 1.0
        model.logarithmic_net(model.embedding_layer(model.get_inputs(batch)))
        for bn in norms:
            bn.eval()
            bn.momentum = 0.1
            bn.num_batches_tracked.zero_()
    handle.remove()
    u = seen[0]
    u_std, u_absmax = float(u.std()), float(u.abs().max())
    assert 0.05 <= u_std <= 3.0 and u_absmax <= 20.0, (case["name"], u_std, u_absmax)
    clamped = float((model.embedding_layer(model.get_inputs(batch)).abs() < 1e-5).float().mean())
    with probing(model, batch) as forward:
        logit0, p0 = forward()
    return logit0, p0, {"u_std": u_std, "u_absmax": u_absmax, "clamped_share": clamped}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True)


if __name__ == "__main__":
    main(CASES, run_case)
