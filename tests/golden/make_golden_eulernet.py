"""Golden vectors of EulerNet from the REAL reference (model_zoo.EulerNet of reczoo/FuxiCTR), next to those of
make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`,
`meta`), so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_eulernet.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must be neither degenerate nor on a discontinuity.  Both are conditions on the REFERENCE's forward, asserted
by the probe on every interaction layer's input: max |ul| <= 20 (exp neither saturates nor dwarfs the dense path), and
for every layer after the first every element with r < 0 has |p| >= 1e-3, so that no fp32 reordering upstream can move
atan2 across its branch cut (the first layer's input is mu (cos E, sin E), which a kernel reproduces to the last bits).
The tables are scaled by `emb_scale` as everywhere, so that E is O(1) and the phases fill the circle.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="EulerNet", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-3, max_norm=10.0, seed=7, emb_scale=1e4,
             optimizer="adam", layer_norm=True)
CASES = [
    # the hyper-parameters of the zoo's own EulerNet_test (model_zoo/EulerNet/config/model_config.yaml) with both
    # dropouts at 0 and a smaller shape
    dict(_BASE, name="eulernet_zoo_test", embedding_dim=10, shape=[12], seed=2021),
    # the second layer has inshape == outshape: the eye initialisation
    dict(_BASE, name="eulernet_two_layers_sgd", embedding_dim=8, shape=[6, 6], layer_norm=False, optimizer="SGD",
         lr=5e-2),
    dict(_BASE, name="eulernet_d10_adam", embedding_dim=10, shape=[5, 7], lr=1e-2, seed=11),
]


def build_reference(case, fmap):
    from model_zoo import EulerNet
    return EulerNet(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                    optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                    metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                    embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                    shape=case["shape"], net_ex_dropout=0, net_im_dropout=0, layer_norm=case["layer_norm"])


def probe(model, batch, case):
    import torch
    seen = []
    handles = [layer.register_forward_pre_hook(lambda m, inp: seen.append((m, inp[0][0].detach(), inp[0][1].detach())))
               for layer in model.Euler_interaction_layers]
    with probing(model, batch) as forward:
        logit0, p0 = forward()
    for h in handles:
        h.remove()
    ul_absmax, cut_margin = 0.0, float("inf")
    for k, (m, r, p) in enumerate(seen):
        lam = 0.5 * torch.log(r ** 2 + p ** 2 + 1e-8).reshape(r.shape[0], -1, m.feature_dim).transpose(-2, -1)
        ul_absmax = max(ul_absmax, float((lam @ m.inter_orders + m.bias_lam).detach().abs().max()))
        if k > 0 and bool((r < 0).any()):
            cut_margin = min(cut_margin, float(p[r < 0].abs().min()))
    assert ul_absmax <= 20.0 and cut_margin >= 1e-3, (case["name"], ul_absmax, cut_margin)
    return logit0, p0, {"ul_absmax": ul_absmax, "cut_margin": min(cut_margin, 1e3)}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True)


if __name__ == "__main__":
    main(CASES, run_case)
