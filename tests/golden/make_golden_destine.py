"""Golden vectors of DESTINE from the REAL reference (model_zoo.DESTINE of reczoo/FuxiCTR), next to those of
make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`,
`state1/`, `meta`), so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_destine.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must exercise both soft-maxes, so the generator asserts on the first recorded forward, from the input
of layer 0 and that layer's own weights:
  * the pairwise soft-max is neither uniform nor one-hot: the median over (sample, group, query) of
    max_j P - 1/F lies in [0.05, 0.5];
  * the unary soft-max is not uniform: the median over (sample, head) of max_f us - 1/F is >= 0.01.
The tables are rescaled (`emb_scale`) for that, never the weights.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
# W_unary's bias has a gradient that is zero in exact arithmetic (a constant added to a column of u leaves the soft-max
# over the fields alone), and so have the bias in front of a BatchNorm and, at one head, the biases of W_q and W_k
# (the whitening takes a constant off again).  What the reference computes there is the rounding residue of its own
# sums, far below Adam's eps = 1e-8, where Adam's step is lr * g / eps: pure rounding noise that no other order of the
# same sums reproduces (the torch-CPU emulation of tests/test_destine_host.py missed conftest.assert_weights_close in
# exactly those entries).  As in make_golden_bst.py, the Adam cases therefore train under a clip that IS reached:
# max_norm 1e-3 scales every gradient by c = 1e-3 / |g| before Adam sees it.  Adam's step does not depend on the scale
# of a gradient that stays above eps, so every real entry trains as before; the residue entries move c times as far,
# below the tolerance.
ADAM_CLIP = 1e-3
_BASE = dict(model="DESTINE", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=ADAM_CLIP, seed=7,
             emb_scale=1e4, optimizer="adam", layers=2, heads=2, use_scale=False, use_wide=True,
             residual_mode="each_layer", relu_before_att=False, batch_norm=False)
CASES = [
    # the hyper-parameters of the zoo's own DESTINE_test (model_zoo/DESTINE/config/model_config.yaml), wide part on
    dict(_BASE, name="destine_zoo_test", embedding_dim=4, attention_dim=4, hidden=[64, 32], lr=1e-3,
         use_scale=True, batch_norm=True),
    # (seed: three Adam steps through three layers amplify the reference's own fp32 rounding; with seed 7 the same
    # model with the attention layers computed in fp64 on the CPU ends 1e-3 away from the recorded logits, ten times
    # the tolerance of tests/zoo_cases.py, with seed 11 3e-5 — the seed was chosen by that probe, on the CPU:
    # tests/golden/probe_destine_fp64.py)
    dict(_BASE, name="destine_adam", embedding_dim=8, attention_dim=16, layers=3, hidden=[32, 16], seed=11),
    dict(_BASE, name="destine_last_layer_sgd", embedding_dim=8, attention_dim=8, heads=4, hidden=[],
         residual_mode="last_layer", optimizer="SGD", lr=5e-2, max_norm=10.0),
    dict(_BASE, name="destine_nores_relu", embedding_dim=8, attention_dim=8, heads=1, hidden=[32, 16],
         residual_mode=None, relu_before_att=True),
    # F hd = 40 is no multiple of A = 12: the groups start in the middle of a field
    dict(_BASE, name="destine_h3", embedding_dim=8, attention_dim=12, heads=3, hidden=[32, 16], use_scale=True),
]


def build_reference(case, fmap):
    import torch
    from model_zoo import DESTINE
    model = DESTINE(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"],
                    learning_rate=case["lr"], optimizer=case["optimizer"], loss="binary_crossentropy",
                    task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                    embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                    attention_dim=case["attention_dim"], num_heads=case["heads"],
                    attention_layers=case["layers"], dnn_hidden_units=case["hidden"], net_dropout=0,
                    att_dropout=0, relu_before_att=case["relu_before_att"], batch_norm=case["batch_norm"],
                    use_scale=case["use_scale"], use_wide=case["use_wide"], residual_mode=case["residual_mode"])
    with torch.no_grad():        # the wide part's one-column tables, which the rescaling leaves alone
        for k, p in model.named_parameters():
            if k.startswith("lr.") and "embedding_layers" in k and p.shape[0] > 1:
                p.mul_(1000.0)
    return model


def probe(model, batch, case):
    import torch
    seen = []
    layer = model.self_attns[0]
    handle = layer.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().clone()))
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        handle.remove()
        # the two soft-maxes of layer 0, as DisentangledSelfAttention.forward computes them
        x, H, hd = seen[0], layer.num_heads, layer.head_dim
        B, F = x.shape[0], x.shape[1]
        q, k = layer.W_q(x), layer.W_k(x)
        if layer.relu_before_att:
            q, k = q.relu(), k.relu()
        q, k = q.view(B * H, -1, hd), k.view(B * H, -1, hd)
        s = torch.bmm(q - q.mean(dim=1, keepdim=True), (k - k.mean(dim=1, keepdim=True)).transpose(1, 2))
        if layer.use_scale:
            s = s / hd ** 0.5
        pair = float((s.softmax(dim=2).max(dim=2).values - 1.0 / F).median())
        unary = float((layer.W_unary(x).softmax(dim=1).max(dim=1).values - 1.0 / F).median())
    assert 0.05 <= pair <= 0.5, (case["name"], pair)
    assert unary >= 0.01, (case["name"], unary)
    return logit0, p0, {"pair_peak_median": pair, "unary_peak_median": unary}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True)


if __name__ == "__main__":
    main(CASES, run_case)
