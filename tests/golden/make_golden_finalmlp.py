"""Golden vectors of FinalMLP and DualMLP from the REAL reference (model_zoo.FinalMLP / model_zoo.DualMLP of
reczoo/FuxiCTR), next to those of make_golden.py and in the same layout (`state0/`, `batchN/`,
`expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_finalmlp.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

On a fresh model a gate without context features is exactly 1: `fsN_ctx_bias` is zero and the reference's
reset_parameters zeroes the Linear biases, so the gate tower's output is 0 and 2 sigmoid(0) = 1.  Before `state0` is
recorded the generator therefore perturbs `fsN_ctx_bias` and the gate towers' biases, and nothing else, with seeded
normal values; that perturbation is part of `state0`.

A fixture must exercise the gates and the bilinear head, so the generator asserts on the first recorded forward:
  * every gate 2 sigmoid(z) has a spread (max - min over its columns) of at least 0.2;
  * the gates matter: with both replaced by ones the logits move by at least 5 % of their largest magnitude;
  * the bilinear term matters: with w_xy zeroed the logits move by at least 5 % of their largest magnitude;
  * consecutive losses differ;
  * `fsN_ctx_bias` of `state1` differs from that of `state0`.
The tables are rescaled (`emb_scale`) for that, never the weights.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="FinalMLP", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=11,
             emb_scale=2e4, optimizer="adam", use_fs=True, fs_hidden=[16], fs1_context=[], fs2_context=[],
             num_heads=1, bias_std=1.0)
CASES = [
    # no context features: both gates are one row for the whole batch
    dict(_BASE, name="finalmlp_adam", embedding_dim=8, mlp1=[32, 16], mlp2=[32], num_heads=2),
    # both gates with context features; D = 10: W % 4 != 0, the kernels' scalar arm; SGD, a net regularizer
    dict(_BASE, name="finalmlp_ctx_sgd", embedding_dim=10, mlp1=[32, 16], mlp2=[32], fs1_context=["C2"],
         fs2_context=["C5", "C6"], optimizer="SGD", lr=5e-2, net_reg=1e-4),
    # one gate with context features and one without
    dict(_BASE, name="finalmlp_mixed", embedding_dim=8, mlp1=[32, 16], mlp2=[24, 32], fs1_context=["C1", "C4"],
         num_heads=2),
    # no feature selection; four heads over towers of unequal width (dxh = 6, dyh = 10)
    dict(_BASE, name="finalmlp_nofs_heads4", embedding_dim=8, mlp1=[32, 24], mlp2=[40], use_fs=False, num_heads=4),
    # the hyper-parameters of the zoo's own FinalMLP_test (model_zoo/FinalMLP/config/model_config.yaml); its context
    # fields userid / adgroup_id, cate_id stand at C1 / C2, C3 of this schema
    dict(_BASE, name="finalmlp_zoo_test", embedding_dim=4, mlp1=[64, 32], mlp2=[64, 64, 64], fs_hidden=[64, 64],
         fs1_context=["C1"], fs2_context=["C2", "C3"], num_heads=2, lr=1e-3),
    dict(_BASE, name="dualmlp_adam", model="DualMLP", embedding_dim=8, mlp1=[32, 16], mlp2=[24, 24, 8]),
]


def build_reference(case, fmap):
    import torch
    from model_zoo.FinalMLP.src import DualMLP, FinalMLP
    common = dict(model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                  optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                  metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                  embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                  mlp1_hidden_units=case["mlp1"], mlp2_hidden_units=case["mlp2"])
    if case["model"] == "DualMLP":
        return DualMLP(fmap, **common)
    model = FinalMLP(fmap, use_fs=case["use_fs"], fs_hidden_units=case["fs_hidden"], fs1_context=case["fs1_context"],
                     fs2_context=case["fs2_context"], num_heads=case["num_heads"], **common)
    gen = torch.Generator().manual_seed(case["seed"] + 1)
    with torch.no_grad():
        for k, p in model.named_parameters():
            # the gates of a fresh model are exactly 1: move the context bias and the gate towers' biases
            if case["use_fs"] and (k.endswith("_ctx_bias") or ("_gate.mlp." in k and k.endswith(".bias"))):
                p.copy_(case["bias_std"] * torch.randn(p.shape, generator=gen))
    return model


def probe(model, batch, case):
    import torch
    name = case["name"]
    final = case["model"] == "FinalMLP"
    gates = [model.fs_module.fs1_gate, model.fs_module.fs2_gate] if final and case["use_fs"] else []
    seen = []
    with probing(model, batch) as forward:
        handles = [g.register_forward_hook(lambda m, i, r: seen.append(2.0 * r.detach().clone())) for g in gates]
        logit0, p0 = forward()
        for h in handles:
            h.remove()
        gate_spread = [float((g.max(dim=1).values - g.min(dim=1).values).min()) for g in seen]
        gate_share, bilinear_share = None, None
        if gates:
            # the same forward with both gates replaced by ones (the tower's sigmoid by 0.5)
            handles = [g.register_forward_hook(lambda m, i, r: torch.full_like(r, 0.5)) for g in gates]
            gate_share = logit_share(forward()[0], logit0)
            for h in handles:
                h.remove()
        if final:
            kept = model.fusion_module.w_xy.detach().clone()
            model.fusion_module.w_xy.zero_()
            bilinear_share = logit_share(forward()[0], logit0)
            model.fusion_module.w_xy.copy_(kept)
    # the fixture is not vacuous
    for s in gate_spread:
        assert s >= 0.2, (name, "gate spread", gate_spread)
    assert gate_share is None or gate_share >= 0.05, (name, "gate share", gate_share)
    assert bilinear_share is None or bilinear_share >= 0.05, (name, "bilinear share", bilinear_share)
    return logit0, p0, {"gate_spread": gate_spread, "gate_share": gate_share, "bilinear_share": bilinear_share}


def finish(out, model, case, fmap):
    import numpy as np
    for k in [k[7:] for k in out if k.startswith("state1/") and k.endswith("_ctx_bias")]:
        assert not np.array_equal(out["state1/" + k], out["state0/" + k]), (case["name"], k)
    return {}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True, finish)


if __name__ == "__main__":
    main(CASES, run_case)
