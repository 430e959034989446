"""Golden vectors of MaskNet from the REAL reference (model_zoo.MaskNet of reczoo/FuxiCTR), next to those of
make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`,
`state1/`, `meta`), so that conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_masknet.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must exercise the LayerNorms, their ReLUs and the mask, so the generator asserts on the first recorded
forward:
  * behind every LayerNorm + ReLU between 10 % and 90 % of the outputs are zero;
  * at least 90 % of the (sample, field) embedding vectors have a variance of at least 100 eps: the
    normalisation divides by the vectors' spread, not by sqrt(eps);
  * the mask matters: with every V_mask replaced by ones the logits move by at least 5 % of their largest
    magnitude;
  * consecutive losses differ.
The tables are rescaled (`emb_scale`) for that, never the weights.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 1500, 900, 11, 5, 211]
_BASE = dict(model="MaskNet", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=11,
             emb_scale=2e4, optimizer="adam", model_type="SerialMaskNet", num_blocks=1, block_dim=64, ratio=1,
             emb_layernorm=True, net_layernorm=True)
CASES = [
    dict(_BASE, name="masknet_serial_adam", embedding_dim=8, hidden=[32, 16], ratio=2),
    # D = 10: the kernels' scalar path; a fractional reduction ratio
    dict(_BASE, name="masknet_parallel_adam", embedding_dim=10, hidden=[32], model_type="ParallelMaskNet",
         num_blocks=3, block_dim=20, ratio=0.5),
    # the hyper-parameters of the zoo's own MaskNet_test (model_zoo/MaskNet/config/model_config.yaml)
    dict(_BASE, name="masknet_zoo_test", embedding_dim=4, hidden=[64, 32], lr=1e-3),
    # both LayerNorms off, SGD, a net regularizer: what the regularizer touches
    dict(_BASE, name="masknet_plain_sgd", embedding_dim=8, hidden=[32, 16], emb_layernorm=False,
         net_layernorm=False, optimizer="SGD", lr=5e-2, net_reg=1e-4, emb_scale=1e4),
]


def build_reference(case, fmap):
    from model_zoo import MaskNet
    return MaskNet(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"],
                   learning_rate=case["lr"], optimizer=case["optimizer"], loss="binary_crossentropy",
                   task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                   embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                   dnn_hidden_units=case["hidden"], model_type=case["model_type"],
                   parallel_num_blocks=case["num_blocks"], parallel_block_dim=case["block_dim"],
                   reduction_ratio=case["ratio"], emb_layernorm=case["emb_layernorm"],
                   net_layernorm=case["net_layernorm"])


def probe(model, batch, case):
    import torch
    name, seen = case["name"], {}

    def keep(key):
        def hook(module, inp, result):      # (returns None: a hook's return value would replace the output)
            seen[key] = result.detach().clone()
        return hook
    blocks = model.mask_net.mask_blocks
    handles = [model.embedding_layer.register_forward_hook(keep("emb"))]
    relu_keys = ["relu%d" % bi for bi in range(len(blocks))] if case["net_layernorm"] else []
    for key, block in zip(relu_keys, blocks):
        handles.append(block.hidden_layer[2].register_forward_hook(keep(key)))
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        for h in handles:
            h.remove()
        # the same forward with every V_mask replaced by ones
        handles = [block.mask_layer.register_forward_hook(lambda m, i, r: torch.ones_like(r)) for block in blocks]
        mask_share = logit_share(forward()[0], logit0)
        for h in handles:
            h.remove()
    relu_zero = [float((seen[k] == 0).float().mean()) for k in relu_keys]
    emb = seen["emb"]                                                    # [B, F, D]
    emb_var_share = float((emb.var(dim=-1, unbiased=False) >= 100 * 1e-5).float().mean())
    # the fixture is not vacuous
    for k, z in zip(relu_keys, relu_zero):
        assert 0.1 <= z <= 0.9, (name, k, z)
    assert emb_var_share >= 0.9, (name, emb_var_share)
    assert mask_share >= 0.05, (name, mask_share)
    return logit0, p0, {"relu_zero_share": relu_zero, "emb_var_share": emb_var_share, "mask_share": mask_share}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: True)


if __name__ == "__main__":
    main(CASES, run_case)
