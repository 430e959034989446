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
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, _import_reference, make_batches, small_criteo_spec  # noqa: E402

OUT_DIR = os.environ.get("FX_GOLDEN_OUT") or HERE

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


def run_case(case):
    import numpy as np
    import torch
    from fuxictr.features import FeatureMap
    from fuxictr.pytorch.torch_utils import seed_everything
    from model_zoo import MaskNet
    name = case["name"]
    spec = small_criteo_spec(name, case["n_dense"], case["cards"])
    os.makedirs(os.path.join(TMP, name), exist_ok=True)
    fm_path = os.path.join(TMP, name, "feature_map.json")
    with open(fm_path, "w") as f:
        json.dump(spec, f)
    seed_everything(case["seed"])
    torch.set_num_threads(8)
    fmap = FeatureMap(name, os.path.join(TMP, name))
    fmap.load(fm_path, {"embedding_dim": case["embedding_dim"]})
    model = MaskNet(fmap, model_id=name, gpu=-1, embedding_dim=case["embedding_dim"],
                    learning_rate=case["lr"], optimizer=case["optimizer"], loss="binary_crossentropy",
                    task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                    embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                    dnn_hidden_units=case["hidden"], model_type=case["model_type"],
                    parallel_num_blocks=case["num_blocks"], parallel_block_dim=case["block_dim"],
                    reduction_ratio=case["ratio"], emb_layernorm=case["emb_layernorm"],
                    net_layernorm=case["net_layernorm"])
    with torch.no_grad():        # make the (1e-4 std) tables matter: scale the tables, not the weights
        for k, p in model.named_parameters():
            if "embedding_layers" in k and p.dim() == 2 and p.shape[0] > 1 and p.shape[1] > 1:
                p.mul_(case["emb_scale"])
    model._max_gradient_norm = case["max_norm"]
    logits, seen = [], {}
    model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))

    def keep(key, pick):
        def hook(module, inp, result):      # (returns None: a hook's return value would replace the output)
            if key not in seen:
                seen[key] = pick(inp, result).detach().clone()
        return hook
    model.embedding_layer.register_forward_hook(keep("emb", lambda i, r: r))
    relu_keys = []
    for bi, block in enumerate(model.mask_net.mask_blocks):
        if case["net_layernorm"]:
            block.hidden_layer[2].register_forward_hook(keep("relu%d" % bi, lambda i, r: r))
            relu_keys.append("relu%d" % bi)
    rng = np.random.default_rng(case["seed"])
    batches = make_batches(rng, spec, case["B"], case["steps"] + 1)
    out = {}
    for k, v in model.state_dict().items():
        out["state0/" + k] = v.detach().cpu().numpy().copy()

    def to_torch(b):
        return {k: torch.from_numpy(v) for k, v in b.items()}
    model.eval()
    with torch.no_grad():
        p0 = model.forward(to_torch(batches[-1]))["y_pred"]
        logit0 = logits[-1].clone()
        # the same forward with every V_mask replaced by ones
        handles = [block.mask_layer.register_forward_hook(lambda m, i, r: torch.ones_like(r))
                   for block in model.mask_net.mask_blocks]
        model.forward(to_torch(batches[-1]))
        for h in handles:
            h.remove()
        mask_share = float((logits[-1] - logit0).abs().max() / logit0.abs().max())
    relu_zero = [float((seen[k] == 0).float().mean()) for k in relu_keys]
    emb = seen["emb"]                                                    # [B, F, D]
    emb_var_share = float((emb.var(dim=-1, unbiased=False) >= 100 * 1e-5).float().mean())
    # the fixture is not vacuous
    for k, z in zip(relu_keys, relu_zero):
        assert 0.1 <= z <= 0.9, (name, k, z)
    assert emb_var_share >= 0.9, (name, emb_var_share)
    assert mask_share >= 0.05, (name, mask_share)
    out["expect/pred0"] = p0.numpy().reshape(-1).copy()
    out["expect/logit0"] = logit0.numpy().reshape(-1).copy()
    model.train()
    losses = []
    for i in range(case["steps"]):
        losses.append(float(model.train_step(to_torch(batches[i])).item()))
    assert all(a != b for a, b in zip(losses, losses[1:])), losses
    out["expect/loss"] = np.asarray(losses, dtype=np.float64)
    model.eval()
    with torch.no_grad():
        p1 = model.forward(to_torch(batches[-1]))["y_pred"]
    out["expect/pred1"] = p1.numpy().reshape(-1).copy()
    out["expect/logit1"] = logits[-1].numpy().reshape(-1).copy()
    for k, v in model.state_dict().items():
        out["state1/" + k] = v.detach().cpu().numpy().copy()
    for i, b in enumerate(batches):
        for k, v in b.items():
            out["batch%d/%s" % (i, k)] = v
    meta = dict(case)
    meta["spec"] = spec
    meta["torch"] = torch.__version__
    meta["relu_zero_share"] = [round(z, 3) for z in relu_zero]
    meta["emb_var_share"] = round(emb_var_share, 3)
    meta["mask_share"] = round(mask_share, 3)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "relu zero", meta["relu_zero_share"], "emb var share", meta["emb_var_share"],
          "mask share", meta["mask_share"], "->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
