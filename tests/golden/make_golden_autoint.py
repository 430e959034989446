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
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, _import_reference, make_batches, small_criteo_spec  # noqa: E402

OUT_DIR = os.environ.get("FX_GOLDEN_OUT") or HERE

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


def run_case(case):
    import numpy as np
    import torch
    from fuxictr.features import FeatureMap
    from fuxictr.pytorch.torch_utils import seed_everything
    from model_zoo import AutoInt
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
    model = AutoInt(fmap, model_id=name, gpu=-1, embedding_dim=case["embedding_dim"],
                    learning_rate=case["lr"], optimizer=case["optimizer"], loss="binary_crossentropy",
                    task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                    embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                    dnn_hidden_units=case["hidden"], attention_layers=case["layers"],
                    num_heads=case["heads"], attention_dim=case["attention_dim"],
                    layer_norm=case["layer_norm"], use_scale=case["use_scale"], use_wide=case["use_wide"],
                    use_residual=case["use_residual"])
    with torch.no_grad():        # make the (1e-4 std) tables matter: scale the tables, not the weights
        for k, p in model.named_parameters():
            if "embedding_layers" in k and "lr_layer" not in k and p.dim() == 2 and p.shape[0] > 1 \
                    and p.shape[1] > 1:
                p.mul_(case["emb_scale"])
            if "lr_layer" in k and "embedding_layers" in k and p.shape[0] > 1:
                p.mul_(1000.0)
    model._max_gradient_norm = case["max_norm"]
    logits, probs, outs = [], {}, {}
    model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))
    def keep(store, i, pick):
        def hook(module, inp, result):      # (returns None: a hook's return value would replace the output)
            if i not in store:
                store[i] = pick(result).detach().clone()
        return hook
    for i, layer in enumerate(model.self_attention):
        layer.dot_attention.register_forward_hook(keep(probs, i, lambda r: r[1]))
        layer.register_forward_hook(keep(outs, i, lambda r: r))
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
    # the fixture is not vacuous: the attention is neither uniform nor one-hot, the ReLU cuts some outputs
    F = spec["num_fields"]
    peaks, zeros = [], []
    for i in range(case["layers"]):
        peak = float((probs[i].max(dim=-1).values - 1.0 / F).median())
        zero = float((outs[i] == 0).float().mean())
        peaks.append(round(peak, 3))
        zeros.append(round(zero, 3))
        if i == 0:
            assert 0.05 <= peak <= 0.5, (name, i, peak)
        else:
            assert peak >= 0.01, (name, i, peak)
        assert 0.1 <= zero <= 0.9, (name, i, zero)
    out["expect/pred0"] = p0.numpy().reshape(-1).copy()
    out["expect/logit0"] = logits[-1].numpy().reshape(-1).copy()
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
    meta["attention_peak_median"] = peaks
    meta["relu_zero_share"] = zeros
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "peaks", peaks, "relu zeros", zeros, "->", path,
          os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
