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
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, _import_reference, make_batches, small_criteo_spec  # noqa: E402

OUT_DIR = os.environ.get("FX_GOLDEN_OUT") or HERE

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


def run_case(case):
    import numpy as np
    import torch
    from fuxictr.features import FeatureMap
    from fuxictr.pytorch.torch_utils import seed_everything
    from model_zoo import FiBiNET
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
    model = FiBiNET(fmap, model_id=name, gpu=-1, embedding_dim=case["embedding_dim"],
                    learning_rate=case["lr"], optimizer=case["optimizer"], loss="binary_crossentropy",
                    task="binary_classification", metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                    embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                    hidden_units=case["hidden"], excitation_activation=case["excitation"],
                    reduction_ratio=case["ratio"], bilinear_type=case["bilinear_type"])
    with torch.no_grad():        # make the (1e-4 std) tables matter: scale the tables, not the weights
        for k, p in model.named_parameters():
            if "embedding_layers" in k and "lr_layer" not in k and p.dim() == 2 and p.shape[0] > 1 \
                    and p.shape[1] > 1:
                p.mul_(case["emb_scale"])
            if "lr_layer" in k and "embedding_layers" in k and p.shape[0] > 1:
                p.mul_(1000.0)
    model._max_gradient_norm = case["max_norm"]
    logits, seen = [], {}
    model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))

    def keep(key, pick):
        def hook(module, inp, result):      # (returns None: a hook's return value would replace the output)
            if key not in seen:
                seen[key] = pick(inp, result).detach().clone()
        return hook
    model.senet_layer.excitation[1].register_forward_hook(keep("hidden", lambda i, r: r))
    model.senet_layer.excitation.register_forward_hook(keep("gates", lambda i, r: r))
    model.dnn.register_forward_hook(keep("comb", lambda i, r: i[0]))
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
    meta["gate_zero_share"] = round(gate_zero, 3)
    meta["hidden_zero_share"] = round(hidden_zero, 3)
    meta["senet_branch_share"] = round(share, 3)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "gates zero", meta["gate_zero_share"], "hidden zero", meta["hidden_zero_share"],
          "senet share", meta["senet_branch_share"], "->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
