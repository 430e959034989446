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
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, _import_reference, make_batches, small_criteo_spec  # noqa: E402

OUT_DIR = os.environ.get("FX_GOLDEN_OUT") or HERE

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
    from model_zoo.FinalMLP.src import DualMLP, FinalMLP
    common = dict(model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                  optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                  metrics=["logloss", "AUC"], verbose=0, model_root=TMP,
                  embedding_regularizer=case.get("emb_reg", 0), net_regularizer=case.get("net_reg", 0),
                  mlp1_hidden_units=case["mlp1"], mlp2_hidden_units=case["mlp2"])
    if case["model"] == "DualMLP":
        return DualMLP(fmap, **common)
    return FinalMLP(fmap, use_fs=case["use_fs"], fs_hidden_units=case["fs_hidden"], fs1_context=case["fs1_context"],
                    fs2_context=case["fs2_context"], num_heads=case["num_heads"], **common)


def run_case(case):
    import numpy as np
    import torch
    from fuxictr.features import FeatureMap
    from fuxictr.pytorch.torch_utils import seed_everything
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
    model = build_reference(case, fmap)
    final = case["model"] == "FinalMLP"
    gated = final and case["use_fs"]
    gen = torch.Generator().manual_seed(case["seed"] + 1)
    with torch.no_grad():        # make the (1e-4 std) tables matter: scale the tables, not the weights
        for k, p in model.named_parameters():
            if "embedding_layers" in k and p.dim() == 2 and p.shape[0] > 1 and p.shape[1] > 1:
                p.mul_(case["emb_scale"])
            # the gates of a fresh model are exactly 1: move the context bias and the gate towers' biases
            if gated and (k.endswith("_ctx_bias") or ("_gate.mlp." in k and k.endswith(".bias"))):
                p.copy_(case["bias_std"] * torch.randn(p.shape, generator=gen))
    model._max_gradient_norm = case["max_norm"]
    logits, seen = [], {}
    model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))
    if gated:
        def keep(key):
            def hook(module, inp, result):      # (returns None: a hook's return value would replace the output)
                if key not in seen:
                    seen[key] = 2.0 * result.detach().clone()
            return hook
        model.fs_module.fs1_gate.register_forward_hook(keep("gate1"))
        model.fs_module.fs2_gate.register_forward_hook(keep("gate2"))
    rng = np.random.default_rng(case["seed"])
    batches = make_batches(rng, spec, case["B"], case["steps"] + 1)
    out = {}
    for k, v in model.state_dict().items():
        out["state0/" + k] = v.detach().cpu().numpy().copy()

    def to_torch(b):
        return {k: torch.from_numpy(v) for k, v in b.items()}
    model.eval()
    gate_spread, gate_share, bilinear_share = [], None, None
    with torch.no_grad():
        p0 = model.forward(to_torch(batches[-1]))["y_pred"]
        logit0 = logits[-1].clone()
        top = float(logit0.abs().max())
        if gated:
            gate_spread = [float((seen[k].max(dim=1).values - seen[k].min(dim=1).values).min())
                           for k in ("gate1", "gate2")]
            # the same forward with both gates replaced by ones (the tower's sigmoid by 0.5)
            handles = [g.register_forward_hook(lambda m, i, r: torch.full_like(r, 0.5))
                       for g in (model.fs_module.fs1_gate, model.fs_module.fs2_gate)]
            model.forward(to_torch(batches[-1]))
            for h in handles:
                h.remove()
            gate_share = float((logits[-1] - logit0).abs().max() / top)
        if final:
            kept = model.fusion_module.w_xy.detach().clone()
            model.fusion_module.w_xy.zero_()
            model.forward(to_torch(batches[-1]))
            model.fusion_module.w_xy.copy_(kept)
            bilinear_share = float((logits[-1] - logit0).abs().max() / top)
    # the fixture is not vacuous
    for s in gate_spread:
        assert s >= 0.2, (name, "gate spread", gate_spread)
    assert gate_share is None or gate_share >= 0.05, (name, "gate share", gate_share)
    assert bilinear_share is None or bilinear_share >= 0.05, (name, "bilinear share", bilinear_share)
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
        if k.endswith("_ctx_bias"):
            assert not np.array_equal(out["state1/" + k], out["state0/" + k]), (name, k)
    for i, b in enumerate(batches):
        for k, v in b.items():
            out["batch%d/%s" % (i, k)] = v
    meta = dict(case)
    meta["spec"] = spec
    meta["torch"] = torch.__version__
    meta["gate_spread"] = [round(s, 3) for s in gate_spread]
    meta["gate_share"] = None if gate_share is None else round(gate_share, 3)
    meta["bilinear_share"] = None if bilinear_share is None else round(bilinear_share, 3)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "gate spread", meta["gate_spread"], "gate share", meta["gate_share"],
          "bilinear share", meta["bilinear_share"], "->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
