"""Golden vectors of FwFM and FmFM from the REAL reference (model_zoo.FwFM, model_zoo.FmFM of reczoo/FuxiCTR), next to
those of make_golden.py and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`,
`state1/`, `meta`), so that conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_pairfm.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

The reference's tables start at std 1e-4: every pair term is ~1e-8 and a fixture that ignores the interaction weight
would still pass.  The main embedding tables are rescaled (`emb_scale`, doubled until the assertions hold, at most
`emb_scale_max`), never the weights; the scale that was used is kept in `meta`.  Asserted per case, on the first
recorded forward and the recorded steps:
  * zeroing the interaction weight moves the logits by at least 5 % of their largest magnitude (`pair_share`);
  * consecutive losses differ;
  * the interaction weight differs between state0 and state1; for FwFM so do interaction_weight.bias and the linear
    part's parameters.
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
_BASE = dict(n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=23, emb_scale=1e3,
             emb_scale_max=1e6, optimizer="adam", regularizer=0)
_FMFM = dict(_BASE, model="FmFM", field_interaction_type="matrixed")
_FWFM = dict(_BASE, model="FwFM", linear_type="FiLV")
CASES = [
    dict(_FMFM, name="fmfm_matrixed_adam", embedding_dim=8),
    # the reference's default D = 10 over 9 fields (7 sparse + 2 dense): the kernels' 4-byte arm; SGD with a
    # regularizer, which reaches the bare Parameter as a net parameter
    dict(_FMFM, name="fmfm_matrixed_d10_sgd", embedding_dim=10, n_dense=2, optimizer="SGD", lr=5e-2,
         regularizer=1e-4),
    dict(_FMFM, name="fmfm_vectorized", embedding_dim=8, field_interaction_type="vectorized"),
    # two fields: one pair
    dict(_FMFM, name="fmfm_two_fields", embedding_dim=8, n_dense=0, cards=[37, 211]),
    dict(_FWFM, name="fwfm_filv_adam", embedding_dim=8),
    dict(_FWFM, name="fwfm_felv_sgd", embedding_dim=10, linear_type="FeLV", optimizer="SGD", lr=5e-2),
    dict(_FWFM, name="fwfm_lw", embedding_dim=8, linear_type="LW"),
    # the hyper-parameters of the zoo's own FmFM_test / FwFM_test (model_zoo/F{m,w}FM/config/model_config.yaml)
    dict(_FMFM, name="fmfm_zoo_test", embedding_dim=4, lr=1e-3),
    dict(_FWFM, name="fwfm_zoo_test", embedding_dim=4, regularizer=1e-8, lr=1e-3),
]


def build_reference(case, fmap):
    kw = dict(model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
              optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
              metrics=["logloss", "AUC"], verbose=0, model_root=TMP, regularizer=case["regularizer"])
    if case["model"] == "FmFM":
        from model_zoo.FmFM.src.FmFM import FmFM
        return FmFM(fmap, field_interaction_type=case["field_interaction_type"], **kw)
    from model_zoo.FwFM.src.FwFM import FwFM
    return FwFM(fmap, linear_type=case["linear_type"], **kw)


def interaction_weight(model, case):
    return model.interaction_weight if case["model"] == "FmFM" else model.interaction_weight.weight


def must_move(case, keys):
    """state_dict keys that have to differ between state0 and state1"""
    if case["model"] == "FmFM":
        return ["interaction_weight"]
    return ["interaction_weight.weight", "interaction_weight.bias"] + \
        [k for k in keys if k.startswith("linear_weight_layer.")]


def _probe(model, batch, case):
    """-> (logit0, pred0, pair_share) of one eval forward of `batch`"""
    import torch
    logits = []
    h_logit = model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))
    with torch.no_grad():
        p0 = model.forward(batch)["y_pred"]
        logit0 = logits[-1].clone()
        top = float(logit0.abs().max())
        w = interaction_weight(model, case)
        kept = w.detach().clone()
        w.zero_()
        model.forward(batch)
        w.copy_(kept)
        share = float((logits[-1] - logit0).abs().max() / top)
    h_logit.remove()
    return logit0, p0, share


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
    model._max_gradient_norm = case["max_norm"]
    rng = np.random.default_rng(case["seed"])
    batches = make_batches(rng, spec, case["B"], case["steps"] + 1)

    def to_torch(b):
        return {k: torch.from_numpy(v) for k, v in b.items()}
    tables = [p for k, p in model.named_parameters()
              if k.startswith("embedding_layer.") and p.dim() == 2 and p.shape[0] > 1 and p.shape[1] > 1]
    model.eval()
    scale = case["emb_scale"]
    with torch.no_grad():
        for p in tables:
            p.mul_(scale)
    while True:
        logit0, p0, share = _probe(model, to_torch(batches[-1]), case)
        if share >= 0.05:
            break
        assert scale * 2.0 <= case["emb_scale_max"], (name, scale, share)
        scale *= 2.0
        with torch.no_grad():
            for p in tables:
                p.mul_(2.0)
    out = {}
    for k, v in model.state_dict().items():
        out["state0/" + k] = v.detach().cpu().numpy().copy()
    logits = []
    model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))
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
    keys = list(model.state_dict().keys())
    for k, v in model.state_dict().items():
        out["state1/" + k] = v.detach().cpu().numpy().copy()
    want = must_move(case, keys)
    moved = [k for k in want if not np.array_equal(out["state1/" + k], out["state0/" + k])]
    assert moved == want, (name, want, moved)
    for i, b in enumerate(batches):
        for k, v in b.items():
            out["batch%d/%s" % (i, k)] = v
    meta = dict(case)
    meta["spec"] = spec
    meta["torch"] = torch.__version__
    meta["emb_scale_used"] = scale
    meta["n_pairs"] = fmap.num_fields * (fmap.num_fields - 1) // 2
    meta["moved"] = moved
    meta["pair_share"] = round(share, 3)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "scale", scale, "pair_share", round(share, 3), "moved", moved, "->", path,
          os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
