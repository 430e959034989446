"""Golden vectors of DCN from the REAL reference (model_zoo.DCN of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_dcn.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

A fixture must exercise the cross weights, so the generator asserts on the first recorded forward:
  * the cross weights matter: with every cross `weight` zeroed the logits move by at least 5 % of their largest
    magnitude;
  * consecutive losses differ;
  * every cross `bias` and `weight` of `state1` differs from that of `state0`.
The tables are rescaled (`emb_scale`, doubled until the assertion holds, at most `emb_scale_max`) for that, never
the weights; the scale that was used is kept in `meta`.
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
_BASE = dict(model="DCN", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=23, emb_scale=2e3,
             emb_scale_max=1e6, optimizer="adam", embedding_dim=8, n_cross=3, dnn=[32, 16])
CASES = [
    dict(_BASE, name="dcn_adam"),
    # D = 10 over 9 fields (7 sparse + 2 dense): F * D = 90, no multiple of 4: the kernels' scalar arm; SGD with a net
    # regularizer, which the reference applies to every parameter outside the tables, the cross biases included
    dict(_BASE, name="dcn_d10_sgd", embedding_dim=10, n_dense=2, optimizer="SGD", lr=5e-2, net_reg=1e-4),
    # no tower: `dnn` is None and `fc` sits over the cross width alone
    dict(_BASE, name="dcn_cross_only", dnn=[]),
    # one cross layer: layer 0 is also the last
    dict(_BASE, name="dcn_one_layer", n_cross=1),
    # the hyper-parameters of the zoo's own DCN_test (model_zoo/DCN/DCN_torch/config/model_config.yaml; its
    # `crossing_layers` is no keyword of the class, so the default of 3 layers holds)
    dict(_BASE, name="dcn_zoo_test", embedding_dim=4, n_cross=3, dnn=[64, 32], emb_reg=1e-8, lr=1e-3),
]


def build_reference(case, fmap):
    from model_zoo.DCN.DCN_torch.src.DCN import DCN
    return DCN(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
               optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
               metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=case.get("emb_reg", 0),
               net_regularizer=case.get("net_reg", 0), dnn_hidden_units=case["dnn"], dnn_activations="relu",
               num_cross_layers=case["n_cross"])


def _probe(model, batch):
    """-> (logit0, pred0, w share) of one eval forward of `batch`"""
    import torch
    logits = []
    h_logit = model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))
    with torch.no_grad():
        p0 = model.forward(batch)["y_pred"]
        logit0 = logits[-1].clone()
        top = float(logit0.abs().max())
        # the same forward with every cross weight zeroed
        kept = [layer.weight.weight.detach().clone() for layer in model.crossnet.cross_net]
        for layer in model.crossnet.cross_net:
            layer.weight.weight.zero_()
        model.forward(batch)
        for layer, k in zip(model.crossnet.cross_net, kept):
            layer.weight.weight.copy_(k)
        w_share = float((logits[-1] - logit0).abs().max() / top)
    h_logit.remove()
    return logit0, p0, w_share


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
    assert (model.dnn is None) == (not case["dnn"])
    model._max_gradient_norm = case["max_norm"]
    rng = np.random.default_rng(case["seed"])
    batches = make_batches(rng, spec, case["B"], case["steps"] + 1)

    def to_torch(b):
        return {k: torch.from_numpy(v) for k, v in b.items()}
    tables = [p for k, p in model.named_parameters()
              if "embedding_layers" in k and p.dim() == 2 and p.shape[0] > 1 and p.shape[1] > 1]
    model.eval()
    # make the (1e-4 std) tables matter: scale the tables, not the weights, until the fixture is not vacuous
    scale = case["emb_scale"]
    with torch.no_grad():
        for p in tables:
            p.mul_(scale)
    while True:
        logit0, p0, w_share = _probe(model, to_torch(batches[-1]))
        if w_share >= 0.05:
            break
        assert scale * 2.0 <= case["emb_scale_max"], (name, scale, w_share)
        scale *= 2.0
        with torch.no_grad():
            for p in tables:
                p.mul_(2.0)
    assert w_share >= 0.05, (name, "w share", w_share)
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
    n_cross_keys = 0
    for k, v in model.state_dict().items():
        out["state1/" + k] = v.detach().cpu().numpy().copy()
        if k.startswith("crossnet.cross_net."):
            n_cross_keys += 1
            assert not np.array_equal(out["state1/" + k], out["state0/" + k]), (name, k)
    assert n_cross_keys == 2 * case["n_cross"], (name, n_cross_keys)
    for i, b in enumerate(batches):
        for k, v in b.items():
            out["batch%d/%s" % (i, k)] = v
    meta = dict(case)
    meta["spec"] = spec
    meta["torch"] = torch.__version__
    meta["emb_scale_used"] = scale
    meta["w_share"] = round(w_share, 3)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "scale", scale, "w share", meta["w_share"], "->", path,
          os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
