"""Golden vectors of AFM from the REAL reference (model_zoo.AFM of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_afm.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

The reference's tables start at std 1e-4: every pair product is ~1e-8, every score equal, the attention uniform and
the fixture vacuous.  The tables are rescaled (`emb_scale`, doubled until the assertions hold, at most
`emb_scale_max`), never the weights; the scale that was used and the measured shares are kept in `meta`.  Asserted
on the first recorded forward and the recorded steps, for a case with attention over more than one pair:
  * in at least half of the samples the largest attention weight is at least twice the smallest (`att_ratio_share`);
  * replacing the attention by the uniform 1 / P moves the logits by at least 5 % of their largest magnitude
    (`att_share`);
  * zeroing `weight_p` moves the logits by at least 5 % of their largest magnitude (`wp_share`);
  * consecutive losses differ;
  * attention.0.weight, attention.0.bias, attention.2.weight and weight_p.weight differ between state0 and state1.
`afm_two_fields` has one pair: its softmax is 1 whatever the score and the attention's three parameters get a zero
gradient, so of these only the `weight_p` share, the losses and weight_p's change can hold and are asserted.
`afm_noatt` does not run the attention: there the pair sum itself must matter (zeroing the tables' second-order
part is the `pair_share`) and the losses differ.
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
_BASE = dict(model="AFM", n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=23, emb_scale=2e3,
             emb_scale_max=1e6, optimizer="adam", use_attention=True)
CASES = [
    dict(_BASE, name="afm_adam", embedding_dim=8, attention_dim=8),
    # the reference's defaults D = 10, A = 10 over 9 fields (7 sparse + 2 dense): F * D = 90, no multiple of 4: the
    # kernels' scalar arm; SGD with a net regularizer
    dict(_BASE, name="afm_d10_sgd", embedding_dim=10, attention_dim=10, n_dense=2, optimizer="SGD", lr=5e-2,
         net_reg=1e-4),
    dict(_BASE, name="afm_noatt", embedding_dim=8, attention_dim=8, use_attention=False),
    # two fields: one pair, a softmax over a single score
    dict(_BASE, name="afm_two_fields", embedding_dim=8, attention_dim=8, n_dense=0, cards=[37, 211]),
    # the hyper-parameters of the zoo's own AFM_test (model_zoo/AFM/config/model_config.yaml)
    dict(_BASE, name="afm_zoo_test", embedding_dim=4, attention_dim=8, emb_reg=1e-8, lr=1e-3),
]
ATT_KEYS = ["attention.0.weight", "attention.0.bias", "attention.2.weight", "weight_p.weight"]


def build_reference(case, fmap):
    from model_zoo.AFM.src.AFM import AFM
    return AFM(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
               optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
               metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=case.get("emb_reg", 0),
               net_regularizer=case.get("net_reg", 0), attention_dim=case["attention_dim"],
               attention_dropout=[0, 0], use_attention=case["use_attention"])


def _probe(model, batch, case):
    """-> (logit0, pred0, shares) of one eval forward of `batch`"""
    import torch
    logits, att = [], []
    h_logit = model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))
    shares = {}
    with torch.no_grad():
        h_att = model.attention.register_forward_hook(lambda m, i, r: att.append(r.detach().clone()))
        p0 = model.forward(batch)["y_pred"]
        h_att.remove()
        logit0 = logits[-1].clone()
        top = float(logit0.abs().max())
        if case["use_attention"]:
            a = att[-1].squeeze(-1)                                     # [B, P]
            if a.shape[1] > 1:
                ratio = a.max(dim=1).values / a.min(dim=1).values
                shares["att_ratio_share"] = float((ratio >= 2.0).float().mean())
                h_uni = model.attention.register_forward_hook(lambda m, i, r: torch.full_like(r, 1.0 / r.shape[1]))
                model.forward(batch)
                h_uni.remove()
                shares["att_share"] = float((logits[-1] - logit0).abs().max() / top)
            kept = model.weight_p.weight.detach().clone()
            model.weight_p.weight.zero_()
            model.forward(batch)
            model.weight_p.weight.copy_(kept)
            shares["wp_share"] = float((logits[-1] - logit0).abs().max() / top)
        else:
            # without the pair sum: the linear part alone
            shares["pair_share"] = float((model.lr_layer(model.get_inputs(batch)) - logit0).abs().max() / top)
    h_logit.remove()
    return logit0, p0, shares


def _enough(shares):
    floors = {"att_ratio_share": 0.5, "att_share": 0.05, "wp_share": 0.05, "pair_share": 0.05}
    return all(v >= floors[k] for k, v in shares.items())


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
        logit0, p0, shares = _probe(model, to_torch(batches[-1]), case)
        if _enough(shares):
            break
        assert scale * 2.0 <= case["emb_scale_max"], (name, scale, shares)
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
    for k, v in model.state_dict().items():
        out["state1/" + k] = v.detach().cpu().numpy().copy()
    n_pairs = fmap.num_fields * (fmap.num_fields - 1) // 2
    moved = [k for k in ATT_KEYS if not np.array_equal(out["state1/" + k], out["state0/" + k])]
    if case["use_attention"]:
        want = ATT_KEYS if n_pairs > 1 else ["weight_p.weight"]
        assert all(k in moved for k in want), (name, moved)
    for i, b in enumerate(batches):
        for k, v in b.items():
            out["batch%d/%s" % (i, k)] = v
    meta = dict(case)
    meta["spec"] = spec
    meta["torch"] = torch.__version__
    meta["emb_scale_used"] = scale
    meta["n_pairs"] = n_pairs
    meta["moved"] = moved
    for k, v in shares.items():
        meta[k] = round(v, 3)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "scale", scale, shares, "moved", moved, "->", path, os.path.getsize(path) // 1024,
          "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
