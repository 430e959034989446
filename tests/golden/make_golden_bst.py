"""Golden vectors of BST from the REAL reference (model_zoo.BST of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Run in the build container only (the reference does not travel to the GPU box):
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_bst.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else (tests/golden/check_regen.py compares with the committed files).

A fixture must exercise the masked soft-max, the LeakyReLU and the padding, so the generator asserts on the first
recorded forward and records in `meta`:
  * block 0, over the rows of unpadded queries with at least 3 open keys: the median of max_k P - 1 / (open keys)
    lies in [0.05, 0.5] (neither uniform nor one-hot).  P comes from a forward hook that calls the attention once
    more with need_weights (the model's own call discards it);
  * block 0: between 10 % and 90 % of the LeakyReLU's inputs are negative;
  * every batch holds an all-padding history, a full one and one with padding (rows 0 and 1 are overwritten).
The tables are rescaled (`emb_scale`) for that, never the weights.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, _import_reference, make_batches, pair_seq_spec, small_seq_spec  # noqa: E402

OUT_DIR = os.environ.get("FX_GOLDEN_OUT") or HERE

_BASE = dict(model="BST", B=64, steps=3, lr=1e-2, max_norm=10.0, seed=7, emb_scale=3e4, optimizer="adam",
             schema="small_seq", embedding_dim=8, heads=2, layers=1, pooling="mean", causal=False, layer_norm=True,
             use_residual=True, use_position_emb=True, hidden=[32, 16])
# The K third of attention.in_proj_bias has a gradient that is zero in exact arithmetic (a constant added to every key's
# score leaves the soft-max alone), and the K rows' entries at position columns that hardly vary nearly so.  What the
# reference computes there is the rounding residue of its own sums, ~1e-10, far below Adam's eps = 1e-8, where Adam's
# step is lr * g / eps: at the default clip (max_norm 10, never reached) three steps move such an entry by up to
# ~0.06 lr of pure rounding noise, which no other order of the same sums reproduces (the torch-CPU emulation of
# tests/test_bst_host.py and the HIP kernels both missed conftest.assert_weights_close in exactly those entries, and
# nowhere else).  The Adam cases therefore train under a clip that IS reached: max_norm 1e-3 scales every gradient
# by c = 1e-3 / |g| before Adam sees it.  Adam's step does not depend on the scale of a gradient that stays above
# eps, so every real entry trains as before (and the clip coefficient is now part of what the fixtures check); the
# residue entries move c times as far, below the tolerance.
ADAM_CLIP = 1e-3
CASES = [
    # two aligned histories: dm = 3 * 8 = 24, L1 = 6
    dict(_BASE, name="bst_pair_adam", schema="pair_seq", max_norm=ADAM_CLIP),
    # the hyper-parameters of the zoo's own BST_test (model_zoo/BST/config/model_config.yaml)
    dict(_BASE, name="bst_zoo_test", embedding_dim=4, heads=4, hidden=[64, 32], lr=1e-3, max_norm=ADAM_CLIP),
    dict(_BASE, name="bst_single_causal_sgd", causal=True, pooling="target", optimizer="SGD", lr=5e-2),
    # (the cases whose optimizer is free run SGD: the K third of in_proj_bias has a gradient that is zero in exact
    # arithmetic - a constant added to every key's score leaves the soft-max alone - and so have the K rows' entries
    # at position columns that hardly vary; under Adam such an entry moves by ~lr * noise / eps per step in the
    # reference itself, which no other summation order reproduces)
    dict(_BASE, name="bst_concat_two_layers", layers=2, pooling="concat", optimizer="SGD", lr=5e-2),
    dict(_BASE, name="bst_plain", schema="pair_seq", layer_norm=False, use_residual=False, use_position_emb=False,
         pooling="sum", heads=1, emb_scale=1.5e4, optimizer="SGD", lr=5e-2),      # (no position columns: the tables alone make the scores)
]


def fields_of(case):
    if case["schema"] == "pair_seq":
        return [["adgroup_id", "cate_id"]], [["click_sequence", "cate_sequence"]]
    return ["adgroup_id"], ["click_sequence"]


def run_case(case):
    import numpy as np
    import torch
    from fuxictr.features import FeatureMap
    from fuxictr.pytorch.torch_utils import seed_everything
    from model_zoo import BST
    name = case["name"]
    spec = pair_seq_spec(name) if case["schema"] == "pair_seq" else small_seq_spec(name)
    os.makedirs(os.path.join(TMP, name), exist_ok=True)
    fm_path = os.path.join(TMP, name, "feature_map.json")
    with open(fm_path, "w") as f:
        json.dump(spec, f)
    seed_everything(case["seed"])
    torch.set_num_threads(8)
    fmap = FeatureMap(name, os.path.join(TMP, name))
    fmap.load(fm_path, {"embedding_dim": case["embedding_dim"]})
    target, sequence = fields_of(case)
    as_field = lambda f: tuple(f) if isinstance(f, list) else f      # noqa: E731
    model = BST(fmap, model_id=name, gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=0, net_regularizer=0,
                dnn_hidden_units=case["hidden"], dnn_activations="relu", num_heads=case["heads"],
                stacked_transformer_layers=case["layers"], layer_norm=case["layer_norm"],
                use_residual=case["use_residual"], bst_target_field=[as_field(f) for f in target],
                bst_sequence_field=[as_field(f) for f in sequence], seq_pooling_type=case["pooling"],
                use_position_emb=case["use_position_emb"], use_causal_mask=case["causal"])
    with torch.no_grad():        # make the (1e-4 std) tables matter: scale the tables, not the weights
        for k, p in model.named_parameters():
            if "embedding_layers" in k and p.dim() == 2 and p.shape[0] > 1 and p.shape[1] > 1:
                p.mul_(case["emb_scale"])
    model._max_gradient_norm = case["max_norm"]
    logits, seen = [], {}
    model.output_activation.register_forward_pre_hook(lambda m, inp: logits.append(inp[0].detach().clone()))
    block0 = model.transformer_encoders[0].transformer_blocks[0]

    def attention_hook(module, args, kwargs, result):
        if "P" in seen or seen.get("busy"):
            return None
        seen["busy"] = True
        with torch.no_grad():
            _, P = module(*args, attn_mask=kwargs["attn_mask"], need_weights=True, average_attn_weights=False)
        seen["busy"] = False
        seen["P"], seen["mask"] = P.detach().clone(), kwargs["attn_mask"].detach().clone()
        return None
    block0.attention.register_forward_hook(attention_hook, with_kwargs=True)

    def lrelu_hook(module, inp):     # (returns None: a pre-hook's return value would replace the input)
        seen.setdefault("neg", float((inp[0] < 0).float().mean()))
    block0.ffn[1].register_forward_pre_hook(lrelu_hook)
    rng = np.random.default_rng(case["seed"])
    batches = make_batches(rng, spec, case["B"], case["steps"] + 1)
    seq_names = [n for item in spec["features"] for n, fs in item.items() if fs["type"] == "sequence"]
    first = seq_names[0] if case["schema"] != "pair_seq" else "click_sequence"
    for b in batches:            # row 0: an all-padding history, row 1: a full one
        for n in seq_names:
            b[n][0, :] = 0
            b[n][1, :] = np.where(b[n][1] == 0, 1 + (np.arange(b[n].shape[1]) % 5), b[n][1])
        lens = (b[first] != 0).sum(axis=1)
        L = b[first].shape[1]
        assert (lens == 0).any() and (lens == L).any() and ((lens > 0) & (lens < L)).any(), name
    out = {}
    for k, v in model.state_dict().items():
        out["state0/" + k] = v.detach().cpu().numpy().copy()

    def to_torch(b):
        return {k: torch.from_numpy(v) for k, v in b.items()}
    model.eval()
    with torch.no_grad():
        p0 = model.forward(to_torch(batches[-1]))["y_pred"]
    # the fixture is not vacuous
    H = case["heads"]
    P, mask = seen["P"], seen["mask"]                       # [B, H, L1, L1], [B * H, L1, L1] (True = masked)
    B, L1 = P.shape[0], P.shape[-1]
    open_keys = (~mask).view(B, H, L1, L1).sum(dim=-1)      # [B, H, L1]
    pad = torch.cat([torch.from_numpy(batches[-1][first] == 0), torch.zeros(B, 1, dtype=torch.bool)], dim=1)
    rows = (~pad).unsqueeze(1).expand(B, H, L1) & (open_keys >= 3)
    peak = float((P.max(dim=-1).values - 1.0 / open_keys.float())[rows].median())
    assert int(rows.sum()) >= 32, (name, int(rows.sum()))
    assert 0.05 <= peak <= 0.5, (name, peak)
    assert 0.1 <= seen["neg"] <= 0.9, (name, seen["neg"])
    out["expect/pred0"] = p0.numpy().reshape(-1).copy()
    out["expect/logit0"] = logits[-1].numpy().reshape(-1).copy()
    model.train()
    losses = []
    for i in range(case["steps"]):
        losses.append(float(model.train_step(to_torch(batches[i])).item()))
    assert all(a != b for a, b in zip(losses, losses[1:])), losses
    out["expect/loss"] = np.asarray(losses, dtype=np.float64)
    # the residue claim above, shown on the reference's own last gradient (as clipped; the ratio does not depend on
    # the clip): the K third of in_proj_bias against the Q third
    bias_grad = block0.attention.in_proj_bias.grad
    third = bias_grad.numel() // 3
    k_res, q_max = float(bias_grad[third:2 * third].abs().max()), float(bias_grad[:third].abs().max())
    assert k_res <= 1e-4 * q_max, (name, k_res, q_max)
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
    meta["bst_target"], meta["bst_sequence"] = target, sequence
    meta["attention_peak_median"] = round(peak, 3)
    # what departs from the reference's defaults, spelled out: fit()'s clip is 10
    meta["max_norm_default"] = 10.0
    meta["max_norm_reached"] = bool(case["max_norm"] < 10.0)
    meta["k_bias_grad_residue"] = [k_res, q_max]          # max |grad| of in_proj_bias's K third, of its Q third
    meta["attention_rows"] = int(rows.sum())
    meta["lrelu_negative_share"] = round(seen["neg"], 3)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", losses, "peak", round(peak, 3), "lrelu negatives", round(seen["neg"], 3), "->", path,
          os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    _import_reference()
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["name"] in only:
            run_case(case)
