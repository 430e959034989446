"""Golden vectors of FiGNN from the REAL reference (model_zoo.FiGNN of reczoo/FuxiCTR), next to those of make_golden.py
and in the same layout (`state0/`, `batchN/`, `expect/{logit0,pred0,loss,logit1,pred1}`, `state1/`, `meta`), so that
conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_fignn.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

The reference's tables start at std 1e-4: h is then ~1e-4 everywhere, the graph is uniform and a fixture that ignores
the propagation would still pass.  The embedding tables are rescaled (`emb_scale`, doubled until the assertions hold,
at most `emb_scale_max`), never the weights; the scale that was used is kept in `meta`.  Asserted per case, on the
first recorded forward and the recorded steps:
  * zeroing every W_in (the messages) moves the logits by at least 5 % of their largest magnitude (`message_share`);
  * zeroing W_attn (a uniform graph) moves them at all where there are more than two fields (`graph_share` > 0; with
    two fields the soft-max has one neighbour and g = 1 whatever W_attn holds: the share is recorded as 0);
  * consecutive losses differ;
  * every parameter of `fignn.` and `fc.` differs between state0 and state1, except W_attn with two fields.
No parameter of FiGNN has a rounding-residue gradient (there is no normalisation in it), so every case keeps the
default clip of 10: `finish` records the smallest |gradient| maximum over the dense parameters of the reference's
last step (`min_dense_grad_max`, far above Adam's eps) to show it, and whether that step's clip was reached
(`max_norm_reached`, from the norm of the clipped gradients, `last_grad_norm`).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, logit_share, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 150, 90, 11, 5, 211]
_BASE = dict(model="FiGNN", n_dense=1, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=29, emb_scale=1e3,
             emb_scale_max=1e6, optimizer="adam", emb_reg=0, net_reg=0, gnn_layers=3, use_gru=True,
             use_residual=True, reuse_graph_layer=False)
CASES = [
    # the hyper-parameters of the zoo's own FiGNN_test (model_zoo/FiGNN/config/model_config.yaml)
    dict(_BASE, name="fignn_zoo_test", embedding_dim=4, gnn_layers=2, lr=1e-3, emb_reg=1e-8),
    # the Criteo-like arm: D = 16 (16-byte accesses), 3 layers, 8 fields of which one is numeric
    dict(_BASE, name="fignn_adam", embedding_dim=16),
    # one shared graph layer (its gradients sum over the layers) at the reference's default D = 10: the 4-byte arm
    dict(_BASE, name="fignn_reuse_d10_sgd", embedding_dim=10, reuse_graph_layer=True, optimizer="SGD", lr=1e-2),
    # the two other branches of FiGNN.py:163-171
    dict(_BASE, name="fignn_nogru_nores", embedding_dim=8, gnn_layers=2, use_gru=False, use_residual=False),
    # two fields: the soft-max over a single neighbour, g = 1
    dict(_BASE, name="fignn_two_fields", embedding_dim=8, gnn_layers=1, n_dense=0, cards=[37, 211]),
]


def build_reference(case, fmap):
    from model_zoo.FiGNN.src.FiGNN import FiGNN
    return FiGNN(fmap, model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
                 optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
                 metrics=["logloss", "AUC"], verbose=0, model_root=TMP, embedding_regularizer=case["emb_reg"],
                 net_regularizer=case["net_reg"], gnn_layers=case["gnn_layers"], use_gru=case["use_gru"],
                 use_residual=case["use_residual"], reuse_graph_layer=case["reuse_graph_layer"])


def _graph_layers(model, case):
    return [model.fignn.gnn] if case["reuse_graph_layer"] else list(model.fignn.gnn)


def probe(model, batch, case):
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        w_in = [m.W_in for m in _graph_layers(model, case)]
        kept = [w.detach().clone() for w in w_in]
        for w in w_in:
            w.zero_()
        message = logit_share(forward()[0], logit0)
        for w, k in zip(w_in, kept):
            w.copy_(k)
        wa = model.fignn.W_attn.weight
        kept = wa.detach().clone()
        wa.zero_()
        graph = logit_share(forward()[0], logit0)
        wa.copy_(kept)
    return logit0, p0, {"message_share": message, "graph_share": graph}


def accept(shares, case):
    two = len(case["cards"]) + case["n_dense"] == 2
    return shares["message_share"] >= 0.05 and (two or shares["graph_share"] > 0.0)


def finish(out, model, case, fmap):
    import numpy as np
    two = fmap.num_fields == 2
    want = [k[7:] for k in out if k.startswith("state1/") and k[7:].startswith(("fignn.", "fc."))
            and not (two and k[7:] == "fignn.W_attn.weight")]
    moved = [k for k in want if not np.array_equal(out["state1/" + k], out["state0/" + k])]
    assert moved == want, (case["name"], sorted(set(want) - set(moved)))
    gmax = [float(p.grad.abs().max()) for k, p in model.named_parameters()
            if k.startswith(("fignn.", "fc.")) and p.grad is not None and not (two and k == "fignn.W_attn.weight")]
    norm = float(sum(float(p.grad.pow(2).sum()) for p in model.parameters() if p.grad is not None) ** 0.5)
    return {"num_fields": fmap.num_fields, "min_dense_grad_max": min(gmax), "last_grad_norm": norm,
            "max_norm_reached": bool(norm >= case["max_norm"] * (1.0 - 1e-5))}


def run_case(case):
    record_case(case, build_reference, probe, accept, finish, is_table=lambda k: k.startswith("embedding_layer."))


if __name__ == "__main__":
    main(CASES, run_case)
