"""Golden vectors of FFMv2 and ONNv2 from the REAL reference (model_zoo.FFM.src.FFMv2, model_zoo.ONN.ONN_torch.src.ONNv2 of
reczoo/FuxiCTR), next to those of make_golden.py and in the same layout, so that conftest.Golden reads them.

Needs a checkout of the reference where make_golden.py looks for it (no test does); on the CPU:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/tests/golden/make_golden_ffm.py [case ...]
FX_GOLDEN_OUT=<dir> writes somewhere else.

The interaction is a polynomial of degree 2 of the tables: at the 1e-4 initialisation every pair term is ~1e-8 and a
fixture would pass with any slot rule.  The wide tables are rescaled (`emb_scale`, doubled until the probe's figure
reaches the window, at most `emb_scale_max`), never the weights.  The probe asserts, on the REFERENCE's forward, and
keeps in `meta["pair_absmax"]`:
    FFMv2: 1e-2 <= max |ffm_out| <= 10;     ONNv2: 1e-2 <= max |pair columns of dnn_input| and max |logit| <= 10.
A table row is F (or F - 1) times wider than usual, so the cardinalities are small.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden import TMP, main, probing, record_case  # noqa: E402

CARDS = [37, 13, 300, 180, 11, 5]
WINDOW = (1e-2, 10.0)
_BASE = dict(n_dense=3, cards=CARDS, B=64, steps=3, lr=1e-2, max_norm=10.0, seed=29, emb_scale=64.0,
             emb_scale_max=64.0 * 2 ** 12, optimizer="adam")
_FFM = dict(_BASE, model="FFMv2", regularizer=0)
_ONN = dict(_BASE, model="ONNv2", hidden_units=[32, 16], hidden_activations="relu", emb_reg=0, net_reg=0)
CASES = [
    dict(_FFM, name="ffmv2_adam", embedding_dim=4),
    # an odd embedding_dim over 8 fields: the kernels' 4-byte arms; SGD with the one regularizer that feeds both
    dict(_FFM, name="ffmv2_sgd", embedding_dim=3, n_dense=2, optimizer="SGD", lr=5e-2, regularizer=1e-4, seed=31),
    dict(_ONN, name="onnv2_adam", embedding_dim=4, seed=37),
    # the hyper-parameters of the zoo's own ONNv2_test (model_zoo/ONN/ONN_torch/config/model_config.yaml)
    dict(_ONN, name="onnv2_zoo_test", embedding_dim=2, hidden_units=[64, 32], lr=1e-3, seed=2019),
]


def build_reference(case, fmap):
    kw = dict(model_id=case["name"], gpu=-1, embedding_dim=case["embedding_dim"], learning_rate=case["lr"],
              optimizer=case["optimizer"], loss="binary_crossentropy", task="binary_classification",
              metrics=["logloss", "AUC"], verbose=0, model_root=TMP)
    if case["model"] == "FFMv2":
        from model_zoo.FFM.src.FFMv2 import FFMv2
        return FFMv2(fmap, regularizer=case["regularizer"], **kw)
    from model_zoo.ONN.ONN_torch.src.ONNv2 import ONNv2
    return ONNv2(fmap, embedding_regularizer=case["emb_reg"], net_regularizer=case["net_reg"],
                 hidden_units=case["hidden_units"], hidden_activations=case["hidden_activations"], net_dropout=0,
                 batch_norm=False, **kw)


def probe(model, batch, case):
    F, D = model.num_fields, model.embedding_dim
    with probing(model, batch) as forward:
        logit0, p0 = forward()
        emb = model.embedding_layer(model.get_inputs(batch))
        pairs = model.ffm_interaction(emb.view(-1, F, F - 1 if case["model"] == "FFMv2" else F, D))
    top = float(pairs.abs().max())
    assert top <= WINDOW[1] and float(logit0.abs().max()) <= WINDOW[1], (case["name"], top, float(logit0.abs().max()))
    return logit0, p0, {"pair_absmax": top}


def run_case(case):
    record_case(case, build_reference, probe, lambda shares, case: shares["pair_absmax"] >= WINDOW[0],
                is_table=lambda k: k.startswith("embedding_layer."))


if __name__ == "__main__":
    main(CASES, run_case)
