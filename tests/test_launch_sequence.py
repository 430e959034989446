"""The embedding path's launch sequence, pinned on the kernel emulation (tests/_cpu_emul.py): which
of pack / de-dup / catch-up / gather / first-order launches a training step issues, in which order
and with which flags, for the four ways a model reaches `_TableGroup`.  The expected sequences in
tests/golden/launch_sequences.json are recorded data (this test body run on the code before the
per-batch state became an object): equality, no tolerance.  A second test stands in for the
captured step: packed matrices survive `keep_only_packs()`, de-dup results do not."""
import inspect
import json
import os

import pytest
import torch

import _cpu_emul
from conftest import GOLDEN
from test_host_wiring import _cpu_opt_init

WATCHED = ("pack_columns", "dedup", "dedup_catchup", "adam_catchup_rows", "emb_fm_fwd",
           "emb_gather_fwd", "emb_seq_pool_fwd", "lr_fwd")
FIXTURE = os.path.join(GOLDEN, "launch_sequences.json")
B, D = 8, 4


def _cat(name, vocab, **kw):
    return {name: dict({"source": "", "type": "categorical", "vocab_size": vocab}, **kw)}


CAT = [_cat("a", 16, padding_idx=0), _cat("b", 12), _cat("c", 9)]
SEQ = CAT + [
    {"hist": {"source": "", "type": "sequence", "padding_idx": 0, "vocab_size": 16, "max_len": 3,
              "feature_encoder": "layers.MaskedSumPooling()"}},
    {"raw": {"source": "", "type": "sequence", "padding_idx": 0, "vocab_size": 16, "max_len": 2,
             "share_embedding": "a", "feature_encoder": None}}]
TWO_DIMS = [_cat("a", 16, padding_idx=0), _cat("b", 12), _cat("c", 9, embedding_dim=1)]


def _spec(name, features):
    return {"dataset_id": name, "num_fields": len(features), "total_features": 0, "input_length": 0,
            "labels": ["y"], "features": features}


def _batches(features, steps=2):
    gen = torch.Generator().manual_seed(7)
    out = []
    for _ in range(steps):
        b = {"y": (torch.rand(B, generator=gen) > 0.5).float()}
        for item in features:
            (name, fs), = item.items()
            shape = (B, fs["max_len"]) if fs["type"] == "sequence" else (B,)
            b[name] = torch.randint(0, fs["vocab_size"], shape, generator=gen)
        out.append(b)
    return out


def _record(monkeypatch, log):
    """Wrap the emulated launches: each call appends [name, columns_sorted, grouped, want_uid,
    begin_scal is not None] (None where the launch has no such argument)."""
    import fuxictr_amd.ops as ops
    for name in WATCHED:
        fn = getattr(ops, name)
        sig = inspect.signature(fn)

        def wrapped(*a, _fn=fn, _sig=sig, _name=name, **k):
            args = _sig.bind(*a, **k)
            args.apply_defaults()
            args = args.arguments
            log.append([_name] + [bool(args[f]) if f in args else None
                                  for f in ("columns_sorted", "grouped", "want_uid")]
                       + [args["begin_scal"] is not None if "begin_scal" in args else None])
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)


def _model(case, tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import optim, zoo
    from fuxictr_amd.features import FeatureMap
    monkeypatch.setattr(optim._NativeOptimizer, "__init__", _cpu_opt_init(optim))
    features = {"deepfm_cat": CAT, "deepfm_seq": SEQ, "deepfm_cat_plain_dict": CAT,
                "two_dims": TWO_DIMS}[case]
    fmap = FeatureMap(case, str(tmp_path))
    fmap.load_dict(_spec(case, features), {"embedding_dim": D})
    common = dict(model_id=case, gpu=-1, embedding_dim=D, learning_rate=1e-3, optimizer="adam",
                  loss="binary_crossentropy", task="binary_classification", metrics=["logloss"],
                  verbose=0, model_root=str(tmp_path))

    class SeqDeepFM(zoo.DeepFM):
        """DeepFM over a dict with a raw [B, L, D] entry: the raw positions are summed by torch."""

        def forward(self, inputs):
            X = self.get_inputs(inputs)
            d = self.embedding_layer.embedding_layer(X)
            emb = torch.stack([e if e.dim() == 2 else e.sum(dim=1) for e in d.values()], dim=1)
            logit = self.mlp(emb.flatten(start_dim=1), out_add=self.fm(X, emb))
            return {"y_pred": self.output_activation(logit)}

    torch.manual_seed(3)
    if case == "two_dims":
        model = zoo.DCNv2(fmap, num_cross_layers=1, parallel_dnn_hidden_units=[8], **common)
    else:
        model = (SeqDeepFM if case == "deepfm_seq" else zoo.DeepFM)(fmap, hidden_units=[8], **common)
    if case == "deepfm_cat_plain_dict":
        get_inputs = model.get_inputs
        monkeypatch.setattr(model, "get_inputs", lambda inputs, feature_source=None:
                            dict(get_inputs(inputs, feature_source)))
    model.train()
    return model, _batches(features)


@pytest.mark.parametrize("case", ["deepfm_cat", "deepfm_seq", "deepfm_cat_plain_dict", "two_dims"])
def test_launch_sequence_of_two_training_steps(case, tmp_path, monkeypatch):
    """(a) LR + FM over categorical columns: the fused front, the column fast path of the de-dup;
    (b) + a pooled sequence and a raw sequence that aliases a table: the generic de-dup, the
    catch-up-rows launch, gather + pooling + separate first-order launch; (c) model (a) on a plain
    dict batch: nothing is shared between the layers; (d) two embedding dims: two table groups, no
    fused front."""
    model, batches = _model(case, tmp_path, monkeypatch)
    log = []
    _record(monkeypatch, log)
    for b in batches:
        model.train_step(b)
    with open(FIXTURE) as fd:
        expect = json.load(fd)[case]
    assert log == expect


def test_second_forward_after_keep_only_packs_repacks_nothing_and_dedups_again(tmp_path, monkeypatch):
    """What the captured step relies on: after `keep_only_packs()` the batch still holds its packed
    id / dense matrices (the static buffers the graph reads), every other per-batch entry is gone."""
    import fuxictr_amd.layers as nat
    model, batches = _model("deepfm_cat", tmp_path, monkeypatch)
    X = nat.FeatureDict(model.get_inputs(batches[0]))
    X._fx_ready = True
    log = []
    _record(monkeypatch, log)
    model.forward(X)
    first = [(key, ids, dense) for key, _, _, ids, dense in X.cache.packs()]
    assert first and nat.FeatureEmbeddingDict.packed_ids(X, "b").data_ptr() == \
        first[0][1][:, 1].data_ptr()
    n_pack = sum(e[0] == "pack_columns" for e in log)
    n_dedup = sum(e[0] in ("dedup", "dedup_catchup") for e in log)
    assert n_pack >= 1 and n_dedup == 1
    model.forward(X)                                     # same batch, nothing dropped: all shared
    assert sum(e[0] in ("dedup", "dedup_catchup") for e in log) == n_dedup
    X.cache.keep_only_packs()
    model.forward(X)
    again = [(key, ids, dense) for key, _, _, ids, dense in X.cache.packs()]
    assert [k for k, _, _ in again] == [k for k, _, _ in first]
    for (_, i0, d0), (_, i1, d1) in zip(first, again):
        assert (i0 is None) == (i1 is None) and (d0 is None) == (d1 is None)
        assert i0 is None or i0.data_ptr() == i1.data_ptr()
        assert d0 is None or d0.data_ptr() == d1.data_ptr()
    assert sum(e[0] == "pack_columns" for e in log) == n_pack
    assert sum(e[0] in ("dedup", "dedup_catchup") for e in log) == n_dedup + 1
