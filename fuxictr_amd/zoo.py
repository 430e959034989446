"""The callers of the hot path that BASELINE.json's configs name — DeepFM, DCNv2, DIN, DLRM, xDeepFM —
and AutoInt, FiBiNET, MaskNet, FinalMLP, DualMLP, GDCN, GDCNP, AFM, DCN, FwFM, FmFM, BST, DIEN and FiGNN, on the native drop-in layers.  Constructor keywords, attribute (= state_dict) names and the forward
composition are the reference's (model_zoo/DeepFM/DeepFM_torch/src/DeepFM.py:41-88,
model_zoo/DCNv2/src/DCNv2.py:44-132, model_zoo/DIN/src/DIN.py:50-150, model_zoo/DLRM/src/DLRM.py:44-124,
model_zoo/xDeepFM/src/xDeepFM.py:41-97, model_zoo/AutoInt/src/AutoInt.py:49-119,
model_zoo/FiBiNET/src/FiBiNET.py:45-104,
model_zoo/MaskNet/src/MaskNet.py:51-123,
model_zoo/FinalMLP/src/FinalMLP.py:49-127, model_zoo/FinalMLP/src/DualMLP.py:44-101,
model_zoo/GDCN/src/GDCN.py:24-172, model_zoo/AFM/src/AFM.py:24-96,
model_zoo/DCN/DCN_torch/src/DCN.py:24-101, model_zoo/FwFM/src/FwFM.py:24-91,
model_zoo/FmFM/src/FmFM.py:25-94,
model_zoo/BST/src/BST.py:33-366,
model_zoo/DIEN/src/DIEN.py:27-503,
model_zoo/FiGNN/src/FiGNN.py:27-231), so its checkpoints and YAML configs apply unchanged.  These
classes exist because /root/reference does not travel to the GPU box; with the reference installed,
its own model_zoo classes run unmodified on the same layers through `fuxictr_amd.patch.install()`
(tests/test_dropin_reference_zoo.py).
"""
import os as _os

import torch
from torch import nn

from .layers import (AttentionLayer, AttentionalPrediction, BehaviorTransformer, FiGNN_Layer, DynamicGRU, GRU, MaskedSumPooling, BilinearInteractionV2, CompressedInteractionNet, CrossNet, CrossNetV2, DIN_Attention, Dice,
                     FactorizationMachine, FeatureEmbedding, FeatureEmbeddingDict, FeatureSelection, FieldLayerNorm,
                     FxLinear, GateCrossLayer, InnerProductInteraction, InteractionAggregation, LogisticRegression, MLP_Block, MultiHeadSelfAttention,
                     ParallelMaskNet, SerialMaskNet, SqueezeExcitation, _DlrmMixFn, _FiBiNETMixFn, _RecordGradSlot, din_record_layout,
                     _FMFn, afm_attention, afm_attention_native, pair_interaction, pair_interaction_native, side_by_side,
                     tower_pad)
from . import ops
from .rank_model import BaseModel


class _ZooModel(BaseModel):
    """Shared plumbing of the models: base-class construction and the closing
    compile / reset_parameters / model_to_device sequence every model_zoo ctor ends with."""

    def _base(self, feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs):
        BaseModel.__init__(self, feature_map, model_id=model_id, gpu=gpu,
                           embedding_regularizer=embedding_regularizer,
                           net_regularizer=net_regularizer, **kwargs)

    def _ready(self, kwargs, learning_rate):
        self.compile(kwargs["optimizer"], kwargs["loss"], learning_rate)
        self.reset_parameters()
        self.model_to_device()

    @staticmethod
    def _fused_flag(kwargs, env_name):
        """The model's `fused` keyword; without it the environment switch `env_name` (on unless "0")."""
        return bool(kwargs.get("fused", _os.environ.get(env_name, "1") != "0"))

    def _first_seq_ids(self, X, sequence, fallback):
        """The packed int32 ids of a pair's FIRST sequence field (0 = padding: the mask and the lengths, on the
        device); a batch that was not packed gets the model's own `fallback(X[name])`."""
        name = _fields(sequence)[0]
        ids = self.embedding_layer.packed_ids(X, name)
        return ids if ids is not None else fallback(X[name])

    def _tower(self, input_dim, units, activations, dropout, batch_norm, output_dim=1,
               output_activation=None):
        return MLP_Block(input_dim=input_dim, output_dim=output_dim, hidden_units=units,
                         hidden_activations=activations, output_activation=output_activation,
                         dropout_rates=dropout, batch_norm=batch_norm)


class DeepFM(_ZooModel):
    def __init__(self, feature_map, model_id="DeepFM", gpu=-1, learning_rate=1e-3,
                 embedding_dim=10, hidden_units=[64, 64, 64], hidden_activations="ReLU",
                 net_dropout=0, batch_norm=False, embedding_regularizer=None,
                 net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.fm = FactorizationMachine(feature_map)
        self.mlp = self._tower(feature_map.sum_emb_out_dim(), hidden_units, hidden_activations,
                               net_dropout, batch_norm)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # [B, F, D]
        logit = self.fm(X, emb)                             # first order + FM second order
        logit = self.mlp(emb.flatten(start_dim=1), out_add=logit)   # += in the head GEMM's epilogue
        return {"y_pred": self.output_activation(logit)}


class DCNv2(_ZooModel):
    _STRUCTURES = {"crossnet_only": (False, False), "stacked": (True, False),
                   "parallel": (False, True), "stacked_parallel": (True, True)}

    def __init__(self, feature_map, model_id="DCNv2", gpu=-1, model_structure="parallel",
                 use_low_rank_mixture=False, low_rank=32, num_experts=4, learning_rate=1e-3,
                 embedding_dim=10, stacked_dnn_hidden_units=[], parallel_dnn_hidden_units=[],
                 dnn_activations="ReLU", num_cross_layers=3, net_dropout=0, batch_norm=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        assert model_structure in self._STRUCTURES, \
            "model_structure={} not supported!".format(model_structure)
        if use_low_rank_mixture:
            raise NotImplementedError("CrossNetMix is outside the hot-path scope (SURVEY §2 #5)")
        self.model_structure = model_structure
        stacked, parallel = self._STRUCTURES[model_structure]
        width = feature_map.sum_emb_out_dim()
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.crossnet = CrossNetV2(width, num_cross_layers)
        head_in = 0 if stacked else width                   # what feeds `fc` from the cross branch
        if stacked:                                         # cross output -> DNN
            self.stacked_dnn = self._tower(width, stacked_dnn_hidden_units, dnn_activations,
                                           net_dropout, batch_norm, output_dim=None)
            head_in = stacked_dnn_hidden_units[-1]
        if parallel:                                        # embeddings -> DNN, next to the cross
            self.parallel_dnn = self._tower(width, parallel_dnn_hidden_units, dnn_activations,
                                            net_dropout, batch_norm, output_dim=None)
            head_in += parallel_dnn_hidden_units[-1]
        self.fc = FxLinear(head_in, 1, device=self.device)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        flat = self.embedding_layer(X, flatten_emb=True)    # [B, F*D]
        stacked, parallel = self._STRUCTURES[self.model_structure]
        fused = self._fused_parallel(flat) if (parallel and not stacked) else None
        if fused is not None:
            branch = fused                                   # [cross | deep], one buffer, no cat
        else:
            branch = self.crossnet(flat)
            if stacked:
                branch = self.stacked_dnn(branch)
            if parallel:
                branch = torch.cat([branch, self.parallel_dnn(flat)], dim=-1)
        return {"y_pred": self.output_activation(self.fc(branch))}

    def _fused_parallel(self, flat):
        """`parallel`: cross layer i and deep layer i as one grid (layers._CrossDeepFn) when the deep
        tower is a plain Linear / ReLU stack over 16-byte aligned rows; else None."""
        from .layers import _CrossDeepFn
        fz = getattr(self.parallel_dnn, "_fused", None)
        if fz is None or fz[1] or flat.dim() != 2 or flat.shape[1] % 4 or self.crossnet.num_layers < 1:
            return None
        stack = fz[0]
        if any(lin.weight.shape[0] % 4 for lin, _ in stack):
            return None
        wb = []
        for lin in self.crossnet.cross_layers:
            wb += [lin.weight, lin.bias]
        for lin, _ in stack:
            wb += [lin.weight, lin.bias]
        return _CrossDeepFn.apply(flat, self.crossnet.num_layers, tuple(r for _, r in stack), *wb)


def _fields(spec):
    """'a' | ('a','b') | ['a','b'] -> tuple of field names."""
    return tuple(spec) if isinstance(spec, (list, tuple)) else (spec,)


def _field_list(option):
    """A *_target_field / *_sequence_field / *_neg_seq_field option as the reference's public attribute: a list
    whose entries are a str, or a tuple for grouped fields."""
    return [tuple(f) if isinstance(f, list) else f for f in (option if isinstance(option, list) else [option])]


def _field_pairs(target_option, sequence_option, mismatch):
    """-> (targets, sequences), one entry per (target, sequence) pair; `mismatch` is the model's own assertion text."""
    targets, sequences = _field_list(target_option), _field_list(sequence_option)
    assert len(targets) == len(sequences), mismatch
    return targets, sequences


class DIN(_ZooModel):
    def __init__(self, feature_map, model_id="DIN", gpu=-1, dnn_hidden_units=[512, 128, 64],
                 dnn_activations="ReLU", attention_hidden_units=[64],
                 attention_hidden_activations="Dice", attention_output_activation=None,
                 attention_dropout=0, learning_rate=1e-3, embedding_dim=10, net_dropout=0,
                 batch_norm=False, din_target_field=[("item_id", "cate_id")],
                 din_sequence_field=[("click_history", "cate_history")], din_use_softmax=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.din_target_field, self.din_sequence_field = _field_pairs(
            din_target_field, din_sequence_field, "len(din_target_field) != len(din_sequence_field)")
        self.embedding_dim = embedding_dim
        self.embedding_layer = FeatureEmbeddingDict(feature_map, embedding_dim)
        self.attention_layers = nn.ModuleList(
            DIN_Attention(embedding_dim * len(_fields(t)), attention_units=attention_hidden_units,
                          hidden_activations=attention_hidden_activations,
                          output_activation=attention_output_activation,
                          dropout_rate=attention_dropout, use_softmax=din_use_softmax)
            for t in self.din_target_field)
        if isinstance(dnn_activations, str) and dnn_activations.lower() == "dice":
            dnn_activations = [Dice(units) for units in dnn_hidden_units]
        self.dnn = self._tower(feature_map.sum_emb_out_dim(), dnn_hidden_units, dnn_activations,
                               net_dropout, batch_norm, output_activation=self.output_activation)
        # the reference's configuration — one target field, one raw sequence that is the LAST feature —
        # runs the attention inside the gather record (layers._DinRecordFn): no cat / slice / add launches
        self._in_record = None
        names = list(feature_map.features)
        if (_os.environ.get("FX_DIN_INPLACE", "1") != "0" and len(self.din_target_field) == 1
                and isinstance(self.din_target_field[0], str)
                and isinstance(self.din_sequence_field[0], str)
                and names and names[-1] == self.din_sequence_field[0]
                and feature_map.features[names[-1]]["type"] == "sequence"
                and not feature_map.features[names[-1]].get("feature_encoder")):
            self._in_record = (self.din_target_field[0], self.din_sequence_field[0])
            self.embedding_layer.reserve_pooled_slot(self.din_sequence_field[0])
        self._ready(kwargs, learning_rate)

    def _record_layout(self, emb):
        """(rec, tslot, hole) when the embedding dict is ONE gather record laid out
        [single-slot fields.. | reserved | the sequence's positions]; None otherwise."""
        if self._in_record is None:
            return None
        return din_record_layout(emb, *self._in_record)

    def get_embedding(self, field, feature_emb_dict):
        names = _fields(field)
        if len(names) == 1:
            return feature_emb_dict[names[0]]
        return torch.cat([feature_emb_dict[f] for f in names], dim=-1)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # name -> [B,D] | [B,L,D]
        layout = self._record_layout(emb)
        if layout is not None:
            rec, tslot, hole = layout
            B, n_slots, D = rec.shape
            slot = _RecordGradSlot(B, n_slots, D, hole + 1, rec.device) if rec.requires_grad else None
            flat = self.attention_layers[0].forward_in_record(
                rec, self.embedding_layer.packed_ids(X, self._in_record[1]), tslot, hole, slot)
            if flat is not None:
                return {"y_pred": self.dnn(flat, dx_into=slot)}
        for attend, target, sequence in zip(self.attention_layers, self.din_target_field,
                                            self.din_sequence_field):
            seq_names = _fields(sequence)
            # padding_idx 0 marks the empty positions (DIN.py:125: `X[field].long() != 0`); the packed
            # int32 id columns themselves serve as the mask (kept when != 0): no cast / compare launches
            valid = self._first_seq_ids(X, sequence, lambda ids: ids.long() != 0)
            pooled = attend(self.get_embedding(target, emb), self.get_embedding(sequence, emb),
                            valid)
            # the attended vector replaces each sequence field's [B,L,D] entry by its [B,D] share
            for name, part in zip(seq_names, pooled.split(self.embedding_dim, dim=-1)):
                emb[name] = part
        return {"y_pred": self.dnn(self.embedding_layer.dict2tensor(emb, flatten_emb=True))}


class DLRM(_ZooModel):
    def __init__(self, feature_map, model_id="DLRM", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 top_mlp_units=[64, 64, 64], bottom_mlp_units=[64, 64, 64],
                 top_mlp_activations="ReLU", bottom_mlp_activations="ReLU", top_mlp_dropout=0,
                 bottom_mlp_dropout=0, interaction_op="dot", batch_norm=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        if interaction_op not in ("dot", "cat"):
            raise ValueError("interaction_op={} not supported.".format(interaction_op))
        self.interaction_op = interaction_op
        self.dense_feats = [name for name, spec in feature_map.features.items()
                            if spec["type"] == "numeric"]
        has_dense = len(self.dense_feats) > 0
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim,
                                                not_required_feature_columns=self.dense_feats)
        # the numeric features enter as ONE extra "field": the bottom MLP's embedding_dim output
        n_fields = feature_map.num_fields - len(self.dense_feats) + int(has_dense)
        if has_dense:
            self.bottom_mlp = self._tower(len(self.dense_feats), bottom_mlp_units,
                                          bottom_mlp_activations, bottom_mlp_dropout, batch_norm,
                                          output_dim=embedding_dim,
                                          output_activation=bottom_mlp_activations)
        if interaction_op == "dot":
            self.interact = InnerProductInteraction(num_fields=n_fields, output="inner_product")
            top_in = n_fields * (n_fields - 1) // 2 + embedding_dim * int(has_dense)
        else:
            self.interact = nn.Flatten(start_dim=1)
            top_in = n_fields * embedding_dim
        self.top_mlp = self._tower(top_in, top_mlp_units, top_mlp_activations, top_mlp_dropout,
                                   batch_norm, output_activation=self.output_activation)
        # native fast path of the reference's configuration (dot interaction + numeric features): the
        # bottom tower's vector becomes the last field of the gather record (layers._DlrmMixFn)
        self._in_record = False
        if (_os.environ.get("FX_DLRM_INPLACE", "1") != "0" and has_dense and interaction_op == "dot"
                and n_fields <= 32 and embedding_dim <= 32 and embedding_dim % 2 == 0):
            self._in_record = True
            self.embedding_layer.embedding_layer.reserve_tail_slots(1)
        self._ready(kwargs, learning_rate)

    def _forward_in_record(self, X, fields):
        """-> the top tower's input, or None when this forward cannot take the in-record path."""
        records = getattr(fields, "_fx_records", None)
        if not self._in_record or not records or len(records) != 1:
            return None
        rec, plan = records[0]
        B, n_slots, D = rec.shape
        if plan.tail0 != n_slots - 1 or fields.shape[1] != n_slots - 1 \
                or getattr(self.bottom_mlp, "_fused", None) is None or self.bottom_mlp._fused[1] \
                or self.bottom_mlp._fused[0][-1][0].out_features != D:
            return None
        groups = list(self.embedding_layer.embedding_layer._groups.values())
        dense_in = groups[0].pack_dense(X, self.dense_feats)     # one cast launch (none in a captured step)
        dest = rec.detach()[:, n_slots - 1, :]
        dense_vec = self.bottom_mlp(dense_in, out_into=dest)       # written into the record's last slot
        assert dense_vec.data_ptr() == dest.data_ptr()
        P = n_slots * (n_slots - 1) // 2
        # the top tower pads an unaligned input width itself (one cat): hand it the padded row instead
        return _DlrmMixFn.apply(rec, dense_vec, tower_pad(self.top_mlp, P + D))

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        fields = self.embedding_layer(X)                    # [B, Fs, D]
        mixed = self._forward_in_record(X, fields)
        if mixed is not None:
            return {"y_pred": self.top_mlp(mixed)}
        dense_vec = None
        if self.dense_feats:
            dense_in = torch.cat([X[name].float().view(-1, 1) for name in self.dense_feats], dim=-1)
            dense_vec = self.bottom_mlp(dense_in)           # [B, D]
            fields = torch.cat([fields, dense_vec.unsqueeze(1)], dim=1)
        mixed = self.interact(fields)
        if dense_vec is not None and self.interaction_op == "dot":
            mixed = torch.cat([mixed, dense_vec], dim=-1)
        return {"y_pred": self.top_mlp(mixed)}


class xDeepFM(_ZooModel):
    def __init__(self, feature_map, model_id="xDeepFM", gpu=-1, learning_rate=1e-3,
                 embedding_dim=10, dnn_hidden_units=[64, 64, 64], dnn_activations="ReLU",
                 cin_hidden_units=[16, 16, 16], net_dropout=0, batch_norm=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.dnn = None
        if dnn_hidden_units:
            self.dnn = self._tower(feature_map.sum_emb_out_dim(), dnn_hidden_units,
                                   dnn_activations, net_dropout, batch_norm)
        self.lr_layer = LogisticRegression(feature_map, use_bias=False)
        self.cin = CompressedInteractionNet(feature_map.num_fields, cin_hidden_units, output_dim=1)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)
        # linear part + explicit interactions (+ implicit ones): the sums ride in the GEMM epilogues
        logit = self.cin(emb, out_add=self.lr_layer(X))
        if self.dnn is not None:
            logit = self.dnn(emb.flatten(start_dim=1), out_add=logit)
        return {"y_pred": self.output_activation(logit)}


class AutoInt(_ZooModel):
    def __init__(self, feature_map, model_id="AutoInt", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 dnn_hidden_units=[64, 64, 64], dnn_activations="ReLU", attention_layers=2, num_heads=1,
                 attention_dim=8, net_dropout=0, batch_norm=False, layer_norm=False, use_scale=False,
                 use_wide=False, use_residual=True, embedding_regularizer=None, net_regularizer=None,
                 **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        if feature_map.num_fields > 64:
            raise NotImplementedError("AutoInt: {} fields, the fused self-attention takes fields <= 64"
                                      .format(feature_map.num_fields))
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.lr_layer = LogisticRegression(feature_map, use_bias=False) if use_wide else None
        self.dnn = self._tower(feature_map.sum_emb_out_dim(), dnn_hidden_units, dnn_activations,
                               net_dropout, batch_norm) if dnn_hidden_units else None
        # (AutoInt.py:89 hands net_dropout to the attention layers as well: > 0 raises there)
        self.self_attention = nn.Sequential(
            *[MultiHeadSelfAttention(embedding_dim if i == 0 else attention_dim,
                                     attention_dim=attention_dim, num_heads=num_heads,
                                     dropout_rate=net_dropout, use_residual=use_residual,
                                     use_scale=use_scale, layer_norm=layer_norm)
              for i in range(attention_layers)])
        self.fc = FxLinear(feature_map.num_fields * attention_dim, 1, device=self.device)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # [B, F, D]
        attended = self.self_attention(emb)                 # [B, F, A]
        # wide part + attention head (+ deep tower): the sums ride in the GEMM epilogues
        logit = self.lr_layer(X) if self.lr_layer is not None else None
        logit = self.fc(attended.flatten(start_dim=1), out_add=logit)
        if self.dnn is not None:
            logit = self.dnn(emb.flatten(start_dim=1), out_add=logit)
        return {"y_pred": self.output_activation(logit)}


class FiBiNET(_ZooModel):
    def __init__(self, feature_map, model_id="FiBiNET", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 hidden_units=[], hidden_activations="ReLU", excitation_activation="ReLU", reduction_ratio=3,
                 bilinear_type="field_interaction", net_dropout=0, batch_norm=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        num_fields = feature_map.num_fields
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.senet_layer = SqueezeExcitation(num_fields, reduction_ratio, excitation_activation)
        self.bilinear_interaction1 = BilinearInteractionV2(num_fields, embedding_dim, bilinear_type)
        self.bilinear_interaction2 = BilinearInteractionV2(num_fields, embedding_dim, bilinear_type)
        self.lr_layer = LogisticRegression(feature_map, use_bias=False)
        self.dnn = self._tower(num_fields * (num_fields - 1) * embedding_dim, hidden_units,
                               hidden_activations, net_dropout, batch_norm)
        # fused=False: the layers one after another, as the reference's class composes them behind
        # patch.install() (V = A * X, the two branch tensors and their cat in memory): the same numbers
        self._fused = self._fused_flag(kwargs, "FX_FIBINET_FUSED")
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # [B, F, D]
        if self._fused:
            width = 2 * self.bilinear_interaction1.interact_dim * emb.shape[2]
            # (the tower pads an unaligned input width itself, one cat: hand it the padded rows instead)
            pad = tower_pad(self.dnn, width)
            excite = self.senet_layer.excitation
            comb = _FiBiNETMixFn.apply(emb, excite[0].weight, excite[2].weight, self.senet_layer._act,
                                       self.bilinear_interaction1.bilinear_W,
                                       self.bilinear_interaction2.bilinear_W,
                                       ops.BILINEAR_TYPES[self.bilinear_interaction1.bilinear_type], pad)
        else:
            senet_emb = self.senet_layer(emb)
            comb = torch.cat([self.bilinear_interaction1(emb), self.bilinear_interaction2(senet_emb)],
                             dim=1).flatten(start_dim=1)
        # the linear part rides into the tower's head through the last GEMM's epilogue
        return {"y_pred": self.output_activation(self.dnn(comb, out_add=self.lr_layer(X)))}


class MaskNet(_ZooModel):
    def __init__(self, feature_map, model_id="MaskNet", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 dnn_hidden_units=[64, 64, 64], dnn_hidden_activations="ReLU", model_type="SerialMaskNet",
                 parallel_num_blocks=1, parallel_block_dim=64, reduction_ratio=1, embedding_regularizer=None,
                 net_regularizer=None, net_dropout=0, emb_layernorm=True, net_layernorm=True, **kwargs):
        if model_type not in ("SerialMaskNet", "ParallelMaskNet"):
            # (the reference leaves `mask_net` unset here and fails at the first forward, MaskNet.py:76-95)
            raise ValueError("model_type={} not supported: SerialMaskNet or ParallelMaskNet".format(model_type))
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        width = feature_map.num_fields * embedding_dim
        # the head's sigmoid sits inside `mask_net` as its output activation (MaskNet.py:79, 88), as DIN's does
        if model_type == "SerialMaskNet":
            self.mask_net = SerialMaskNet(input_dim=width, output_dim=1, output_activation=self.output_activation,
                                          hidden_units=dnn_hidden_units, hidden_activations=dnn_hidden_activations,
                                          reduction_ratio=reduction_ratio, dropout_rates=net_dropout,
                                          layer_norm=net_layernorm)
        else:
            self.mask_net = ParallelMaskNet(input_dim=width, output_dim=1, output_activation=self.output_activation,
                                            num_blocks=parallel_num_blocks, block_dim=parallel_block_dim,
                                            hidden_units=dnn_hidden_units, hidden_activations=dnn_hidden_activations,
                                            reduction_ratio=reduction_ratio, dropout_rates=net_dropout,
                                            layer_norm=net_layernorm)
        self.num_fields = feature_map.num_fields
        self.emb_norm = FieldLayerNorm(self.num_fields, embedding_dim) if emb_layernorm else None
        # fused=False: module by module, as the reference's class composes them (one LayerNorm launch per field and
        # their cat, V_mask * V_hidden as a tensor, LayerNorm and ReLU apart): the same numbers
        self._fused = self._fused_flag(kwargs, "FX_MASKNET_FUSED")
        self.mask_net.fused = self._fused
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # [B, F, D]
        flat = emb.flatten(start_dim=1)
        if self.emb_norm is None:
            V_hidden = flat
        elif self._fused:
            V_hidden = self.emb_norm(emb)                   # one grouped launch over the gather record
        else:
            V_hidden = torch.cat([norm(emb[:, i, :]) for i, norm in enumerate(self.emb_norm)], dim=1)
        return {"y_pred": self.mask_net(flat, V_hidden)}


class FinalMLP(_ZooModel):
    def __init__(self, feature_map, model_id="FinalMLP", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 mlp1_hidden_units=[64, 64, 64], mlp1_hidden_activations="ReLU", mlp1_dropout=0,
                 mlp1_batch_norm=False, mlp2_hidden_units=[64, 64, 64], mlp2_hidden_activations="ReLU",
                 mlp2_dropout=0, mlp2_batch_norm=False, use_fs=True, fs_hidden_units=[64], fs1_context=[],
                 fs2_context=[], num_heads=1, embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        feature_dim = embedding_dim * feature_map.num_fields
        self.mlp1 = self._tower(feature_dim, mlp1_hidden_units, mlp1_hidden_activations, mlp1_dropout,
                                mlp1_batch_norm, output_dim=None)
        self.mlp2 = self._tower(feature_dim, mlp2_hidden_units, mlp2_hidden_activations, mlp2_dropout,
                                mlp2_batch_norm, output_dim=None)
        self.use_fs = use_fs
        if self.use_fs:
            self.fs_module = FeatureSelection(feature_map, feature_dim, embedding_dim, fs_hidden_units, fs1_context,
                                              fs2_context)
        self.fusion_module = InteractionAggregation(mlp1_hidden_units[-1], mlp2_hidden_units[-1], output_dim=1,
                                                    num_heads=num_heads)
        # fused=False: module by module, as the reference's class composes them (the gate towers on B rows with their
        # Sigmoid, the gates and the gated records as tensors, the head from two Linears and broadcast matmuls): the
        # same numbers
        self._fused = self._fused_flag(kwargs, "FX_FINALMLP_FUSED")
        self.fusion_module.fused = self._fused
        if self.use_fs:
            self.fs_module.fused = self._fused
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        flat_emb = self.embedding_layer(X).flatten(start_dim=1)
        if self.use_fs:
            feat1, feat2 = self.fs_module(X, flat_emb)      # fused: both gates in one launch
        else:
            feat1, feat2 = flat_emb, flat_emb               # (no gate launch)
        y_pred = self.fusion_module(self.mlp1(feat1), self.mlp2(feat2))
        return {"y_pred": self.output_activation(y_pred)}


class DualMLP(_ZooModel):
    def __init__(self, feature_map, model_id="DualMLP", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 mlp1_hidden_units=[64, 64, 64], mlp1_hidden_activations="ReLU", mlp1_dropout=0,
                 mlp1_batch_norm=False, mlp2_hidden_units=[64, 64, 64], mlp2_hidden_activations="ReLU",
                 mlp2_dropout=0, mlp2_batch_norm=False, embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        feature_dim = embedding_dim * feature_map.num_fields
        self.mlp1 = self._tower(feature_dim, mlp1_hidden_units, mlp1_hidden_activations, mlp1_dropout,
                                mlp1_batch_norm)
        self.mlp2 = self._tower(feature_dim, mlp2_hidden_units, mlp2_hidden_activations, mlp2_dropout,
                                mlp2_batch_norm)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        flat_emb = self.embedding_layer(X).flatten(start_dim=1)
        # the second tower's logit rides into the first's head through the last GEMM's epilogue
        y_pred = self.mlp1(flat_emb, out_add=self.mlp2(flat_emb))
        return {"y_pred": self.output_activation(y_pred)}


def _gdcn_tower_units(name, dnn_hidden_units):
    if not dnn_hidden_units:
        # (the reference fails here too, but later and less clearly: GDCN leaves `dnn` None and its forward calls it,
        # GDCN.py:139-146, 165; GDCNP reads dnn_hidden_units[-1] for `fc`, GDCN.py:74: an IndexError)
        raise ValueError("{}: dnn_hidden_units is empty: the model needs its deep tower".format(name))
    return list(dnn_hidden_units)


class GDCN(_ZooModel):
    """The stacked form (GDCN.py:104-172): the deep tower, ending in the logit, over the gated cross network."""

    def __init__(self, feature_map, model_id="GDCN", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 dnn_hidden_units=[], dnn_activations="ReLU", num_cross_layers=3, net_dropout=0, batch_norm=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        units = _gdcn_tower_units("GDCN", dnn_hidden_units)
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        width = feature_map.sum_emb_out_dim()
        self.dnn = self._tower(width, units, dnn_activations, net_dropout, batch_norm, output_dim=1)
        self.cross_net = GateCrossLayer(width, num_cross_layers)
        # fused=False: module by module, as the reference's class composes it (two Linears per layer, the sigmoid, the
        # products and the sums as tensors): the same numbers
        self._fused = self._fused_flag(kwargs, "FX_GDCN_FUSED")
        self.cross_net.fused = self._fused
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        flat = self.embedding_layer(X, flatten_emb=True)    # [B, F*D]
        return {"y_pred": self.output_activation(self.dnn(self.cross_net(flat)))}


class GDCNP(_ZooModel):
    """The parallel form (GDCN.py:24-101): the gated cross network and the deep tower side by side, `fc` over both."""

    def __init__(self, feature_map, model_id="GDCNP", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 dnn_hidden_units=[], dnn_activations="ReLU", num_cross_layers=3, net_dropout=0, batch_norm=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        units = _gdcn_tower_units("GDCNP", dnn_hidden_units)
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        width = feature_map.sum_emb_out_dim()
        self.dnn = self._tower(width, units, dnn_activations, net_dropout, batch_norm, output_dim=None)
        self.cross_net = GateCrossLayer(width, num_cross_layers)
        self.fc = FxLinear(units[-1] + width, 1, device=self.device)
        self._fused = self._fused_flag(kwargs, "FX_GDCN_FUSED")
        self.cross_net.fused = self._fused
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        flat = self.embedding_layer(X, flatten_emb=True)    # [B, F*D]
        if not self._fused or self.cross_net.cn_layers < 1:
            both = torch.cat([self.cross_net(flat), self.dnn(flat)], dim=1)
        else:
            both = side_by_side(self.cross_net, self.dnn, flat, self.fc.in_features)
        return {"y_pred": self.output_activation(self.fc(both))}


class AFM(_ZooModel):
    """Attentional Factorization Machine (AFM.py:24-96): the attention over the pairwise products of the fields."""

    def __init__(self, feature_map, model_id="AFM", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 attention_dropout=[0, 0], attention_dim=10, use_attention=True, embedding_regularizer=None,
                 net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.use_attention = use_attention
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.product_layer = InnerProductInteraction(feature_map.num_fields, output="elementwise_product")
        self.lr_layer = LogisticRegression(feature_map, use_bias=True)
        self.attention = nn.Sequential(nn.Linear(embedding_dim, attention_dim), nn.ReLU(),
                                       nn.Linear(attention_dim, 1, bias=False), nn.Softmax(dim=1))
        self.weight_p = nn.Linear(embedding_dim, 1, bias=False)
        self.dropout1 = nn.Dropout(attention_dropout[0])
        self.dropout2 = nn.Dropout(attention_dropout[1])
        for lin in (self.attention[0], self.attention[2], self.weight_p):
            lin.__dict__["_fx_head_off"] = True             # none of them ends in the model's logit
        # fused=False: module by module, as the reference's class composes it (the [B, P, D] products, the hidden
        # tensor, the softmax and the weighted sum as tensors): the same numbers
        self._fused = self._fused_flag(kwargs, "FX_AFM_FUSED")
        self._native = afm_attention_native(feature_map.num_fields, embedding_dim, attention_dim)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # [B, F, D]
        drops = self.training and (self.dropout1.p > 0 or self.dropout2.p > 0)
        if self._fused and not self.use_attention and emb.shape[1] > 1:
            # the plain sum of all pair products is FM's second-order term; the linear part is its addend
            return {"y_pred": self.output_activation(_FMFn.apply(emb, self.lr_layer(X)))}
        if self._fused and self.use_attention and self._native and not drops:
            # ... and the fused node's addend: no separate add launch
            y_pred = afm_attention(emb, self.attention, self.weight_p, addend=self.lr_layer(X))
            return {"y_pred": self.output_activation(y_pred)}
        elementwise_product = self.product_layer(emb)       # [B, F (F - 1) / 2, D]
        if self.use_attention:
            attention_weight = self.dropout1(self.attention(elementwise_product))
            attention_sum = self.dropout2(torch.sum(attention_weight * elementwise_product, dim=1))
            afm_out = self.weight_p(attention_sum)
        else:
            afm_out = torch.flatten(elementwise_product, start_dim=1).sum(dim=-1).unsqueeze(-1)
        return {"y_pred": self.output_activation(self.lr_layer(X) + afm_out)}


class DCN(_ZooModel):
    """Deep & Cross Network (DCN.py:24-101): the rank-1 cross network next to the deep tower, `fc` over both; with
    `dnn_hidden_units` empty the cross network alone (`dnn` is None, DCN.py:64-76)."""

    def __init__(self, feature_map, model_id="DCN", gpu=-1, learning_rate=1e-3, embedding_dim=10,
                 dnn_hidden_units=[], dnn_activations="ReLU", num_cross_layers=3, net_dropout=0, batch_norm=False,
                 embedding_regularizer=None, net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        width = feature_map.sum_emb_out_dim()
        units = list(dnn_hidden_units) if dnn_hidden_units else []
        self.dnn = self._tower(width, units, dnn_activations, net_dropout, batch_norm, output_dim=None) \
            if units else None
        self.crossnet = CrossNet(width, num_cross_layers)
        self.fc = FxLinear(width + (units[-1] if units else 0), 1, device=self.device)
        # fused=False: module by module, as the reference's class composes it (per layer a Linear to one output, the
        # product, the two sums as tensors): the same numbers
        self._fused = self._fused_flag(kwargs, "FX_DCN_FUSED")
        self.crossnet.fused = self._fused
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        flat = self.embedding_layer(X, flatten_emb=True)    # [B, F*D]
        if self.dnn is None:
            both = self.crossnet(flat)
        elif not self.crossnet.native(flat):
            both = torch.cat([self.crossnet(flat), self.dnn(flat)], dim=-1)
        else:
            both = side_by_side(self.crossnet, self.dnn, flat, self.fc.in_features)
        return {"y_pred": self.output_activation(self.fc(both))}


class FwFM(_ZooModel):
    """Field-weighted Factorization Machine (FwFM.py:24-91): a trained scalar per field pair over the inner products,
    plus one of three linear parts."""

    def __init__(self, feature_map, model_id="FwFM", gpu=-1, learning_rate=1e-3, embedding_dim=10, regularizer=None,
                 linear_type="FiLV", **kwargs):
        self._base(feature_map, model_id, gpu, regularizer, regularizer, kwargs)      # one keyword feeds both
        interact_dim = int(feature_map.num_fields * (feature_map.num_fields - 1) / 2)
        self.interaction_weight = nn.Linear(interact_dim, 1)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.inner_product_layer = InnerProductInteraction(feature_map.num_fields, output="inner_product")
        self._linear_type = linear_type
        if linear_type == "LW":
            self.linear_weight_layer = FeatureEmbedding(feature_map, 1, use_pretrain=False)
        elif linear_type == "FeLV":
            self.linear_weight_layer = FeatureEmbedding(feature_map, embedding_dim)
        elif linear_type == "FiLV":
            self.linear_weight_layer = nn.Linear(feature_map.num_fields * embedding_dim, 1, bias=False)
            self.linear_weight_layer.__dict__["_fx_head_off"] = True
        else:
            raise NotImplementedError("linear_type={} is not supported.".format(linear_type))
        self.interaction_weight.__dict__["_fx_head_off"] = True
        # fused=False: module by module, as the reference's class composes it (the [B, P] inner products, the
        # Linear over them, the linear part and the sum as tensors): the same numbers
        self._fused = self._fused_flag(kwargs, "FX_PAIRFM_FUSED")
        self._native = pair_interaction_native(feature_map.num_fields, embedding_dim, "scalar")
        self._ready(kwargs, learning_rate)

    def _linear_part(self, X, feature_emb):
        if self._linear_type == "LW":
            return self.linear_weight_layer(X).sum(dim=1)
        if self._linear_type == "FeLV":
            return (feature_emb * self.linear_weight_layer(X)).sum((1, 2)).view(-1, 1)
        return self.linear_weight_layer(feature_emb.flatten(start_dim=1))

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        feature_emb = self.embedding_layer(X)               # [B, F, D]
        if self._fused and self._native:
            lin, bias = self.interaction_weight, self.interaction_weight.bias
            if self._linear_type == "FiLV":                 # pairs, linear part and bias: one launch
                y_pred = pair_interaction(feature_emb, lin.weight, "scalar", wlin=self.linear_weight_layer.weight,
                                          bias=bias)
            else:                                           # the second table's linear part rides as the addend
                y_pred = pair_interaction(feature_emb, lin.weight, "scalar", bias=bias,
                                          addend=self._linear_part(X, feature_emb))
            return {"y_pred": self.output_activation(y_pred)}
        poly2_part = self.interaction_weight(self.inner_product_layer(feature_emb))
        y_pred = poly2_part + self._linear_part(X, feature_emb)     # bias added in poly2_part
        return {"y_pred": self.output_activation(y_pred)}


class FmFM(_ZooModel):
    """Field-matrixed Factorization Machine (FmFM.py:25-94): a trained vector ("vectorized") or matrix ("matrixed")
    per field pair between the two embeddings."""

    def __init__(self, feature_map, model_id="FmFM", gpu=-1, learning_rate=1e-3, embedding_dim=10, regularizer=None,
                 field_interaction_type="matrixed", **kwargs):
        self._base(feature_map, model_id, gpu, regularizer, regularizer, kwargs)
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        num_fields = feature_map.num_fields
        interact_dim = int(num_fields * (num_fields - 1) / 2)
        self.field_interaction_type = field_interaction_type
        # a bare Parameter: reset_parameters() does not touch it, regularization_loss() counts it as a net parameter
        if field_interaction_type == "vectorized":
            self.interaction_weight = nn.Parameter(torch.Tensor(interact_dim, embedding_dim))
        elif field_interaction_type == "matrixed":
            self.interaction_weight = nn.Parameter(torch.Tensor(interact_dim, embedding_dim, embedding_dim))
        else:
            raise ValueError("field_interaction_type={} is not supported.".format(field_interaction_type))
        nn.init.xavier_normal_(self.interaction_weight)
        self.lr_layer = LogisticRegression(feature_map)
        self.triu_index = torch.triu_indices(num_fields, num_fields, offset=1).to(self.device)
        self._mode = "vector" if field_interaction_type == "vectorized" else "matrix"
        # fused=False: module by module, as the reference's class composes it (the two [B, P, D] gathers, the batched
        # product, the two sums as tensors): the same numbers
        self._fused = self._fused_flag(kwargs, "FX_PAIRFM_FUSED")
        self._native = pair_interaction_native(num_fields, embedding_dim, self._mode)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        feature_emb = self.embedding_layer(X)               # [B, F, D]
        if self._fused and self._native:
            # ... and lr_layer(X) is the fused node's addend: no separate add launch
            y_pred = pair_interaction(feature_emb, self.interaction_weight, self._mode, addend=self.lr_layer(X))
            return {"y_pred": self.output_activation(y_pred)}
        index = self.triu_index.to(feature_emb.device)
        left_emb = torch.index_select(feature_emb, 1, index[0])
        right_emb = torch.index_select(feature_emb, 1, index[1])
        if self.field_interaction_type == "vectorized":
            left_emb = left_emb * self.interaction_weight
        else:
            left_emb = torch.matmul(left_emb.unsqueeze(2), self.interaction_weight).squeeze(2)
        y_pred = (left_emb * right_emb).sum(dim=-1).sum(dim=-1, keepdim=True)
        y_pred = y_pred + self.lr_layer(X)
        return {"y_pred": self.output_activation(y_pred)}


class BST(_ZooModel):
    """Behavior Sequence Transformer (BST.py:33-245): per (target, sequence) pair a stack of transformer blocks over
    [history | target] with a trained position embedding, pooled over the positions, next to the other fields'
    embeddings in front of the DNN.  Each block is one fused launch per direction (layers.BehaviorTransformer)."""

    def __init__(self, feature_map, model_id="BST", gpu=-1, dnn_hidden_units=[256, 128, 64], dnn_activations="ReLU",
                 num_heads=2, stacked_transformer_layers=1, attention_dropout=0, learning_rate=1e-3, embedding_dim=10,
                 net_dropout=0, batch_norm=False, layer_norm=True, use_residual=True,
                 bst_target_field=[("item_id", "cate_id")], bst_sequence_field=[("click_history", "cate_history")],
                 seq_pooling_type="mean", use_position_emb=True, use_causal_mask=False, embedding_regularizer=None,
                 net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.bst_target_field, self.bst_sequence_field = _field_pairs(
            bst_target_field, bst_sequence_field, "len(self.bst_target_field) != len(self.bst_sequence_field)")
        if seq_pooling_type not in ("mean", "sum", "target", "concat"):
            raise ValueError("seq_pooling_type={} not supported.".format(seq_pooling_type))
        self.use_causal_mask = use_causal_mask
        self.seq_pooling_type = seq_pooling_type
        self.feature_map = feature_map
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.embedding_layer = FeatureEmbeddingDict(feature_map, embedding_dim)
        self.transformer_encoders = nn.ModuleList()
        seq_out_dim = 0
        for sequence_field in self.bst_sequence_field:
            names = _fields(sequence_field)
            model_dim = embedding_dim * (int(use_position_emb) + len(names))      # the position emb is concatenated
            seq_len = feature_map.features[names[0]]["max_len"] + 1                # + the target item
            seq_out_dim += self.get_seq_out_dim(model_dim, seq_len, sequence_field, embedding_dim)
            self.transformer_encoders.append(
                BehaviorTransformer(seq_len=seq_len, model_dim=model_dim, num_heads=num_heads,
                                    stacked_transformer_layers=stacked_transformer_layers,
                                    attn_dropout=attention_dropout, net_dropout=net_dropout,
                                    position_dim=embedding_dim, use_position_emb=use_position_emb,
                                    layer_norm=layer_norm, use_residual=use_residual))
        self.dnn = self._tower(feature_map.sum_emb_out_dim() + seq_out_dim, dnn_hidden_units, dnn_activations,
                               net_dropout, batch_norm, output_activation=self.output_activation)
        self._ready(kwargs, learning_rate)

    def get_seq_out_dim(self, model_dim, seq_len, sequence_field, embedding_dim):
        num_seq_field = len(sequence_field) if type(sequence_field) == tuple else 1
        if self.seq_pooling_type == "concat":
            return seq_len * model_dim - num_seq_field * embedding_dim
        return model_dim - num_seq_field * embedding_dim

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # name -> [B, D] | [B, L, D]
        pooled, dropped = [], set()
        for encoder, target, sequence in zip(self.transformer_encoders, self.bst_target_field,
                                             self.bst_sequence_field):
            seq_names = _fields(sequence)
            # padding_idx 0 marks the empty positions (BST.py:193 on the FIRST sequence field); the packed int32 id
            # columns themselves are the mask: no cast / compare / [B * H, L1, L1] tensor
            ids = self._first_seq_ids(X, sequence, lambda ids: (ids.long() != 0).to(torch.int32).contiguous())
            pooled.append(encoder.forward_parts([emb[f] for f in seq_names], [emb[f] for f in _fields(target)],
                                                ids=ids, causal=self.use_causal_mask, pool=self.seq_pooling_type))
            dropped.update(seq_names)
        # the other fields in the feature map's order, which is the order the reference's loaders hand the batch in
        # (BST.py:178 follows the batch dict's own order; a captured step's static batch is ordered by packed matrix,
        # so the dict's order is nothing to build the DNN's input on)
        rest = [emb[f] for f in self.feature_map.features if f in emb and f not in dropped]
        return {"y_pred": self.dnn(torch.cat(rest + pooled, dim=-1))}


class FiGNN(_ZooModel):
    """Feature Interaction Graph Neural Network (FiGNN.py:27-231): the fields of a sample as the nodes of a gated
    graph network (layers.FiGNN_Layer: the attentional graph and all gnn_layers in one launch per direction) under
    an attentional prediction head (layers.AttentionalPrediction)."""

    def __init__(self, feature_map, model_id="FiGNN", gpu=-1, learning_rate=1e-3, embedding_dim=10, gnn_layers=3,
                 use_residual=True, use_gru=True, reuse_graph_layer=False, embedding_regularizer=None,
                 net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        num_fields = feature_map.num_fields
        self.embedding_layer = FeatureEmbedding(feature_map, embedding_dim)
        self.fignn = FiGNN_Layer(num_fields, embedding_dim, gnn_layers=gnn_layers,
                                 reuse_graph_layer=reuse_graph_layer, use_gru=use_gru, use_residual=use_residual)
        self.fc = AttentionalPrediction(num_fields, embedding_dim)
        self._ready(kwargs, learning_rate)

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        feature_emb = self.embedding_layer(X)               # [B, F, D]
        h_out = self.fignn(feature_emb)
        y_pred = self.fc(h_out)
        return {"y_pred": self.output_activation(y_pred)}


def _flat_len(fields):
    """len(list(pandas.core.common.flatten([fields]))): the names in a str / tuple / list of them."""
    if isinstance(fields, (list, tuple)):
        return sum(_flat_len(f) for f in fields)
    return 1


class DIEN(_ZooModel):
    """Deep Interest Evolution Network (DIEN.py:27-310): per (target, sequence) pair a GRU over the history
    (interest extraction), attention scores of its states against the target, and an attention-gated GRU towards
    the target (interest evolution), next to the other fields' embeddings in front of the DNN.  Three launches per
    pair and direction (layers.GRU, layers.AttentionLayer, layers.DynamicGRU); the lengths stay on the device:
    no host read, no compaction of the batch, no packing, so the step captures into a hipGraph.
    Not native, each for the reason its message gives: aux_loss_alpha > 0, gru_type="AIGRU" (both raise in the
    reference as well) and attention_type="din_attention"."""

    def __init__(self, feature_map, model_id="DIEN", gpu=-1, dnn_hidden_units=[200, 80], dnn_activations="ReLU",
                 learning_rate=1e-3, embedding_dim=16, net_dropout=0, batch_norm=True,
                 dien_target_field=[("item_id", "cate_id")], dien_sequence_field=[("click_history", "cate_history")],
                 dien_neg_seq_field=[("neg_click_history", "neg_cate_history")], gru_type="AUGRU",
                 enable_sum_pooling=False, attention_dropout=0, attention_type="bilinear_attention",
                 attention_hidden_units=[80, 40], attention_activation="Dice", use_attention_softmax=True,
                 aux_hidden_units=[100, 50], aux_activation="ReLU", aux_loss_alpha=0, embedding_regularizer=None,
                 net_regularizer=None, **kwargs):
        self._base(feature_map, model_id, gpu, embedding_regularizer, net_regularizer, kwargs)
        self.dien_target_field, self.dien_sequence_field = _field_pairs(
            dien_target_field, dien_sequence_field, "dien_sequence_field or dien_target_field not supported.")
        self.dien_neg_seq_field = _field_list(dien_neg_seq_field)
        if aux_loss_alpha > 0:
            raise NotImplementedError("DIEN: aux_loss_alpha > 0 is not native; the reference's own auxiliary loss "
                                      "raises at DIEN.py:228 (the .view of a non-contiguous cat; the mask and loss "
                                      "shapes of DIEN.py:235-237 do not broadcast either)")
        if gru_type == "AIGRU":
            raise NotImplementedError("DIEN: gru_type=AIGRU is not native; the reference raises at DIEN.py:283 "
                                      "([B, L, H] * [B, L] does not broadcast)")
        if gru_type not in ("GRU", "AGRU", "AUGRU"):
            raise ValueError("gru_type={} not supported.".format(gru_type))
        if attention_dropout:
            raise NotImplementedError("DIEN: attention_dropout > 0 only acts inside din_attention, which is not "
                                      "native")
        self.aux_loss_alpha = aux_loss_alpha
        self.feature_map = feature_map
        self.embedding_dim = embedding_dim
        self.embedding_layer = FeatureEmbeddingDict(feature_map, embedding_dim)
        self.sum_pooling = MaskedSumPooling()
        self.gru_type = gru_type
        self.extraction_modules = nn.ModuleList()
        self.evolving_modules = nn.ModuleList()
        self.attention_modules = nn.ModuleList()
        feature_dim = 0
        for target_field, sequence_field in zip(self.dien_target_field, self.dien_sequence_field):
            model_dim = embedding_dim * _flat_len(target_field)
            if len(_fields(sequence_field)) != len(_fields(target_field)):
                raise ValueError("DIEN: target {} and sequence {} differ in their number of fields"
                                 .format(target_field, sequence_field))
            seq_len = feature_map.features[_fields(sequence_field)[0]]["max_len"]
            ops.gru_check(model_dim, seq_len, who="DIEN")
            if len(_fields(target_field)) > ops.GRU_MAX_PARTS:
                raise NotImplementedError("DIEN: {} grouped fields, the fused kernels take 1 or {}"
                                          .format(len(_fields(target_field)), ops.GRU_MAX_PARTS))
            feature_dim += model_dim * 2
            self.extraction_modules.append(GRU(input_size=model_dim, hidden_size=model_dim, batch_first=True))
            if gru_type in ["AGRU", "AUGRU"]:
                self.evolving_modules.append(DynamicGRU(model_dim, model_dim, gru_type=gru_type))
                self.attention_modules.append(
                    AttentionLayer(model_dim, attention_type=attention_type,
                                   attention_hidden_units=attention_hidden_units,
                                   attention_activation=attention_activation,
                                   use_attention_softmax=use_attention_softmax, attention_dropout=attention_dropout))
            else:
                self.evolving_modules.append(GRU(input_size=model_dim, hidden_size=model_dim, batch_first=True))
        # the reference's own width (DIEN.py:134-138): it subtracts the neg-sequence fields whether or not the
        # feature map has them
        feature_dim = feature_dim + feature_map.sum_emb_out_dim() - embedding_dim * _flat_len(self.dien_neg_seq_field)
        self.enable_sum_pooling = enable_sum_pooling
        if not self.enable_sum_pooling:
            feature_dim -= embedding_dim * _flat_len(self.dien_target_field) * 2
        built = self._dnn_input_width()
        if built != feature_dim:        # the reference's shape error at the DNN's first matmul, raised here
            raise RuntimeError("DIEN: mat1 and mat2 shapes cannot be multiplied (Bx{} and {}x{}): DIEN.py:134-135 "
                               "subtracts dien_neg_seq_field={} from the DNN's width, the forward assembles {} "
                               "columns; pass dien_neg_seq_field=[] when the feature map has no such features"
                               .format(built, feature_dim, dnn_hidden_units[0] if dnn_hidden_units else 1,
                                       self.dien_neg_seq_field, built))
        self.dnn = self._tower(feature_dim, dnn_hidden_units, dnn_activations, net_dropout, batch_norm,
                               output_activation=self.output_activation)
        self._ready(kwargs, learning_rate)

    def _neg_names(self):
        names = set()
        for f in self.dien_neg_seq_field:
            names.update(_fields(f))
        return names

    def _dnn_input_width(self):
        """What forward() concatenates in front of the DNN."""
        D = self.embedding_dim
        width = 0
        for target_field in self.dien_target_field:
            width += D * _flat_len(target_field) * (3 if self.enable_sum_pooling else 1)
        neg = self._neg_names()
        for name, spec in self.feature_map.features.items():
            if spec["type"] == "meta" or name in neg:
                continue
            if spec["type"] == "sequence" and not spec.get("feature_encoder"):
                continue                                        # [B, L, D]: not a 2-D embedding
            width += spec.get("emb_output_dim", spec.get("embedding_dim", D))
        return width

    def forward(self, inputs):
        X = self.get_inputs(inputs)
        emb = self.embedding_layer(X)                       # name -> [B, D] | [B, L, D]
        concat_emb = []
        interest_emb = pad_mask = sequence_emb = None
        for idx, (target_field, sequence_field) in enumerate(zip(self.dien_target_field, self.dien_sequence_field)):
            seq_names = _fields(sequence_field)
            tgts = [emb[f] for f in _fields(target_field)]
            seqs = [emb[f] for f in seq_names]
            # padding_idx 0 (DIEN.py:177 on the FIRST sequence field): the packed int32 id columns are the lengths
            # and the mask; they never leave the device
            ids = self._first_seq_ids(X, sequence_field, lambda ids: ids.to(torch.int32).contiguous())
            interest_emb, final = self.extraction_modules[idx].forward_parts(seqs, ids)
            if self.gru_type == "GRU":
                _, final = self.evolving_modules[idx].forward_parts([interest_emb], ids)
            else:
                scores = self.attention_modules[idx].forward_parts(interest_emb, tgts, ids)
                _, final = self.evolving_modules[idx](interest_emb, scores, ids)
            concat_emb.append(final)
            sequence_emb = seqs[0] if len(seqs) == 1 else torch.cat(seqs, dim=-1)
            pad_mask = ids != 0
            if self.enable_sum_pooling:
                sum_pool = [self.sum_pooling(s) for s in seqs]
                concat_emb += sum_pool + [t * s for t, s in zip(tgts, sum_pool)]
        # the other fields in the feature map's order (DIEN.py:189 follows the batch dict's own order, which is the
        # loaders' = the feature map's; a captured step's static batch is ordered by packed matrix)
        neg = self._neg_names()
        concat_emb += [emb[f] for f in self.feature_map.features if f in emb and emb[f].dim() == 2 and f not in neg]
        y_pred = self.dnn(torch.cat(concat_emb, dim=-1))
        return {"y_pred": y_pred, "interest_emb": interest_emb, "neg_emb": None, "pad_mask": pad_mask,
                "pos_emb": sequence_emb}
