"""Layers whose Parameters are views of packed storages (layers._PackedViews: CrossNet, GateCrossLayer,
FieldLayerNorm).  The fused node reads the storages, the optimizer and state_dict see the Parameters; the two must
stay one memory through everything that hands the module new tensors: copy.deepcopy, a pickle round trip and a
dtype round trip.  No kernel runs here: construction, copies and state dicts only."""
import copy
import pickle

import pytest
import torch

from fuxictr_amd import layers

MAKERS = {"CrossNet": lambda: layers.CrossNet(10, 2),
          "GateCrossLayer": lambda: layers.GateCrossLayer(12, 2),
          "FieldLayerNorm": lambda: layers.FieldLayerNorm(3, 10)}

# list(state_dict().items()) as (key, shape), in order
STATE = {
    "CrossNet": [("cross_net.0.bias", (10,)), ("cross_net.0.weight.weight", (1, 10)),
                 ("cross_net.1.bias", (10,)), ("cross_net.1.weight.weight", (1, 10))],
    "GateCrossLayer": [("w.0.weight", (12, 12)), ("w.1.weight", (12, 12)), ("wg.0.weight", (12, 12)),
                       ("wg.1.weight", (12, 12)), ("b.0", (12,)), ("b.1", (12,))],
    "FieldLayerNorm": [("0.weight", (10,)), ("0.bias", (10,)), ("1.weight", (10,)), ("1.bias", (10,)),
                       ("2.weight", (10,)), ("2.bias", (10,))],
}

WAYS = {"deepcopy": copy.deepcopy,
        "pickle": lambda m: pickle.loads(pickle.dumps(m)),
        "double_float": lambda m: m.double().float()}


def packed_slices(layer):
    """-> [(state_dict key, Parameter, its slice of the layer's packed storage)]"""
    out = []
    if isinstance(layer, layers.CrossNet):
        for i, ci in enumerate(layer.cross_net):
            out += [("cross_net.%d.weight.weight" % i, ci.weight.weight, layer._w[i:i + 1]),
                    ("cross_net.%d.bias" % i, ci.bias, layer._b[i])]
    elif isinstance(layer, layers.GateCrossLayer):
        for i, p in enumerate(layer._packed):
            D = p.shape[1]
            out += [("w.%d.weight" % i, layer.w[i].weight, p[:D]), ("wg.%d.weight" % i, layer.wg[i].weight, p[D:])]
    else:
        for i, mod in enumerate(layer):
            out += [("%d.weight" % i, mod.weight, layer._packed[0, i]), ("%d.bias" % i, mod.bias, layer._packed[1, i])]
    return out


def storages(layer):
    if isinstance(layer, layers.CrossNet):
        return [layer._w, layer._b]
    return list(layer._packed) if isinstance(layer, layers.GateCrossLayer) else [layer._packed]


def assert_aliased(layer):
    for key, p, s in packed_slices(layer):
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad, key
        assert p.data_ptr() == s.data_ptr() and p.shape == s.shape and p.stride() == s.stride(), key
        assert p.dtype == s.dtype == torch.float32 and p.device == s.device, key


@pytest.mark.parametrize("way", sorted(WAYS))
@pytest.mark.parametrize("kind", sorted(MAKERS))
def test_parameters_stay_views_of_the_packed_storage(kind, way):
    torch.manual_seed(11)
    orig = MAKERS[kind]()
    with torch.no_grad():                       # (FieldLayerNorm starts as ones / zeros: make every value its own)
        for _, p, _ in packed_slices(orig):
            p.copy_(torch.randn(p.shape))
    assert_aliased(orig)
    before = [s.clone() for s in storages(orig)]
    got = WAYS[way](orig)
    assert_aliased(got)
    assert len(storages(got)) == len(before)
    for s, b in zip(storages(got), before):     # the same numbers as the original's
        assert torch.equal(s, b)
    # an optimizer's in-place step on the copy's Parameters is a step on the copy's storage, and on no other
    for _, p, _ in packed_slices(got):
        p.data.add_(1)
    for s, b in zip(storages(got), before):
        assert torch.equal(s, b + 1)
    if got is not orig:
        assert_aliased(orig)
        for s, b in zip(storages(orig), before):
            assert torch.equal(s, b)
        assert not {s.data_ptr() for s in storages(got)} & {s.data_ptr() for s in storages(orig)}


@pytest.mark.parametrize("kind", sorted(MAKERS))
def test_state_dict_keys_and_shapes_are_the_references(kind):
    sd = MAKERS[kind]().state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == STATE[kind]


@pytest.mark.parametrize("kind", sorted(MAKERS))
def test_load_state_dict_lands_in_the_packed_storage(kind):
    layer = MAKERS[kind]()
    gen = torch.Generator().manual_seed(5)
    sd = {k: torch.randn(*shape, generator=gen) for k, shape in STATE[kind]}
    layer.load_state_dict(sd, strict=True)
    assert_aliased(layer)
    slices = packed_slices(layer)
    assert sum(s.numel() for _, _, s in slices) == sum(t.numel() for t in storages(layer))    # nothing else in there
    for key, _, s in slices:
        assert torch.equal(s.cpu(), sd[key]), key
    back = layer.state_dict()
    for key, v in sd.items():
        assert torch.equal(back[key].cpu(), v), key
