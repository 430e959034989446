"""DCN end to end on a real MI355X: zoo.DCN on the native layers (the rank-1 cross network on csrc/fx_crossnet.hip,
one launch forward and two backward for the whole stack) against the fixtures recorded from the REAL reference's
model_zoo.DCN (tests/golden/make_golden_dcn.py), with the tolerances of tests/test_gpu_gdcn.py / test_gpu_models.py:
  forward logits |d| <= 1e-4, pred atol 2e-5, loss trajectory |d| <= 1e-4 per step, trained weights
  conftest.assert_weights_close.
layers.CrossNet alone is held to the fp64 restatement with the yardstick of tests/test_gpu_layernorm.py:
4 * e32 + 1e-6 * max|ref| per tensor, e32 the error of the fp32 torch composition on the CPU.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import layers, zoo  # noqa: E402
from test_dcn_host import DCN_CASES, build_dcn, cross_net_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402

DEV = "cuda:0"


def build_native(g, tmp_path, sparse_update="exact", hip_graph=False, fused=True):
    return build_dcn(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", DCN_CASES)
def test_forward_logits_match_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    assert model.crossnet.native(torch.empty(2, model.feature_map.sum_emb_out_dim())) == fused
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", DCN_CASES)
def test_training_trajectory_matches_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_trajectory(model, g)
    # the weights and biases are still views of the packed storages the kernels read
    cn = model.crossnet
    for i, ci in enumerate(cn.cross_net):
        assert ci.weight.weight.data_ptr() == cn._w[i].data_ptr() and ci.bias.data_ptr() == cn._b[i].data_ptr()


def _layer_results(layer, x, gy, fused):
    layer.fused = fused
    params = [p for ci in layer.cross_net for p in (ci.weight.weight, ci.bias)]
    xin = x.float().to(DEV).requires_grad_(True)
    out = layer(xin)
    grads = torch.autograd.grad(out, [xin] + params, gy.float().to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach(), "dx": grads[0]}
    for i in range(layer.num_layers):
        res["dw%d" % i], res["db%d" % i] = grads[1 + 2 * i].reshape(-1), grads[2 + 2 * i]
    return res


def _torch_results(x, gy, w, b, dtype):
    xin, wi, bi = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    out = cross_net_reference(xin, wi, bi)
    dx, dw, db = torch.autograd.grad(out, [xin, wi, bi], gy.to(dtype))
    res = {"out": out.detach().double(), "dx": dx.double()}
    for i in range(w.shape[0]):
        res["dw%d" % i], res["db%d" % i] = dw[i].double(), db[i].double()
    return res


@pytest.mark.parametrize("shape", [(33, 90, 3), (65, 624, 2)], ids=lambda s: "B%d-D%d-L%d" % s)
def test_cross_net_layer_forward_and_backward_within_the_fp32_yardstick(shape):
    B, D, n = shape
    gen = torch.Generator().manual_seed(7 + B + n)

    def rnd(*s, scale=1.0):
        return f32_exact(scale * torch.randn(*s, generator=gen, dtype=torch.float64))
    w, b = rnd(n, D, scale=0.5 * D ** -0.5), rnd(n, D, scale=0.3)
    x, gy = rnd(B, D), rnd(B, D)
    layer = layers.CrossNet(D, n).to(DEV)
    sd = {}
    for i in range(n):
        sd["cross_net.%d.weight.weight" % i], sd["cross_net.%d.bias" % i] = w[i:i + 1].float(), b[i].float()
    layer.load_state_dict(sd)
    assert layer._w.is_cuda and layer.cross_net[0].weight.weight.data_ptr() == layer._w.data_ptr()
    assert layer.native(torch.empty(2, D))
    ref, f32 = _torch_results(x, gy, w, b, torch.float64), _torch_results(x, gy, w, b, torch.float32)
    for fused in (True, False):
        tag = "CrossNet %s %s" % (shape, "fused" if fused else "module by module")
        got = _layer_results(layer, x, gy, fused)
        compare(tag, got, ref, f32)
        if fused:
            again = _layer_results(layer, x, gy, fused)                 # the same inputs: the same bits
            for name in got:
                assert torch.equal(got[name], again[name]), name


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits (no atomics in the three
    kernels); the capture really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("dcn_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)
