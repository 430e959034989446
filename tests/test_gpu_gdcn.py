"""GDCN and GDCNP end to end on a real MI355X: zoo.GDCN / zoo.GDCNP on the native layers (the gated cross layer on
csrc/fx_gatecross.hip behind one GEMM against the packed weights) against the fixtures recorded from the REAL
reference's model_zoo.GDCN (tests/golden/make_golden_gdcn.py), with the tolerances of tests/test_gpu_finalmlp.py /
test_gpu_models.py:
  forward logits |d| <= 1e-4, pred atol 2e-5, loss trajectory |d| <= 1e-4 per step, trained weights
  conftest.assert_weights_close.
layers.GateCrossLayer alone is held to the fp64 restatement with the yardstick of tests/test_gpu_layernorm.py:
4 * e32 + 1e-6 * max|ref| per tensor, e32 the error of the fp32 torch composition on the CPU.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import layers, zoo  # noqa: E402
from test_gdcn_host import GDCN_CASES, build_gdcn, gate_cross_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402

DEV = "cuda:0"


def build_native(g, tmp_path, sparse_update="exact", hip_graph=False, fused=True):
    return build_gdcn(zoo, g, tmp_path, gpu=0, sparse_update=sparse_update, hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", GDCN_CASES)
def test_forward_logits_match_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", GDCN_CASES)
def test_training_trajectory_matches_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_trajectory(model, g)
    # w and wg are still views of the packed storage the GEMM reads
    for i, p in enumerate(model.cross_net._packed):
        D = p.shape[1]
        assert model.cross_net.w[i].weight.data_ptr() == p.data_ptr()
        assert model.cross_net.wg[i].weight.data_ptr() == p[D:].data_ptr()


def _layer_results(layer, x, gy, fused):
    layer.fused = fused
    n = layer.cn_layers
    params = [p for i in range(n) for p in (layer.w[i].weight, layer.wg[i].weight, layer.b[i])]
    xin = x.float().to(DEV).requires_grad_(True)
    out = layer(xin)
    grads = torch.autograd.grad(out, [xin] + params, gy.float().to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach(), "dx": grads[0]}
    for i in range(n):
        res["dw%d" % i], res["dwg%d" % i], res["db%d" % i] = grads[1 + 3 * i:4 + 3 * i]
    return res


def _torch_results(x, gy, ws, wgs, bs, dtype):
    xin = x.to(dtype).clone().requires_grad_(True)
    ps = [[t.to(dtype).clone().requires_grad_(True) for t in group] for group in (ws, wgs, bs)]
    out = gate_cross_reference(xin, *ps)
    n = len(ws)
    grads = torch.autograd.grad(out, [xin] + [ps[k][i] for i in range(n) for k in range(3)], gy.to(dtype))
    res = {"out": out.detach().double(), "dx": grads[0].double()}
    for i in range(n):
        res["dw%d" % i], res["dwg%d" % i], res["db%d" % i] = (t.double() for t in grads[1 + 3 * i:4 + 3 * i])
    return res


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [(33, 20), (65, 70)], ids=lambda s: "B%d-D%d" % s)
def test_gate_cross_layer_forward_and_backward_within_the_fp32_yardstick(shape, n):
    B, D = shape
    gen = torch.Generator().manual_seed(7 + B + n)

    def rnd(*s, scale=1.0):
        return f32_exact(scale * torch.randn(*s, generator=gen, dtype=torch.float64))
    ws = [rnd(D, D, scale=D ** -0.5) for _ in range(n)]
    wgs = [rnd(D, D, scale=D ** -0.5) for _ in range(n)]
    bs = [f32_exact(torch.rand(D, generator=gen, dtype=torch.float64)) for _ in range(n)]
    x, gy = rnd(B, D), rnd(B, D)
    layer = layers.GateCrossLayer(D, n).to(DEV)
    sd = {}
    for i in range(n):
        sd["w.%d.weight" % i], sd["wg.%d.weight" % i], sd["b.%d" % i] = ws[i].float(), wgs[i].float(), bs[i].float()
    layer.load_state_dict(sd)
    assert layer._packed[0].is_cuda and layer.w[0].weight.data_ptr() == layer._packed[0].data_ptr()
    ref, f32 = _torch_results(x, gy, ws, wgs, bs, torch.float64), _torch_results(x, gy, ws, wgs, bs, torch.float32)
    for fused in (True, False):
        tag = "GateCrossLayer %s n %d %s" % (shape, n, "fused" if fused else "module by module")
        got = _layer_results(layer, x, gy, fused)
        compare(tag, got, ref, f32)
        if fused:
            again = _layer_results(layer, x, gy, fused)                 # the same inputs: the same bits
            for name in got:
                assert torch.equal(got[name], again[name]), name


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits (no atomics in the two
    kernels); the capture really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("gdcnp_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)
