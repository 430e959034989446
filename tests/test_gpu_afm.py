"""AFM end to end on a real MI355X: zoo.AFM on the native layers (the pairwise attention on csrc/fx_afm.hip) against
the fixtures recorded from the REAL reference's model_zoo.AFM (tests/golden/make_golden_afm.py), with the tolerances
of tests/test_gpu_gdcn.py / test_gpu_models.py:
  forward logits |d| <= 1e-4, pred atol 2e-5, loss trajectory |d| <= 1e-4 per step, trained weights
  conftest.assert_weights_close.
The attention layer alone (layers.afm_attention and the module-by-module composition) is held to the fp64 restatement
with the yardstick of tests/test_gpu_layernorm.py: 4 * e32 + 1e-6 * max|ref| per tensor, e32 the error of the fp32
torch composition on the CPU.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import Golden  # noqa: E402
from fuxictr_amd import layers, zoo  # noqa: E402
from test_afm_host import AFM_CASES, afm_pairs, afm_reference, build_afm  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402
from zoo_cases import check_forward, check_graph_replay, check_trajectory  # noqa: E402

DEV = "cuda:0"


def build_native(g, tmp_path, hip_graph=False, fused=True):
    return build_afm(zoo, g, tmp_path, gpu=0, sparse_update="exact", hip_graph=hip_graph, fused=fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", AFM_CASES)
def test_forward_logits_match_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_forward(model, g, "0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", AFM_CASES)
def test_training_trajectory_matches_reference(case, fused, tmp_path):
    g = Golden(case)
    model = build_native(g, tmp_path, fused=fused)
    check_trajectory(model, g)


def _torch_results(inp, dtype):
    t = {k: v.to(dtype).clone().requires_grad_(k != "g") for k, v in inp.items()}
    out = afm_reference(t["x"], t["W1"], t["b1"], t["w2"], t["wp"], t["add"])
    names = ("x", "W1", "b1", "w2", "wp", "add")
    grads = torch.autograd.grad(out, [t[k] for k in names], t["g"])
    res = {"out": out.detach().double()}
    res.update({"d" + k: v.double() for k, v in zip(names, grads)})
    return res


def _layer_results(att, proj, inp, fused):
    x = inp["x"].float().to(DEV).requires_grad_(True)
    add = inp["add"].float().to(DEV).requires_grad_(True)
    if fused:
        out = layers.afm_attention(x, att, proj, addend=add)
    else:
        e = afm_pairs(x)
        out = proj(torch.sum(att(e) * e, dim=1)) + add
    params = [att[0].weight, att[0].bias, att[2].weight, proj.weight]
    grads = torch.autograd.grad(out, [x] + params + [add], inp["g"].float().to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    res.update({"d" + k: v for k, v in zip(("x", "W1", "b1", "w2", "wp", "add"), grads)})
    return res


@pytest.mark.parametrize("shape", [(33, 6, 10, 7), (65, 9, 8, 16)], ids=lambda s: "B%d-F%d-D%d-A%d" % s)
def test_attention_layer_forward_and_backward_within_the_fp32_yardstick(shape):
    B, F, D, A = shape
    inp = None
    for seed in range(40 + B, 48 + B):             # the ReLU margin of tests/test_gpu_afm_attn.py
        gen = torch.Generator().manual_seed(seed)

        def rnd(*s, scale=1.0):
            return f32_exact(scale * torch.randn(*s, generator=gen, dtype=torch.float64))
        cand = dict(x=rnd(B, F, D), W1=rnd(A, D, scale=0.2 * D ** -0.5), w2=rnd(1, A), wp=rnd(1, D, scale=D ** -0.5),
                    add=rnd(B, 1), g=rnd(B, 1))
        cand["b1"] = f32_exact(torch.sign(rnd(A)) * (1.0 + 0.5 * torch.rand(A, generator=gen, dtype=torch.float64)))
        z = afm_reference(cand["x"], cand["W1"], cand["b1"], cand["w2"], cand["wp"], parts=True)[1]
        if float(z.abs().min()) >= 1e-5 * float(z.abs().max()):
            inp = cand
            break
    assert inp is not None
    att = torch.nn.Sequential(layers.FxLinear(D, A), torch.nn.ReLU(), layers.FxLinear(A, 1, bias=False),
                              torch.nn.Softmax(dim=1)).to(DEV)
    proj = layers.FxLinear(D, 1, bias=False).to(DEV)
    with torch.no_grad():
        att[0].weight.copy_(inp["W1"].float()), att[0].bias.copy_(inp["b1"].float())
        att[2].weight.copy_(inp["w2"].float()), proj.weight.copy_(inp["wp"].float())
    ref, f32 = _torch_results(inp, torch.float64), _torch_results(inp, torch.float32)
    for fused in (True, False):
        tag = "afm attention %s %s" % (shape, "fused" if fused else "module by module")
        got = _layer_results(att, proj, inp, fused)
        compare(tag, got, ref, f32)
        if fused:
            again = _layer_results(att, proj, inp, fused)               # the same inputs: the same bits
            for name in got:
                assert torch.equal(got[name], again[name]), name


def test_hip_graph_replay_is_bit_identical_to_eager(tmp_path):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits (no atomics in the two
    kernels); the capture really happened (`_graph_state`), it did not fall back to eager."""
    g = Golden("afm_adam")
    check_graph_replay(lambda hip_graph: build_native(g, tmp_path, hip_graph=hip_graph), g)
