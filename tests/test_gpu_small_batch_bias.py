"""The bias gradient of a Linear on both sides of the switch in layers._bias_grad, on a real MI355X: the weight-
gradient GEMM sums it in its epilogue only when it contracts over more than 8 rows; a batch of 8 rows or fewer takes
the column sums of dz in a launch of their own (fx_colsum).  B = 5 and 8 take that launch, B = 9 the epilogue.

Every parameter gradient (and the input gradient) of
    GateCrossLayer(12, 2), fused           linear_grads on [w | wg] with the bias row sums: b.<i>, w.<i>, wg.<i>
    MLP_Block 12 -> 16 -> 8 -> 1, biases   linear_grads in every layer (the input wants its gradient)
    the same tower, input without gradient linear_weight_grads in the first layer
    FxLinear(12, 6) with bias              linear_weight_grads alone
against the fp64 restatement on the CPU within the yardstick of tests/test_gpu_layernorm.py (`compare`:
4 e32 + 1e-6 max|ref|, e32 the error of the same formulas in fp32 torch on the CPU)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import layers  # noqa: E402
from test_gdcn_host import gate_cross_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402

DEV = "cuda:0"
ROWS = [5, 8, 9]


def _rnd(gen, *shape, scale=1.0):
    return f32_exact(scale * torch.randn(*shape, generator=gen, dtype=torch.float64))


def _native(module, names, x, gy, x_grad):
    """Forward and backward of `module` on the GPU -> out, the gradients of its Parameters `names` (+ dx)."""
    params = dict(module.named_parameters())
    xin = x.float().to(DEV).requires_grad_(x_grad)
    out = module(xin)
    grads = torch.autograd.grad(out, ([xin] if x_grad else []) + [params[n] for n in names], gy.float().to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    if x_grad:
        res["dx"], grads = grads[0], grads[1:]
    res.update(("d " + n, g) for n, g in zip(names, grads))
    return res


def _torch(formula, values, names, x, gy, x_grad, dtype):
    ps = {n: values[n].to(dtype).clone().requires_grad_(True) for n in names}
    xin = x.to(dtype).clone().requires_grad_(x_grad)
    out = formula(xin, ps)
    grads = torch.autograd.grad(out, ([xin] if x_grad else []) + [ps[n] for n in names], gy.to(dtype))
    res = {"out": out.detach().double()}
    if x_grad:
        res["dx"], grads = grads[0].double(), grads[1:]
    res.update(("d " + n, g.double()) for n, g in zip(names, grads))
    return res


def _check(tag, module, formula, x, gy, x_grad):
    names = [n for n, _ in module.named_parameters()]
    values = {n: p.detach().double().cpu() for n, p in module.named_parameters()}
    ref = _torch(formula, values, names, x, gy, x_grad, torch.float64)
    f32 = _torch(formula, values, names, x, gy, x_grad, torch.float32)
    assert any(n.endswith("bias") or n.startswith("b.") for n in names), names
    compare(tag, _native(module, names, x, gy, x_grad), ref, f32)


def _randomize(module, gen):
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(_rnd(gen, *p.shape, scale=p.shape[-1] ** -0.5).float())
    return module


@pytest.mark.parametrize("B", ROWS)
def test_gate_cross_layer_parameter_gradients(B):
    D, n = 12, 2
    gen = torch.Generator().manual_seed(31 + B)
    layer = _randomize(layers.GateCrossLayer(D, n).to(DEV), gen)
    layer.fused = True

    def formula(x, ps):
        return gate_cross_reference(x, [ps["w.%d.weight" % i] for i in range(n)],
                                    [ps["wg.%d.weight" % i] for i in range(n)], [ps["b.%d" % i] for i in range(n)])
    _check("GateCrossLayer B %d" % B, layer, formula, _rnd(gen, B, D), _rnd(gen, B, D), True)


@pytest.mark.parametrize("x_grad", [True, False], ids=["dx", "no-dx"])
@pytest.mark.parametrize("B", ROWS)
def test_mlp_block_parameter_gradients(B, x_grad):
    gen = torch.Generator().manual_seed(41 + B)
    tower = _randomize(layers.MLP_Block(input_dim=12, hidden_units=[16, 8], output_dim=1), gen)
    assert tower._fused is not None and not tower._fused[1]         # one fused node, nothing behind it

    def formula(x, ps):
        h = torch.relu(x @ ps["mlp.0.weight"].t() + ps["mlp.0.bias"])
        h = torch.relu(h @ ps["mlp.2.weight"].t() + ps["mlp.2.bias"])
        return h @ ps["mlp.4.weight"].t() + ps["mlp.4.bias"]
    _check("MLP_Block B %d %s" % (B, "dx" if x_grad else "no dx"), tower, formula, _rnd(gen, B, 12), _rnd(gen, B, 1),
           x_grad)


@pytest.mark.parametrize("B", ROWS)
def test_fx_linear_parameter_gradients(B):
    gen = torch.Generator().manual_seed(51 + B)
    lin = _randomize(layers.FxLinear(12, 6, device=DEV), gen)
    _check("FxLinear B %d" % B, lin, lambda x, ps: x @ ps["weight"].t() + ps["bias"], _rnd(gen, B, 12),
           _rnd(gen, B, 6), False)
