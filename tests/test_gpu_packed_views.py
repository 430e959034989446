"""A deep copy of a layer whose Parameters are views of packed storages (layers._PackedViews) computes with the
copy's own Parameters, on a real MI355X: the copy's Parameters are overwritten through the Parameters, as an
optimizer does, and the fused node -- which reads the packed storage -- must give what the module-by-module route
-- which reads the Parameters -- gives.  A copy whose Parameters no longer alias its storage fails here: its fused
forward still reads the numbers of the original.

Forward and input gradient of both routes against the fp64 restatement of the formulas on the CPU, within the
yardstick of tests/test_gpu_layernorm.py (`compare`: 4 e32 + 1e-6 max|ref|, e32 the error of the same formulas in
fp32 torch on the CPU).  B = 5 is a partial row tile; width 10 takes the scalar arm of the kernels, width 12 the
16-byte arm."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import layers  # noqa: E402
from test_dcn_host import cross_net_reference  # noqa: E402
from test_gdcn_host import gate_cross_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402

DEV = "cuda:0"
B, L = 5, 2


def _copy_with_new_parameters(layer, gen):
    got = copy.deepcopy(layer)
    with torch.no_grad():
        for p in got.parameters():
            new = f32_exact(p.shape[-1] ** -0.5 * torch.randn(*p.shape, generator=gen, dtype=torch.float64))
            p.data.copy_(new.float())
    return got


def _run(fn, x, gy):
    xin = x.float().to(DEV).requires_grad_(True)
    out = fn(xin)
    (dx,) = torch.autograd.grad(out, [xin], gy.float().to(DEV))
    torch.cuda.synchronize()
    return {"out": out.detach(), "dx": dx}


def _torch(fn, x, gy, dtype):
    xin = x.to(dtype).clone().requires_grad_(True)
    out = fn(xin, dtype)
    (dx,) = torch.autograd.grad(out, [xin], gy.to(dtype))
    return {"out": out.detach().double(), "dx": dx.double()}


def _check(tag, routes, formula, x, gy):
    ref, f32 = _torch(formula, x, gy, torch.float64), _torch(formula, x, gy, torch.float32)
    for name, fn in routes:
        compare("%s %s" % (tag, name), _run(fn, x, gy), ref, f32)


def _rnd(gen, *shape):
    return f32_exact(torch.randn(*shape, generator=gen, dtype=torch.float64))


def _with_fused(layer, fused):
    def fn(x):
        layer.fused = fused
        return layer(x)
    return fn


def test_a_copied_cross_net_computes_with_its_own_parameters():
    D = 10
    gen = torch.Generator().manual_seed(21)
    layer = _copy_with_new_parameters(layers.CrossNet(D, L).to(DEV), gen)
    w = torch.cat([ci.weight.weight.detach() for ci in layer.cross_net]).double().cpu()
    b = torch.stack([ci.bias.detach() for ci in layer.cross_net]).double().cpu()
    _check("copied CrossNet", [("fused", _with_fused(layer, True)), ("module by module", _with_fused(layer, False))],
           lambda x, dt: cross_net_reference(x, w.to(dt), b.to(dt)), _rnd(gen, B, D), _rnd(gen, B, D))


def test_a_copied_gate_cross_layer_computes_with_its_own_parameters():
    D = 12
    gen = torch.Generator().manual_seed(22)
    layer = _copy_with_new_parameters(layers.GateCrossLayer(D, L).to(DEV), gen)
    ws, wgs, bs = ([t.detach().double().cpu() for t in group] for group in (
        [m.weight for m in layer.w], [m.weight for m in layer.wg], list(layer.b)))
    _check("copied GateCrossLayer",
           [("fused", _with_fused(layer, True)), ("module by module", _with_fused(layer, False))],
           lambda x, dt: gate_cross_reference(x, *([t.to(dt) for t in group] for group in (ws, wgs, bs))),
           _rnd(gen, B, D), _rnd(gen, B, D))


def test_a_copied_field_layer_norm_computes_with_its_own_parameters():
    F, D = 3, 10
    gen = torch.Generator().manual_seed(23)
    layer = _copy_with_new_parameters(layers.FieldLayerNorm(F, D).to(DEV), gen)
    gamma = [m.weight.detach().double().cpu() for m in layer]
    beta = [m.bias.detach().double().cpu() for m in layer]

    def formula(x, dt):
        return torch.cat([torch.nn.functional.layer_norm(x[:, i], (D,), gamma[i].to(dt), beta[i].to(dt), layer._eps)
                          for i in range(F)], dim=1)

    def per_field(x):        # one LayerNorm module per field: reads the Parameters
        return torch.cat([norm(x[:, i, :]) for i, norm in enumerate(layer)], dim=1)
    _check("copied FieldLayerNorm", [("fused", layer), ("field by field", per_field)], formula,
           _rnd(gen, B, F, D), _rnd(gen, B, F * D))
