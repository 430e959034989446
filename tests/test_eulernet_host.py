"""EulerNet on the native layers, host side (no GPU): zoo.EulerNet with gpu=-1, where layers.EulerInteractionLayer and
layers.euler_polar take the reference's own torch ops and the other kernels are replaced by the torch-CPU emulations of
tests/_cpu_emul.py, against fixtures recorded from the REAL reference's model_zoo.EulerNet
(tests/golden/make_golden_eulernet.py).  Checks the parameter names, the forward composition, the initialisation order
and the optimizer protocol; the HIP kernels themselves are held to fp64 in tests/test_gpu_euler_kernel.py.

Stated tolerances (those of tests/zoo_cases.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

EULER_CASES = ["eulernet_zoo_test", "eulernet_two_layers_sgd", "eulernet_d10_adam"]


def euler_reference(r, p, z, orders, bias_lam, bias_theta, norms):
    """One Euler interaction layer (EulerNet.py:139-170) in plain torch on tensors: r, p [B, Fi, D], the dense path's
    pre-activation z [2 B, O D], bias [D, O]; norms None or (w_r, b_r, w_p, b_p) -> (o_r, o_p) [B, O, D]."""
    B, _, D = r.shape
    a, t = 0.5 * torch.log(r ** 2 + p ** 2 + 1e-8), torch.atan2(p, r)
    ul = (a.transpose(1, 2) @ orders + bias_lam).transpose(1, 2)
    ut = (t.transpose(1, 2) @ orders + bias_theta).transpose(1, 2)
    zr, zp = torch.relu(z[:B]).reshape(B, -1, D), torch.relu(z[B:]).reshape(B, -1, D)
    o_r, o_p = zr + torch.exp(ul) * torch.cos(ut), zp + torch.exp(ul) * torch.sin(ut)
    if norms is not None:
        ln = torch.nn.functional.layer_norm
        o_r, o_p = ln(o_r, (D,), norms[0], norms[1], 1e-5), ln(o_p, (D,), norms[2], norms[3], 1e-5)
    return o_r, o_p


def build_eulernet(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.EulerNet with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_eulernet.py)."""
    kw = dict(shape=g.meta["shape"], layer_norm=g.meta["layer_norm"], net_ex_dropout=0, net_im_dropout=0)
    kw.update(extra)
    return build_from_golden(zoo.EulerNet, g, tmp_path, gpu=gpu, **kw)


def _build(g, tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_eulernet(zoo, g, tmp_path)


@pytest.mark.parametrize("case", EULER_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    for key in ("mu", "Euler_interaction_layers.0.inter_orders", "Euler_interaction_layers.0.bias_lam",
                "Euler_interaction_layers.0.norm_p.weight", "Euler_interaction_layers.0.im.bias", "reg.bias"):
        assert key in g.state0
    assert g.meta["ul_absmax"] <= 20.0 and g.meta["cut_margin"] >= 1e-3          # the generator's window
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", EULER_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    check_trajectory(_build(g, tmp_path, monkeypatch), g)


def test_constructor_raises_outside_the_envelope_and_for_ex_dropout(tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops, zoo
    g = Golden("eulernet_two_layers_sgd")
    lim = ops.euler_limits()
    assert (lim["F_max"], lim["D_max"], lim["O_max"]) == (64, 64, 64)
    with pytest.raises(NotImplementedError, match=r"shape\[1\] <= 64"):
        build_eulernet(zoo, g, tmp_path, shape=[6, 65])
    with pytest.raises(NotImplementedError, match="embedding_dim <= 64"):
        build_eulernet(zoo, g, tmp_path, embedding_dim=65)
    with pytest.raises(NotImplementedError, match="net_ex_dropout=0.1"):
        build_eulernet(zoo, g, tmp_path, net_ex_dropout=0.1)


def test_initialisers_survive_the_constructor(tmp_path, monkeypatch):
    """reset_parameters() runs before the layers exist: the second [6, 6] layer keeps its eye, `im` its xavier-uniform
    range (a re-initialised Linear would be xavier-normal with zero bias)."""
    _cpu_emul.install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    from fuxictr_amd.features import FeatureMap
    g = Golden("eulernet_two_layers_sgd")
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": 8})
    model = zoo.EulerNet(fmap, gpu=-1, shape=[6, 6], embedding_dim=8, optimizer="SGD", loss="binary_crossentropy",
                         task="binary_classification", metrics=["logloss"], verbose=0, model_root=str(tmp_path))
    second = model.Euler_interaction_layers[1]
    assert torch.equal(second.inter_orders, torch.eye(6))
    assert float(second.im.weight.detach().abs().max()) <= (6.0 / (48 + 48)) ** 0.5 and bool((second.im.bias != 0).any())
    assert float(model.Euler_interaction_layers[0].inter_orders.detach().sum(0).sub(1).abs().max()) < 1e-5


def test_entry_points_validate_before_the_device():
    from fuxictr_amd import _lib
    lib = _lib.load()

    def fwd(B, Fi, D, O):
        return lib.fx_euler_fwd(None, None, B, Fi, D, O, None, None, None, 1, None, None, None, None, 1e-5, None, None,
                                None)

    def bwd(B, Fi, D, O):
        return lib.fx_euler_bwd(None, None, B, Fi, D, O, None, None, None, 1, None, None, 1e-5, *[None] * 9)
    for call in (fwd, bwd):
        assert call(4, 65, 8, 8) == 1 and b"Fi <= 64" in lib.fx_last_error()
        assert call(4, 8, 65, 8) == 1 and b"D <= 64" in lib.fx_last_error()
        assert call(4, 8, 8, 65) == 1 and b"O <= 64" in lib.fx_last_error()
        assert call(4, 8, 8, 8) == 1 and b"null RP" in lib.fx_last_error()
    assert lib.fx_euler_polar_fwd(None, 64, None, 4, 8, 65, None, None) == 1 and b"D <= 64" in lib.fx_last_error()
    assert lib.fx_euler_polar_fwd(None, 8, None, 4, 8, 8, None, None) == 1 and b"stride" in lib.fx_last_error()
    assert lib.fx_euler_polar_fwd(None, 64, None, 4, 8, 8, None, None) == 1 and b"null E" in lib.fx_last_error()
    assert lib.fx_euler_polar_bwd(None, 64, None, 4, 65, 8, None, None, 64, None, None, None) == 1
    assert lib.fx_euler_polar_bwd(None, 64, None, 4, 8, 8, None, None, 64, None, None, None) == 1 \
        and b"null E" in lib.fx_last_error()
    for shape in ((4, 65, 8, 8), (4, 8, 65, 8), (4, 8, 8, 65)):
        assert lib.fx_euler_workspace_floats(*shape) == 0
    # a | t [2, N, FP], dul | dut [2, N, OS], one bias row and 16 LayerNorm rows per workgroup, one orders slab; or
    # the polar backward's chunk rows
    assert lib.fx_euler_workspace_floats(4, 8, 8, 8) == max(2 * 32 * 8 + 2 * 32 * 8 + 2 * 8 * 8 + 16 * 4 * 8 + 8 * 8,
                                                           256 * 8)
