"""AOANet on the native layers, host side (no GPU): zoo.AOANet with gpu=-1, where layers.GeneralizedInteractionNet runs
the factorised formula in torch ops and the other kernels are replaced by the torch-CPU emulations of
tests/_cpu_emul.py, against fixtures recorded from the REAL reference's model_zoo.AOANet
(tests/golden/make_golden_aoanet.py).  Checks the parameter names, the forward composition and the optimizer protocol;
the HIP kernels themselves are held to fp64 in tests/test_gpu_gin_kernel.py.

Stated tolerances (those of tests/zoo_cases.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

AOANET_CASES = ["aoanet_zoo_test", "aoanet_adam", "aoanet_one_layer_sgd"]


def gin_reference(B_0, layers):
    """The stack of generalized-interaction layers in plain torch as the reference writes it (AOANet.py:131-134,
    :165-170): layers = [(W [O, D, D], alpha [S * F, O], h [O, D, 1]), ...]; the [B, S * F, D, D] tensor is formed.
    -> every layer's output."""
    F, D = B_0.shape[1:]
    B_i, outs = B_0, []
    for W, alpha, h in layers:
        outer = torch.einsum("bnh,bnd->bnhd", B_0.repeat(1, B_i.shape[1], 1),
                             B_i.repeat(1, 1, F).view(B_i.size(0), -1, D))
        fusion = W * torch.matmul(outer.permute(0, 2, 3, 1), alpha).permute(0, 3, 1, 2)
        B_i = torch.matmul(fusion, h).squeeze(-1)
        outs.append(B_i)
    return outs


def build_aoanet(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.AOANet with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_aoanet.py)."""
    kw = dict(dnn_hidden_units=g.meta["dnn_hidden_units"], dnn_hidden_activations="ReLU", net_dropout=0,
              num_interaction_layers=g.meta["num_interaction_layers"], num_subspaces=g.meta["num_subspaces"])
    kw.update(extra)
    return build_from_golden(zoo.AOANet, g, tmp_path, gpu=gpu, **kw)


def _build(g, tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_aoanet(zoo, g, tmp_path)


@pytest.mark.parametrize("case", AOANET_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    F, D, O, L = model.feature_map.num_fields, g.meta["embedding_dim"], g.meta["num_subspaces"], \
        g.meta["num_interaction_layers"]
    assert tuple(g.state0["fc.weight"].shape) == (1, g.meta["dnn_hidden_units"][-1] + O * D)
    assert tuple(g.state0["gin.layers.0.alpha"].shape) == (F * F, O)
    assert tuple(g.state0["gin.layers.%d.W" % (L - 1)].shape) == (O, D, D)
    assert tuple(g.state0["gin.layers.%d.h" % (L - 1)].shape) == (O, D, 1) and "gin.layers.%d.W" % L not in g.state0
    assert 1e-2 <= g.meta["gin_absmax"] <= 10.0          # the generator's window
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", AOANET_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    check_trajectory(_build(g, tmp_path, monkeypatch), g)


def test_factorised_formula_is_the_reference_formula():
    """What gpu=-1 / fused=False run against the formula that forms the outer-product tensor, in fp64, two layers."""
    from fuxictr_amd.layers import generalized_interaction_composition
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)    # noqa: E731
    B_0 = rnd(3, 5, 6)
    layers = [(rnd(4, 6, 6), rnd(S * 5, 4), rnd(4, 6, 1)) for S in (5, 4)]
    B_i = B_0
    for ref, (W, alpha, h) in zip(gin_reference(B_0, layers), layers):
        B_i = generalized_interaction_composition(B_0, B_i, W, alpha, h)
        assert float((B_i - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_constructor_raises_outside_the_envelope(tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops, zoo
    g = Golden("aoanet_adam")
    lim = ops.gin_limits()
    assert (lim["F_max"], lim["D_max"], lim["O_max"], lim["L_max"]) == (64, 64, 8, 8)
    for kw, text in ((dict(embedding_dim=65), "embedding_dim <= 64"), (dict(num_subspaces=9), "num_subspaces <= 8"),
                     (dict(num_interaction_layers=9), "num_interaction_layers <= 8"),
                     (dict(num_interaction_layers=0), "1 <= num_interaction_layers")):
        with pytest.raises(NotImplementedError, match=text):
            build_aoanet(zoo, g, tmp_path, **kw)


def test_entry_points_validate_before_the_device():
    from fuxictr_amd import _lib
    lib = _lib.load()

    def fwd(B, F, D, O, L, ldb=1 << 20):
        return lib.fx_gin_fwd(None, ldb, B, F, D, O, L, None, None, None)

    def bwd(B, F, D, O, L, ldb=1 << 20):
        return lib.fx_gin_bwd(None, None, ldb, B, F, D, O, L, None, None, None, 1 << 20, 0, None, None, None)
    for call in (fwd, bwd):
        assert call(4, 65, 8, 4, 3) == 1 and b"F <= 64" in lib.fx_last_error()
        assert call(4, 8, 65, 4, 3) == 1 and b"D <= 64" in lib.fx_last_error()
        assert call(4, 8, 8, 9, 3) == 1 and b"O <= 8" in lib.fx_last_error()
        assert call(4, 8, 8, 4, 9) == 1 and b"L <= 8" in lib.fx_last_error()
        assert call(4, 8, 8, 4, 3, ldb=63) == 1 and b"stride" in lib.fx_last_error()
        assert call(4, 8, 8, 4, 3) == 1 and b"null" in lib.fx_last_error()
    for shape in ((9, 65, 8, 4, 3), (9, 8, 65, 4, 3), (9, 8, 8, 9, 3), (9, 8, 8, 4, 0)):
        assert lib.fx_gin_workspace_floats(*shape) == 0
    # a row of the packed gradients per workgroup.  F 4, D 4, O 4: every layer 64 + 64 + 16 floats, tiles of 16 samples
    assert lib.fx_gin_tile_rows(4, 4, 4, 1) == 16 and lib.fx_gin_param_floats(4, 4, 4, 3) == 3 * 144
    assert lib.fx_gin_workspace_floats(100, 4, 4, 4, 3) == 7 * 3 * 144
    # F 39, D 40, O 4: layer 0 6400 + 6084 + 160, the others 6400 + 624 + 160.  LDS floats: the weights 40 x 41 twice, a
    # sample 2 x 40 x 41 (B_0, dB_0) + 2 x 40 x 41 (dP, dQ) + 3 x 4 x 41 -> (40960 - 3280) // 7052 = 5 samples per tile; the
    # tiles of B 4096 outnumber the 256 workgroups
    assert lib.fx_gin_tile_rows(39, 40, 4, 1) == 5 and lib.fx_gin_param_floats(39, 40, 4, 3) == 12644 + 2 * 7184
    assert lib.fx_gin_workspace_floats(4096, 39, 40, 4, 3) == 256 * (12644 + 2 * 7184)
