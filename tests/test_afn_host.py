"""AFN on the native layers, host side (no GPU): zoo.AFN with gpu=-1, where layers.logarithmic_net takes the
reference's own torch ops and the other kernels are replaced by the torch-CPU emulations of tests/_cpu_emul.py,
against fixtures recorded from the REAL reference's model_zoo.AFN (tests/golden/make_golden_afn.py).  Checks the
parameter and buffer names, the forward composition, two embedding layers behind one lookup state and the optimizer
protocol; the HIP kernels themselves are held to fp64 in tests/test_gpu_lognet_kernel.py.

Stated tolerances (those of tests/zoo_cases.py): logits 1e-4, losses 1e-4 per step, trained weights through
conftest.assert_weights_close."""
import pytest
import torch

import _cpu_emul
from conftest import Golden
from zoo_cases import allow_cpu_optimizer, build_from_golden, check_forward, check_trajectory

AFN_CASES = ["afn_zoo_test", "afn_adam", "afn_sgd_bn", "afn_l13_small"]


def lognet_reference(x, W, g1, b1, g2, b2, rm1, rv1, rm2, rv2, training):
    """AFN.logarithmic_net (AFN.py:121-138) in plain torch on tensors: [B, F, D] -> [B, L D]; the running buffers are
    updated in place in training, as nn.BatchNorm1d (eps 1e-5, momentum 0.1) does."""
    bn = torch.nn.functional.batch_norm
    a = bn(torch.log(torch.clamp(torch.abs(x), min=1e-5)), rm1, rv1, g1, b1, training, 0.1, 1e-5)
    u = (a.transpose(2, 1) @ W.t()).transpose(1, 2)
    return torch.flatten(bn(torch.exp(u), rm2, rv2, g2, b2, training, 0.1, 1e-5), start_dim=1)


def build_afn(zoo, g, tmp_path, gpu=-1, **extra):
    """zoo.AFN with a fixture's hyper-parameters and initial weights (shared with tests/test_gpu_afn.py)."""
    m = g.meta
    kw = dict(ensemble_dnn=m["ensemble_dnn"], dnn_hidden_units=m["dnn_hidden"], afn_hidden_units=m["afn_hidden"],
              logarithmic_neurons=m["neurons"], batch_norm=m["batch_norm"])
    kw.update(extra)
    return build_from_golden(zoo.AFN, g, tmp_path, gpu=gpu, **kw)


def _build(g, tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    allow_cpu_optimizer(monkeypatch)
    from fuxictr_amd import zoo
    return build_afn(zoo, g, tmp_path)


@pytest.mark.parametrize("case", AFN_CASES)
def test_state_dict_keys_and_forward_logits(case, tmp_path, monkeypatch):
    g = Golden(case)
    model = _build(g, tmp_path, monkeypatch)            # (asserts the keys)
    for key in ("coefficient_W.weight", "log_batch_norm.running_var", "exp_batch_norm.num_batches_tracked"):
        assert key in g.state0
    assert ("fc.weight" in g.state0) == ("embedding_layer2.embedding_layer.embedding_layers.C1.weight" in g.state0) \
        == g.meta["ensemble_dnn"]
    assert 0.05 <= g.meta["u_std"] <= 3.0 and g.meta["u_absmax"] <= 20.0          # the generator's window
    check_forward(model, g, "0")


@pytest.mark.parametrize("case", AFN_CASES)
def test_training_trajectory_and_trained_weights(case, tmp_path, monkeypatch):
    g = Golden(case)
    check_trajectory(_build(g, tmp_path, monkeypatch), g)


def test_shapes_outside_the_envelope_raise_in_the_constructor(tmp_path, monkeypatch):
    _cpu_emul.install(monkeypatch)
    from fuxictr_amd import ops, zoo
    g = Golden("afn_adam")
    lim = ops.lognet_limits()
    assert (lim["F_max"], lim["D_max"], lim["L_max"]) == (64, 64, 2048)
    with pytest.raises(NotImplementedError, match="logarithmic_neurons <= 2048"):
        build_afn(zoo, g, tmp_path, logarithmic_neurons=2049)
    with pytest.raises(NotImplementedError, match="embedding_dim <= 64"):
        build_afn(zoo, g, tmp_path, embedding_dim=65)


def test_entry_points_validate_before_the_device():
    from fuxictr_amd import _lib
    lib = _lib.load()
    nul = [None] * 10

    def fwd(B, F, D, L, training=1):
        return lib.fx_lognet_fwd(None, F * D, B, F, D, None, L, None, None, None, None, 1e-5, 0.1, training, *nul)
    assert fwd(4, 65, 8, 8) == 1 and b"F <= 64" in lib.fx_last_error()
    assert fwd(4, 8, 65, 8) == 1 and b"D <= 64" in lib.fx_last_error()
    assert fwd(4, 8, 8, 2049) == 1 and b"L <= 2048" in lib.fx_last_error()
    assert fwd(1, 8, 1, 8) == 1 and b"more than 1 value" in lib.fx_last_error()      # as torch refuses it
    assert fwd(4, 8, 8, 8) == 1 and b"null X" in lib.fx_last_error()
    assert lib.fx_lognet_workspace_floats(4, 65, 8, 8) == 0
    # forward: chunk partials, pivots, one partial row per workgroup; backward: ahat, dahat, partials, dW slabs
    assert lib.fx_lognet_workspace_floats(4, 8, 8, 8) == max(256 * 2 * 8 + 8 + 2 * 8,
                                                            32 * 8 + 8 * 32 + 2 * 8 + 256 * 2 * 8 + 8 * 8)
