"""How well conditioned a DESTINE fixture is, on the CPU: the recorded steps of tests/test_destine_host.py with the
attention layers computed in fp64 (rounded to fp32 once, at the layer's output and gradients) instead of in the
reference's fp32.  Such a run is as far from the reference's rounding as any correct fp32 implementation, so its
distance from the recorded logits is what the fixture itself contributes to tests/zoo_cases.py's 1e-4.  The seed of
destine_adam in make_golden_destine.py was chosen with it (seed 7: 1.1e-3, seed 11: 3.1e-5).

    python tests/golden/probe_destine_fp64.py [case ...]        (after make_golden_destine.py)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import test_destine_host as host  # noqa: E402

_fp32 = host.dsa_reference


def _fp64(X, params, H, use_scale, relu_before_att, dtype=None):
    return _fp32(X, params, H, use_scale, relu_before_att, dtype=torch.float64).float()


def _fwd(X, W, bias, H, use_scale, relu_before_att, Y):
    with torch.no_grad():
        Y.copy_(_fp64(X, list(W) + list(bias), H, use_scale, relu_before_att))
    return Y


if __name__ == "__main__":
    host.dsa_reference, host._emul_dsa_fwd = _fp64, _fwd        # (_emul_dsa_bwd reads the module's dsa_reference)
    only = " or ".join(sys.argv[1:]) or "destine"
    sys.exit(pytest.main(["-q", "-s", "-p", "no:cacheprovider", host.__file__, "-k", "trajectory and (%s)" % only]))
