"""The launches that end every training step, on a real MI355X, arm by arm: the multi-tensor squared norm / Adam / SGD
kernels and the chunking of ops.mt_*, fx_clip_coef / fx_sum_parts, fx_sigmoid_bce, fx_head_train, fx_colsum,
fx_mask_mul and fx_cross_bwd_prep.  Cases, float64 references, guards and bounds: tests/step_tail_cases.py (proven on
the kernel emulation by tests/test_step_tail_host.py); this file only runs them through fuxictr_amd.ops."""
import pytest

pytestmark = pytest.mark.gpu

import step_tail_cases as SC  # noqa: E402
from fuxictr_amd import ops  # noqa: E402

DEV = "cuda:0"
_arms = {}


def _run(group, cid):
    _arms.setdefault(group, set()).update(SC.run(group, cid, ops, DEV))


@pytest.mark.parametrize("cid", SC.ids("mt"))
def test_multi_tensor_sqnorm_clip_adam_sgd(cid):
    """Three steps of fx_mt_sqnorm -> fx_clip_coef -> fx_mt_adam / fx_mt_sgd over views of flat buffers: every
    alignment set, every size around the float4 loop and its grid-stride wrap, 1 / 64 / 65 / 130 tensors."""
    _run("mt", cid)


@pytest.mark.parametrize("cid", SC.ids("mt_agree"))
def test_multi_tensor_adam_arms_agree_bit_for_bit(cid):
    _run("mt_agree", cid)


@pytest.mark.parametrize("cid", SC.ids("clip"))
def test_clip_coef_and_sum_parts(cid):
    _run("clip", cid)


@pytest.mark.parametrize("cid", SC.ids("clip_refusal"))
def test_seventeen_parts_are_refused(cid):
    _run("clip_refusal", cid)


@pytest.mark.parametrize("B", sorted({c["B"] for c in SC.BCE_CASES}))
def test_sigmoid_bce(B):
    for c in SC.BCE_CASES:
        if c["B"] == B:
            _run("bce", c["id"])


@pytest.mark.parametrize("K", SC.HEAD_KS)
def test_head_train(K):
    """Every M of the list at this K: strided h / dz / add against contiguous copies bit for bit, then float64."""
    for c in SC.HEAD_CASES:
        if c["K"] == K:
            _run("head", c["id"])


@pytest.mark.parametrize("cid", SC.ids("head_refusal"))
def test_head_train_refusals(cid):
    _run("head_refusal", cid)


@pytest.mark.parametrize("M", SC.COLSUM_MS)
def test_colsum(M):
    for c in SC.COLSUM_CASES:
        if c["M"] == M:
            _run("colsum", c["id"])


def test_mask_mul_and_cross_bwd_prep():
    for group in ("mask_mul", "cross_prep"):
        for cid in SC.ids(group):
            _run(group, cid)


def test_every_arm_was_reached_on_the_device():
    """The arms the cases report from the device addresses they really passed (a device allocation is aligned like a
    host one, but that is checked here, not assumed).  Runs what has not run yet, so it holds when selected alone."""
    for group, (cases, _) in SC.GROUPS.items():
        if not SC.ARMS[group] <= _arms.get(group, set()):
            for c in cases:
                _run(group, c["id"])
        assert SC.ARMS[group] <= _arms[group], (group, sorted(SC.ARMS[group] - _arms[group]))
