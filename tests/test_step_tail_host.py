"""tests/step_tail_cases.py without a GPU: every case of tests/test_gpu_step_tail.py runs on the kernel emulation
(tests/_cpu_emul.py) against the same float64 references, guards and bounds; the fixed case lists reach every kernel
arm they are there for (read from the addresses and sizes the cases really pass); and the checks raise on the
errors they are there to catch."""
import math

import pytest
import torch

import _cpu_emul as E
import step_tail_cases as SC
from fuxictr_amd import _lib

DEV = "cpu"
_arms = {}


def _run(group, cid):
    _arms.setdefault(group, {})[cid] = SC.run(group, cid, E, DEV)


@pytest.mark.parametrize("cid", SC.ids("mt"))
def test_multi_tensor_cases(cid):
    _run("mt", cid)


@pytest.mark.parametrize("cid", SC.ids("mt_agree"))
def test_multi_tensor_arm_agreement(cid):
    _run("mt_agree", cid)


@pytest.mark.parametrize("cid", SC.ids("clip") + SC.ids("clip_refusal"))
def test_clip_and_sum_parts_cases(cid):
    _run("clip_refusal" if cid in SC.ids("clip_refusal") else "clip", cid)


@pytest.mark.parametrize("cid", SC.ids("bce"))
def test_sigmoid_bce_cases(cid):
    _run("bce", cid)


@pytest.mark.parametrize("K", SC.HEAD_KS)
def test_head_train_cases(K):
    for cid in SC.ids("head"):
        if cid.startswith("K%d-" % K):
            _run("head", cid)


@pytest.mark.parametrize("cid", SC.ids("head_refusal"))
def test_head_train_refusals(cid):
    _run("head_refusal", cid)


@pytest.mark.parametrize("M", SC.COLSUM_MS)
def test_colsum_cases(M):
    for cid in SC.ids("colsum"):
        if cid.startswith("M%d-" % M):
            _run("colsum", cid)


def test_glue_cases():
    for group in ("mask_mul", "cross_prep"):
        for cid in SC.ids(group):
            _run(group, cid)


def test_every_case_ran_and_every_arm_is_reached():
    """Each list has the fixed length written down in step_tail_cases.COUNTS, every id is unique and has run (by the
    tests above; here if this test runs alone) — nothing skipped or filtered — and the union of the arms the cases
    report holds every arm the lists are there for."""
    for group, (cases, _) in SC.GROUPS.items():
        ids = [c["id"] for c in cases]
        assert len(ids) == SC.COUNTS[group] and len(set(ids)) == len(ids), group
        for cid in ids:
            if cid not in _arms.get(group, {}):
                _run(group, cid)
        assert set(_arms[group]) == set(ids), group
        reached = set().union(*_arms[group].values())
        assert SC.ARMS[group] <= reached, (group, sorted(SC.ARMS[group] - reached))


def test_the_chain_lengths_read_from_the_kernels():
    n = SC.MT_STRIDE * 4 + 5
    assert SC.MT_STRIDE == 96 * 256 and n == 98309
    assert SC.sqnorm_chain(n, True) == 2 * 4 + 1 + 8          # two float4 trips and the tail element of thread 0
    assert SC.sqnorm_chain(n, False) == 5 + 8                 # ceil(98309 / 24576) scalar trips
    assert SC.sqnorm_chain(0, True) == SC.sqnorm_chain(0, False) == 8
    assert SC.sqnorm_chain(1027, True) == 4 + 1 + 8
    assert [SC.colsum_chain(M) for M in SC.COLSUM_MS] == [21, 21, 21, 21, 21, 22]
    assert [SC.head_nu(K) for K in SC.HEAD_KS] == [(1, 1), (1, 1), (2, 2), (4, 3), (8, 5), (8, 8)]


def test_the_arena_sees_a_write_outside_the_addressed_elements():
    ar = SC.Arena(SC.Arena.need(12, 5 * 11), DEV)
    v = ar.vec(12, mod=1, write=True)
    m = ar.mat(5, 3, ld=11, col=4, write=True)
    ro = ar.vec(4, fill=torch.ones(4))
    ar.seal()
    assert v.data_ptr() % 16 == 4 and m.data_ptr() % 16 == 0 and m.stride(0) == 11
    assert bool(torch.isnan(v).all()) and bool(torch.isnan(m).all())
    v.fill_(1.0)
    m.fill_(2.0)
    ar.check("inside")
    with pytest.raises(AssertionError, match="outside"):
        ar.check("inside", untouched=True)
    for spoil in (lambda: ar.buf[v.storage_offset() - 1:v.storage_offset()].fill_(0.0),           # the float before
                  lambda: ar.buf[v.storage_offset() + 12:v.storage_offset() + 13].fill_(0.0),     # ... and behind
                  lambda: torch.as_strided(ar.buf, (1,), (1,), m.storage_offset() + 3).fill_(0.0),  # a gap column
                  lambda: ro[2:3].fill_(1.5)):                                                      # an input
        keep = ar.bits.clone()
        spoil()
        with pytest.raises(AssertionError, match="outside"):
            ar.check("spoiled")
        ar.bits.copy_(keep)
    ar.check("restored")


def test_the_exactness_input_needs_fp64():
    """What fx_sum_parts / fx_clip_coef accumulate in fp64 for: 1e8 followed by 4096 ones."""
    (case,) = [c for c in SC.CLIP_CASES if c.get("exact")]
    _, _, vals = SC._clip_parts(case, DEV)
    flat = torch.cat(vals)
    assert flat.numel() == 4097 and float(flat[0]) == 1e8
    run = torch.zeros((), dtype=torch.float32)
    for x in flat[:64]:
        run = run + x
    assert float(run) == 1e8                                   # an fp32 running sum loses every 1.0
    assert float(flat.double().sum()) == 100004096.0
    assert float(torch.tensor(100004096.0, dtype=torch.float32)) == 100004096.0
    out, scal = torch.zeros(1), E.new_scalars(DEV, max_norm=0.0)
    E.sum_parts(vals, out)
    E.clip_coef(vals, scal)
    assert float(out[0]) == 100004096.0
    assert float(scal[_lib.SC_TOTAL_NORM]) == float(torch.tensor(math.sqrt(100004096.0), dtype=torch.float32))
    assert float(scal[_lib.SC_CLIP]) == 1.0


def test_the_references_fail_on_the_errors_they_are_there_for(monkeypatch):
    """Each acceptance check against a stand-in that is subtly wrong: a skipped tail element, a tensor past the 64th
    left alone, a clip coefficient off by three roundings, an unclamped loss, a dropped mask column, a chunk of the
    column sum left out."""
    def broken(name, fn):
        monkeypatch.setattr(E, name, fn)

    good = {k: getattr(E, k) for k in ("mt_adam", "mt_sgd", "mt_sqnorm", "clip_coef", "sigmoid_bce", "head_train",
                                       "colsum", "cross_bwd_prep", "mask_mul")}

    def adam_without_tail(ps, gs, ms, vs, scal):                 # the vector loop without the scalar tail
        n4 = [p.numel() // 4 * 4 for p in ps]
        good["mt_adam"]([p[:n] for p, n in zip(ps, n4)], [g[:n] for g, n in zip(gs, n4)],
                        [m[:n] for m, n in zip(ms, n4)], [v[:n] for v, n in zip(vs, n4)], scal)
    broken("mt_adam", adam_without_tail)
    with pytest.raises(AssertionError):
        SC.run("mt", "adam-sizes-aligned-off", E, DEV)
    broken("mt_adam", lambda ps, gs, ms, vs, scal: good["mt_adam"](ps[:64], gs[:64], ms[:64], vs[:64], scal))
    with pytest.raises(AssertionError):
        SC.run("mt", "adam-count65", E, DEV)
    broken("mt_adam", good["mt_adam"])
    broken("mt_sgd", lambda ps, gs, scal: good["mt_sgd"](ps[:64], gs[:64], scal))
    with pytest.raises(AssertionError):
        SC.run("mt", "sgd-count130", E, DEV)
    broken("mt_sgd", good["mt_sgd"])

    def sqnorm_into_the_neighbour(grads, sq):                    # partial sums of tensor i land in tensor i + 1's slots
        good["mt_sqnorm"](grads, sq)
        sq.copy_(torch.roll(sq, _lib.FX_MT_BLOCKS))
    broken("mt_sqnorm", sqnorm_into_the_neighbour)
    with pytest.raises(AssertionError):
        SC.run("mt", "adam-count65", E, DEV)
    broken("mt_sqnorm", good["mt_sqnorm"])

    def clip_off(parts, scal):
        good["clip_coef"](parts, scal)
        scal[_lib.SC_CLIP] *= 1 - 6 * SC.U
    broken("clip_coef", clip_off)
    with pytest.raises(AssertionError):
        SC.run("clip", "parts16-below", E, DEV)
    with pytest.raises(AssertionError):
        SC.run("clip", "parts1-len5000-off", E, DEV)             # max_norm = 0: exactly 1.0
    broken("clip_coef", good["clip_coef"])

    def bce_unclamped(logit, y, prob=None, loss=None, dlogit=None):
        good["sigmoid_bce"](logit, y, prob=prob, loss=loss, dlogit=dlogit)
        if loss is not None:
            loss.fill_(float(torch.nn.functional.binary_cross_entropy_with_logits(logit.double(), y.double())))
    broken("sigmoid_bce", bce_unclamped)
    with pytest.raises(AssertionError):
        SC.run("bce", "sat+104-y0", E, DEV)
    with pytest.raises(AssertionError):
        SC.run("bce", "B1025", E, DEV)
    broken("sigmoid_bce", good["sigmoid_bce"])

    def head_mask_one_column_late(h, W, bias, add, y, mask_from, *rest):
        good["head_train"](h, W, bias, add, y, mask_from + 4 if mask_from >= 0 else mask_from, *rest)
    broken("head_train", head_mask_one_column_late)
    with pytest.raises(AssertionError, match="dz"):
        SC.run("head", "K12-M5", E, DEV)                         # mask_from = 0
    broken("head_train", good["head_train"])

    def colsum_without_the_last_row(X, out, ws):
        return good["colsum"](X[:-1] if X.shape[0] > 64 else X, out, ws)
    broken("colsum", colsum_without_the_last_row)
    with pytest.raises(AssertionError):
        SC.run("colsum", "M65-N4-contiguous", E, DEV)
    broken("colsum", good["colsum"])

    def prep_always_adds(dxn, x0, z, t, dx0, init, add_dxn):
        good["cross_bwd_prep"](dxn, x0, z, t, dx0, init, True)
    broken("cross_bwd_prep", prep_always_adds)
    with pytest.raises(AssertionError, match="dx0"):
        SC.run("cross_prep", "7x3-dxn1-init0-add0", E, DEV)
    broken("cross_bwd_prep", good["cross_bwd_prep"])

    def mask_ge(dy, y, out):                                     # y >= 0 instead of y > 0
        out.copy_(torch.where(y >= 0, dy, torch.zeros(())))
    broken("mask_mul", mask_ge)
    with pytest.raises(AssertionError, match="exact"):
        SC.run("mask_mul", "7x3-dy1-y1", E, DEV)


def test_the_emulation_refuses_what_the_entry_points_refuse():
    parts = [torch.ones(1)] * (_lib.FX_CLIP_MAX_PARTS + 1)
    with pytest.raises(_lib.FxError, match="n_parts=17"):
        E.sum_parts(parts, torch.zeros(1))
    with pytest.raises(_lib.FxError, match="n_parts=17"):
        E.clip_coef(parts, E.new_scalars(DEV))
    E.sum_parts(parts[:16], torch.zeros(1))
