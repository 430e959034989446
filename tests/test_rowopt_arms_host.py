"""tests/rowopt_cases.py without a GPU: its mirror of fx_row_geom reaches the arms tests/test_gpu_rowopt_arms.py
claims, every record `_TableGroup` can build for those widths is aligned for its vector accesses, the bf16 rounding the
GPU tests expect is round-to-nearest-even, and each acceptance check raises on the error it is there to catch (the
fp32 torch reference stands in for the kernel)."""
import numpy as np
import pytest
import torch

import rowopt_cases as RC
from fuxictr_amd.layers import _TableGroup
from rowopt_cases import DS, LR, R, ROWS, T0

UPTO = T0 + 5


def test_the_width_list_reaches_every_vec_lane_count_and_idle_lane():
    geo = {D: RC.geometry(D) for D in DS}
    assert geo == {1: (1, 1), 2: (2, 1), 3: (1, 4), 6: (2, 4), 12: (4, 4), 16: (4, 4), 40: (4, 16), 65: (1, 128),
                   130: (2, 128), 255: (1, 256), 256: (4, 64)}
    assert {v for v, _ in geo.values()} == {1, 2, 4}
    assert {l for _, l in geo.values()} == {1, 4, 16, 64, 128, 256}
    idle = [D for D in DS if RC.idle_lane(D)]
    assert {6, 12, 40, 130} <= set(idle) and len(idle) >= 4
    assert not RC.idle_lane(16) and not RC.idle_lane(256) and not RC.idle_lane(1)
    # the quad's lane group (4 lanes of vec 4) is shared by a width that is not the quad's
    assert geo[12] == geo[16]


@pytest.mark.parametrize("D", DS)
def test_every_record_is_aligned_for_the_vector_accesses(D):
    """What the argument guard of fx_fill_tables asks of a state, on the record _TableGroup builds: the row stride and
    the field offsets D, 2D, 3D are multiples of vec; rows start on 16 bytes."""
    vec, _ = RC.geometry(D)
    W = _TableGroup.record_width(D)
    assert W >= 3 * D + 1 and W % 4 == 0 and W % vec == 0
    assert all(off % vec == 0 for off in (0, D, 2 * D))
    _, _, _, _, st = RC.make_state(D, R, "fp32", "record", 0)
    assert st.blocks[0].shape == (R + 2, W)
    for f in (st.table, st.m, st.v):
        assert f.stride(0) == W and f.stride(0) % vec == 0 and f.data_ptr() % (4 * vec) == 0
        assert f.shape == (R, D)
    assert st.last_step.stride(0) == W and st.last_step.dtype == torch.int32
    assert st.last_step.data_ptr() == st.table.data_ptr() + 4 * 3 * D
    # packed arrays behind one guard row start D elements in: aligned for vec as well, bf16 included
    for dtype, eb in (("fp32", 4), ("bf16", 2)):
        _, _, _, _, pk = RC.make_state(D, R, dtype, "packed", 0)
        assert pk.table.data_ptr() % (eb * vec) == 0 and pk.m.data_ptr() % (4 * vec) == 0


def test_torch_bfloat16_rounds_to_nearest_even():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(4000) * np.exp(rng.uniform(-30, 30, 4000))).astype(np.float32)
    bits = rng.integers(0, 1 << 16, 64).astype(np.uint32) << 16
    ties = np.concatenate([bits | 0x8000, bits | 0x7FFF, bits | 0x8001]).view(np.float32)
    ties = ties[np.isfinite(ties)]
    fmax = np.float32(np.finfo(np.float32).max)
    x = np.concatenate([x, ties, np.asarray([np.inf, -np.inf, fmax, -fmax, 0.0, -0.0, 1e-45], dtype=np.float32)])
    got = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, RC.bf16_rne(x))
    assert RC.bf16_rne(fmax)[()] == 0x7F80                      # the largest finite value rounds up to infinity
    assert RC.bf16_rne(np.float32(1.00390625))[()] == 0x3F80     # a tie to the even neighbour below
    assert RC.bf16_rne(np.float32(1.01171875))[()] == 0x3F82     # ... and to the even neighbour above


def _stand_in(D, layout, dtype="fp32"):
    """A catch-up 'run' by the fp32 torch reference, written into the state's own fields."""
    p, m, v, last, st = RC.make_state(D, R, dtype, layout, 0)
    refs = [RC.ref_catchup(p[ROWS], m[ROWS], v[ROWS], last[ROWS], UPTO, LR, f64) for f64 in (False, True)]
    st.table[ROWS] = refs[0][0].to(st.table.dtype)
    st.m[ROWS], st.v[ROWS] = refs[0][1], refs[0][2]
    st.last_step[ROWS] = UPTO
    return st, refs


def _accept(st, refs):
    RC.guards_intact(st)
    got = tuple(x[ROWS] for x in st.fields())
    return RC.check_fp32(got, refs[0], refs[1], UPTO, "stand-in")


@pytest.mark.parametrize("layout", ["packed", "record"])
@pytest.mark.parametrize("D", [6, 16])
def test_the_checks_pass_on_the_reference_and_fail_on_each_perturbation(D, layout):
    st, refs = _stand_in(D, layout)
    assert _accept(st, refs) <= 1.0
    # one element moved by 3e-6
    st, refs = _stand_in(D, layout)
    st.table[ROWS[3], D - 1] += 3e-6
    with pytest.raises(AssertionError, match="stand-in"):
        _accept(st, refs)
    # ... one moment by 3e-6
    st, refs = _stand_in(D, layout)
    st.v[ROWS[5], 0] += 3e-6
    with pytest.raises(AssertionError, match="'v'"):
        _accept(st, refs)
    # one last_step stamp off by one
    st, refs = _stand_in(D, layout)
    st.last_step[ROWS[-1]] -= 1
    with pytest.raises(AssertionError, match="last_step"):
        _accept(st, refs)
    # the neighbour row's first element overwritten (a vec-4 store on a narrower row, a wrong stride)
    st, refs = _stand_in(D, layout)
    assert 0 in ROWS and 1 not in ROWS
    st.table[1, 0] = 0.5
    with pytest.raises(AssertionError, match="written outside the listed rows"):
        _accept(st, refs)
    # a stale entry of uniq_row read as a row: the stamp of the guard row behind the table
    st, refs = _stand_in(D, layout)
    st.blocks[-1].view(torch.int32)[R + 1, ...].fill_(UPTO)
    with pytest.raises(AssertionError, match="written outside the listed rows"):
        _accept(st, refs)


@pytest.mark.parametrize("D", [2, 6, 16])
def test_a_changed_padding_float_fails_the_guard_check(D):
    st, refs = _stand_in(D, "record")
    W = st.blocks[0].shape[1]
    assert W > 3 * D + 1                                        # (D = 1 fills its 4-float record: no padding)
    st.blocks[0][1 + ROWS[2], W - 1] = 0.0
    with pytest.raises(AssertionError, match="written outside the listed rows"):
        _accept(st, refs)


def test_a_bf16_element_one_ulp_off_fails_the_bf16_check():
    st32, _ = _stand_in(6, "packed")
    st16, _ = _stand_in(6, "packed", dtype="bf16")
    st16.table[:] = st32.table.bfloat16()
    RC.check_bf16(st16.fields(), st32.fields(), "stand-in")
    bits = st16.table.view(torch.int16)
    bits[ROWS[4], 5] += 1
    with pytest.raises(AssertionError, match="table"):
        RC.check_bf16(st16.fields(), st32.fields(), "stand-in")
    bits[ROWS[4], 5] -= 1
    st16.m.view(torch.int32)[ROWS[0], 0] ^= 1                   # the moments: the same bits, not "close"
    with pytest.raises(AssertionError, match="field 0"):
        RC.check_bf16(st16.fields(), st32.fields(), "stand-in")


def test_bit_equality_sees_one_bit():
    st_a, _ = _stand_in(12, "packed")
    st_b, _ = _stand_in(12, "record")
    RC.check_same_bits(st_a.fields(), st_b.fields(), "record == packed")
    st_b.table.view(torch.int32)[ROWS[1], 11] ^= 1
    with pytest.raises(AssertionError, match="field 0"):
        RC.check_same_bits(st_a.fields(), st_b.fields(), "record == packed")


def test_the_update_reference_is_the_dense_step_with_the_regularizer_inside_the_clip():
    """ref_update against the closed form of the SGD step, p - lr * clip * (g + l1 sign(p) + l2 p), in fp64, and
    against itself without the regularizer."""
    p, m, v, _ = RC.host_case(6, 0)
    g = torch.randn(R, 6, generator=torch.Generator().manual_seed(1)) * 0.1
    out = RC.ref_update("sgd", p, m, v, g, T0 + 1, LR, 0.4, 3e-3, 2e-2, True)[0]
    want = p.double() - LR * 0.4 * (g.double() + 3e-3 * torch.sign(p.double()) + 2e-2 * p.double())
    assert (out - want).abs().max().item() <= 1e-15
    a = RC.ref_update("adam", p, m, v, g, T0 + 1, LR, 0.4, 0.0, 0.0, False)
    b = RC.ref_update("adam", p, m, v, g, T0 + 1, LR, 0.4, 3e-3, 2e-2, False)
    assert a[0].dtype == torch.float32 and not torch.equal(a[0], b[0])
