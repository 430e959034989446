"""Cases, references and acceptance checks of the sparse row optimizer (csrc/fx_rowopt.hip), shared by
tests/test_gpu_rowopt_arms.py (the kernels on an MI355X) and tests/test_rowopt_arms_host.py (the checks themselves,
no GPU).  A plain module: no fixtures.

A case is one table of R rows between two guard rows, as four packed arrays or as the [p | m | v | last_step] row
record of `_TableGroup._set_record`, with every float that no kernel may write — guard rows, record padding — set to
one bit pattern.  The references are dense torch Adam / SGD (oracle.ctr_oracle) on the rows a launch lists, once in
fp32 and once in fp64; no arithmetic of the kernels is restated here.  Every tolerance is one the suite already
carries: the fp64 yardstick and the 1e-6 of the moments (tests/test_gpu_kernels.py), and bit equality."""
import types

import numpy as np
import torch

from fuxictr_amd import ops
from fuxictr_amd.layers import _TableGroup
from oracle import ctr_oracle as O

DS = [1, 2, 3, 6, 12, 16, 40, 65, 130, 255, 256]
R = 37
ROWS = [r for r in range(R) if r % 3 != 1]              # the unique rows of a launch: 25 of 37, rows 0 and R - 1 in
IDS = ROWS[7:] + ROWS[:7] + ROWS[3:18]                  # the lookups: every listed row, 15 of them twice
NEVER = [r for r in range(R) if r % 5 == 2]             # rows no step has touched: m = v = 0, last_step = 0
T0 = 3                                                  # the dense steps every other row has behind it
LR = 1e-2
FILL = 0x4B3C614E                                       # guard rows / padding (fp32 12345678.0; bf16: the high half)


def geometry(D):
    """fx_row_geom of fx_common.h: -> (vec, lanes)."""
    vec = 4 if D % 4 == 0 else (2 if D % 2 == 0 else 1)
    lanes = 1
    while lanes < D // vec:
        lanes *= 2
    return vec, lanes


def idle_lane(D):
    """The lane group of a D-float row has a lane that holds no element (r.act && !r.on)."""
    vec, lanes = geometry(D)
    return (lanes - 1) * vec >= D


def within_yardstick(native, ref32, ref64, floor, what):
    """|native - fp64 Adam| <= max(floor, 1.5 x |torch-fp32 Adam - fp64 Adam|): the reference itself rounds p
    at every step (k roundings of up to half an ulp each); the native path is held to being as close to the
    exact trajectory as the reference's own fp32 stepping is, on the same rows, not to a fixed number that one
    rounding sequence happens to meet."""
    e_nat = (native.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    assert e_nat <= max(floor, 1.5 * e_ref), (what, e_nat, e_ref)
    return e_nat, e_ref


class CaseState(ops.RowState):
    """ops.RowState + what guards_intact needs: the blocks the fields are views of and their first bits."""

    def bits(self):
        return [b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32) for b in self.blocks]

    def fields(self):
        """-> host copies of (table, m, v, last_step) as compact arrays (None where the state has none)."""
        return tuple(None if x is None else x.detach().cpu().contiguous().clone()
                     for x in (self.table, self.m, self.v, self.last_step))


def host_case(D, seed, representable=False):
    """-> host fp32 p, m, v [R, D] and int32 last [R]: T0 real dense Adam steps from zero moments (|m| / sqrt(v) as
    bounded as in a run), the rows of NEVER left untouched."""
    g = torch.Generator().manual_seed(1000 * D + seed)
    p = torch.randn(R, D, generator=g)
    m, v = torch.zeros(R, D), torch.zeros(R, D)
    p0 = p.clone()
    for t in range(1, T0 + 1):
        O.adam_dense(p, torch.randn(R, D, generator=g) * 0.1, m, v, t, LR)
    last = torch.full((R,), T0, dtype=torch.int32)
    p[NEVER], m[NEVER], v[NEVER], last[NEVER] = p0[NEVER], 0.0, 0.0, 0
    if representable:
        p = p.bfloat16().float()
    return p, m, v, last


def make_state(D, R_, dtype, layout, seed, device="cpu", adam=True, representable=None):
    """-> host fp32 p, m, v, last and the CaseState on `device`.  dtype "fp32" | "bf16" (packed only: the product builds
    no bf16 record); layout "packed" | "record".  representable: p holds bf16 values (default: for a bf16 table; pass
    True with "fp32" for the widened twin of one).  adam=False: no moments (the SGD state)."""
    assert R_ == R and dtype in ("fp32", "bf16") and layout in ("packed", "record")
    assert not (dtype == "bf16" and layout == "record")
    if representable is None:
        representable = dtype == "bf16"
    p, m, v, last = host_case(D, seed, representable)
    st = CaseState(None, None, None, None, D)
    st.layout = layout
    if layout == "record":
        W = _TableGroup.record_width(D)
        block = torch.full((R + 2, W), FILL, dtype=torch.int32).view(torch.float32)
        rec = block[1:R + 1]
        rec[:, :D], rec[:, D:2 * D], rec[:, 2 * D:3 * D] = p, m, v
        rec.view(torch.int32)[:, 3 * D] = last
        block = block.to(device)
        rec = block[1:R + 1]
        # the four fields, as _TableGroup._set_record makes them
        st.table, st.m, st.v = rec[:, :D], rec[:, D:2 * D], rec[:, 2 * D:3 * D]
        st.last_step = rec.view(torch.int32)[:, 3 * D]
        st.blocks = [block]
    else:
        def guarded(x, dt):
            if dt == torch.bfloat16:
                b = torch.full((R + 2,) + tuple(x.shape[1:]), FILL >> 16, dtype=torch.int16).view(torch.bfloat16)
            else:
                b = torch.full((R + 2,) + tuple(x.shape[1:]), FILL, dtype=torch.int32).view(dt)
            b[1:R + 1] = x.to(dt)
            return b.to(device)
        st.blocks = [guarded(p, torch.bfloat16 if dtype == "bf16" else torch.float32)]
        if adam:
            st.blocks += [guarded(m, torch.float32), guarded(v, torch.float32)]
        st.blocks.append(guarded(last, torch.int32))
        views = [b[1:R + 1] for b in st.blocks]
        st.table, st.last_step = views[0], views[-1]
        if adam:
            st.m, st.v = views[1], views[2]
    if layout == "record" and not adam:
        st.m = st.v = None
    st.init = [b.clone() for b in st.bits()]
    return p, m, v, last, st


def guards_intact(state, rows=ROWS):
    """Guard rows, record padding and every row outside `rows` carry their first bits (bf16 tables as int16): a store
    of the wrong width or stride lands in one of them."""
    D = state.D
    for k, (now, init) in enumerate(zip(state.bits(), state.init)):
        free = torch.zeros(now.shape, dtype=torch.bool)
        idx = torch.as_tensor(list(rows), dtype=torch.long) + 1
        if state.layout == "record":
            free[idx, :3 * D + 1] = True
        else:
            free[idx] = True
        same = (now.cpu() == init.cpu()) | free
        bad = (~same).nonzero()
        assert bad.numel() == 0, ("written outside the listed rows: block %d of a %s D=%d state at %s"
                                  % (k, state.layout, D, bad[:4].tolist()))


def flush_listed(state, rows, total_rows, upto, upto_offset, scal):
    """The plain replay of `rows` alone up to step `upto` (= the step of `scal` + upto_offset): fx_adam_catchup_all on
    `state` with every other row stamped `upto` for the launch, so that the flush skips it, and its stamp put back.
    fx_adam_catchup_rows hands a D = 16 table alone to the quad replay; the flush is k_catchup_all, which calls the
    fx_catchup_row of the non-quad arm of k_catchup_rows with the same scalars."""
    last = state.last_step
    unlisted = torch.ones(total_rows, dtype=torch.bool, device=last.device)
    unlisted[torch.as_tensor(rows, dtype=torch.long, device=last.device)] = False
    stale = last[unlisted].clone()
    last[unlisted] = upto
    ops.adam_catchup_all(state, total_rows, upto_offset, scal)
    last[unlisted] = stale


def _reg_grad(p, l1, l2):
    """d/dp of the embedding regularizer as ctr_oracle.OracleTrainer.regularization_loss states it
    (rank_model.py:95-118): sum over (norm, lambda) of lambda / norm * ||p||_norm ^ norm."""
    terms = [(n, lam) for n, lam in ((1, l1), (2, l2)) if lam != 0.0]
    if not terms:
        return torch.zeros_like(p)
    q = p.detach().clone().requires_grad_(True)
    stub = types.SimpleNamespace(params=[q], is_emb=[True], emb_reg=terms, net_reg=[])
    O.OracleTrainer.regularization_loss(stub).backward()
    return q.grad.detach()


def ref_update(kind, p, m, v, g, t, lr, clip, l1, l2, dtype64):
    """One dense optimizer step of the rows p (their gradients g) with the regularizer inside the clipped gradient:
    -> (p, m, v) in fp32 (dtype64 False) or fp64."""
    dt = torch.float64 if dtype64 else torch.float32
    p, g = p.to(dt).clone(), g.to(dt)
    grad = (g + _reg_grad(p, l1, l2)) * clip
    if kind == "sgd":
        return p - lr * grad, None, None
    m, v = m.to(dt).clone(), v.to(dt).clone()
    O.adam_dense(p, grad, m, v, t, lr)
    return p, m, v


def ref_catchup(p, m, v, last, upto, lr, dtype64):
    """The zero-gradient steps last + 1 .. upto of dense Adam, row by row of `last`: -> (p, m, v)."""
    dt = torch.float64 if dtype64 else torch.float32
    p, m, v = p.to(dt).clone(), m.to(dt).clone(), v.to(dt).clone()
    for first in sorted(set(last.tolist())):
        sel = (last == first).nonzero().view(-1)
        ps, ms, vs = p[sel], m[sel], v[sel]
        for t in range(first + 1, upto + 1):
            O.adam_dense(ps, torch.zeros_like(ps), ms, vs, t, lr)
        p[sel], m[sel], v[sel] = ps, ms, vs
    return p, m, v


# ---- acceptance (every rule is one an existing test carries) -------------------------------------------------
def check_fp32(got, ref32, ref64, stamp, what):
    """got = (table, m, v, last_step) of the listed rows of an fp32 table against the references (p, m, v) of the
    same rows: p by the fp64 yardstick (floor 2e-6), m and v within 1e-6 of the fp32 reference, the stamps exact.
    -> error / yardstick of p."""
    p, m, v, last = got
    e_nat, e_ref = within_yardstick(p, ref32[0], ref64[0], 2e-6, what)
    if ref32[1] is not None:
        assert (m - ref32[1]).abs().max().item() <= 1e-6, (what, "m")
        assert (v - ref32[2]).abs().max().item() <= 1e-6, (what, "v")
    assert last.tolist() == [stamp] * len(last), (what, "last_step", last.tolist())
    return e_nat / max(2e-6, 1.5 * e_ref)


def _bits(x):
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16)
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def check_same_bits(a, b, what):
    """Two (table, m, v, last_step) results, or any two tuples of arrays, bit for bit."""
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), (what, "field %d" % k)


def check_bf16(got16, got32, what):
    """A bf16 table after a launch == the fp32 launch on the widened table rounded once to nearest-even; the moments
    and stamps of the two runs are the same bits."""
    assert got16[0].dtype == torch.bfloat16 and got32[0].dtype == torch.float32, what
    assert torch.equal(_bits(got16[0]), _bits(got32[0].bfloat16())), (what, "table")
    check_same_bits(got16[1:], got32[1:], what)


def bf16_rne(x):
    """float32 -> bfloat16 bits by round-to-nearest-even, in integer numpy (NaN excluded)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)
