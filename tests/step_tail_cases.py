"""Cases, float64 references and acceptance checks of the launches that end every training step, shared by
tests/test_gpu_step_tail.py (the kernels on an MI355X: `backend` = fuxictr_amd.ops) and tests/test_step_tail_host.py
(the same cases on tests/_cpu_emul.py, no GPU).  A plain module: no fixtures.

  1. fx_mt_sqnorm / fx_mt_adam / fx_mt_sgd (end of csrc/fx_sparse.hip) and the chunking of ops.mt_*
  2. fx_clip_coef / fx_sum_parts
  3. fx_sigmoid_bce              4. fx_head_train + k_head_reduce
  5. fx_colsum                   6. fx_mask_mul / fx_cross_bwd_prep     (3 - 6: csrc/fx_dense_misc.hip)

Every operand lives in an Arena: one flat buffer filled with a NaN bit pattern, the operands views into it with at
least 8 guard floats on either side (and the gap columns of a strided view between its rows).  After a call every
float outside the elements the call may write carries its first bits: inputs, guard floats, gap columns and the
workspace behind the size the product reports.  Workspaces start as NaN: a slab that is read without having been
written ends up in the result.

The case lists are fixed (no random omission); each run_* returns the names of the kernel arms the case reached, read
from the addresses and sizes it really passed.  Every bound is derived beside its assert from the kernel's operation
count (U = 2^-24, the unit roundoff of fp32), or is one the suite already carries."""
import math

import pytest
import torch

from fuxictr_amd import _lib
from oracle import ctr_oracle as O
from rowopt_cases import within_yardstick

U = 2.0 ** -24
NAN_BITS = 0x7FC0BEEF
GAP = 8
MT_STRIDE = _lib.FX_MT_BLOCKS * 256          # elements (scalar arm) / float4s (vector arm) per grid trip


def _bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu())), what


class Arena(object):
    """A flat fp32 buffer of NaNs on `dev`; vec() / mat() hand out views of it, `write` marks the elements a call may
    change.  seal() uploads the fills and remembers every bit; check() compares."""

    def __init__(self, floats, dev):
        self.stage = torch.full((floats,), NAN_BITS, dtype=torch.int32).view(torch.float32)
        self.bits = torch.full((floats,), NAN_BITS, dtype=torch.int32, device=dev)
        self.buf = self.bits.view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.free = torch.zeros(floats, dtype=torch.bool)
        self.cur, self.cap, self.dev, self.slots = 0, floats, dev, []

    @staticmethod
    def need(*spans):
        return sum(int(s) + 2 * GAP + 16 for s in spans)

    def _view(self, t, slot):
        s, shape, ld = slot
        return t[s:s + shape[0]] if len(shape) == 1 else torch.as_strided(t, shape, (ld, 1), s)

    def _take(self, span, mod, shape, ld, col, write, fill):
        start = -(-self.cur // 4) * 4 + GAP + mod
        self.cur = start + span + GAP
        assert self.cur <= self.cap, "arena too small"
        slot = (start + col, shape, ld)
        self.slots.append(slot)
        if write:
            self._view(self.free, slot)[...] = True
        if fill is not None:
            self.put(len(self.slots) - 1, fill)
        return self._view(self.buf, slot)

    def vec(self, n, mod=0, write=False, fill=None):
        """n floats starting `mod` floats behind a 16-byte boundary."""
        return self._take(n, mod, (n,), 1, 0, write, fill)

    def mat(self, M, N, ld=None, col=0, write=False, fill=None):
        """[M, N] with row stride ld, starting `col` floats behind a 16-byte boundary (the rest of a row: gap)."""
        ld = N if ld is None else ld
        assert col + N <= ld
        return self._take(M * ld, 0, (M, N), ld, col, write, fill)

    def put(self, k, values):
        self._view(self.stage, self.slots[k])[...] = values.reshape(self.slots[k][1])

    def seal(self):
        self.bits.copy_(self.stage.view(torch.int32))
        self.init = self.bits.clone()
        self.free_dev = self.free.to(self.dev)
        return self

    def check(self, what, untouched=False):
        changed = self.bits != self.init
        if not untouched:
            changed &= ~self.free_dev
        bad = changed.nonzero().view(-1)
        assert bad.numel() == 0, ("written outside the addressed elements", what, bad[:6].tolist())


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _aligned(t):
    return t.data_ptr() % 16 == 0


# =====================================================================================================================
# 1. multi-tensor squared norm / Adam / SGD
# =====================================================================================================================
MT_LR = 1e-2
MT_STEPS = 3
MT_ALIGN = {"aligned": (0, 0, 0, 0), "g_off": (0, 1, 0, 0), "m_off": (0, 0, 2, 0), "all_off": (1, 2, 3, 5)}
MT_REGIMES = ("off", "above", "below")          # max_norm = 0 | far above the norm | below it
MT_SIZES = [1, 0, 3, 4, 5, 1023, 1024, 1027, MT_STRIDE * 4 + 5, None]      # None: a fresh torch.empty(0)
MT_SMALL = [5, 0, 1, 3, 4, 9, 12, 33]
MT_COUNTS = [1, 64, 65, 130]


def _mt_cases():
    out = []
    for kind in ("adam", "sgd"):
        for al in MT_ALIGN:
            for reg in MT_REGIMES:
                out.append(dict(id="%s-sizes-%s-%s" % (kind, al, reg), kind=kind, sizes=MT_SIZES,
                                offs=[MT_ALIGN[al]] * len(MT_SIZES), regime=reg, seed=1))
        names = list(MT_ALIGN)
        for n in MT_COUNTS:
            out.append(dict(id="%s-count%d" % (kind, n), kind=kind, sizes=[MT_SMALL[i % 8] for i in range(n)],
                            offs=[MT_ALIGN[names[i % 4]] for i in range(n)], regime="below", seed=2))
        out.append(dict(id="%s-lone-empty" % kind, kind=kind, sizes=[None], offs=[MT_ALIGN["aligned"]],
                        regime="below", seed=3))
    return out


MT_CASES = _mt_cases()
MT_AGREE_CASES = [dict(id="agree-" + reg, regime=reg) for reg in MT_REGIMES]


def sqnorm_chain(n, vec):
    """The longest addition chain of one element of k_mt_sqnorm: the fmaf's of the busiest thread (thread 0 of block 0:
    4 per float4 trip of MT_STRIDE float4s and one for a tail element on the vector arm, one per trip of MT_STRIDE
    floats on the scalar arm), the 6 levels of fx_wave_sum and the 2 of fx_block_sum_256's (r0 + r1) + (r2 + r3)."""
    if vec:
        trips = 4 * -(-(n // 4) // MT_STRIDE) + (1 if n % 4 else 0)
    else:
        trips = -(-n // MT_STRIDE)
    return trips + 6 + 2


def _mt_values(sizes, seed):
    g = torch.Generator().manual_seed(4242 + seed)
    ns = [0 if n is None else n for n in sizes]
    p0 = [torch.randn(n, generator=g) for n in ns]
    grads = [[torch.randn(n, generator=g) * 0.1 for n in ns] for _ in range(MT_STEPS)]
    return ns, p0, grads


def _mt_max_norm(regime, grads):
    norm = math.sqrt(sum(float((x.double() ** 2).sum()) for x in grads[0]))
    return {"off": 0.0, "above": 1e6 * max(norm, 1.0), "below": 0.5 * norm}[regime]


class _MtState(object):
    """p, g, m, v of one tensor list as views of four arenas (one per role), each at its own offset past 16 bytes."""

    def __init__(self, sizes, offs, p0, dev):
        ns = [0 if n is None else n for n in sizes]
        cap = Arena.need(*ns) + 16
        self.arenas = [Arena(cap, dev) for _ in range(4)]          # p, g, m, v
        self.t = [[], [], [], []]
        self.slot = []
        for i, n in enumerate(sizes):
            if n is None:
                for r in range(4):
                    self.t[r].append(torch.empty(0, device=dev))
                self.slot.append(None)
                continue
            self.slot.append(len(self.arenas[0].slots))
            for r in range(4):
                fill = p0[i] if r == 0 else (None if r == 1 else torch.zeros(n))
                self.t[r].append(self.arenas[r].vec(n, mod=offs[i][r], write=r != 1, fill=fill))
        for a in self.arenas:
            a.seal()

    def set_grads(self, gs):
        for i, k in enumerate(self.slot):
            if k is not None:
                self.arenas[1].put(k, gs[i])
        self.arenas[1].seal()

    def check(self, what, roles=(0, 1, 2, 3)):
        for r in roles:
            self.arenas[r].check((what, "pgmv"[r]))

    def host(self, r):
        return [x.cpu().clone() for x in self.t[r]]

    def arms(self, kind):
        out = set()
        for p, g, m, v in zip(*self.t):
            n = p.numel()
            if n == 0:
                out.add("mt.empty")
                continue
            sv = _aligned(g)
            out.add("sqnorm.vec" if sv else "sqnorm.scalar")
            if sv and n // 4 > MT_STRIDE:
                out.add("sqnorm.vec.wrap")
            if sv and n % 4:
                out.add("sqnorm.vec.tail")
            if not sv and n > MT_STRIDE:
                out.add("sqnorm.scalar.wrap")
            if kind == "sgd":
                out.add("sgd.wrap" if n > MT_STRIDE else "sgd")
                continue
            av = all(_aligned(x) for x in (p, g, m, v))
            out.add("adam.vec" if av else "adam.scalar")
            if av and n // 4 > MT_STRIDE:
                out.add("adam.vec.wrap")
            if av and n % 4:
                out.add("adam.vec.tail")
            if not av and n > MT_STRIDE:
                out.add("adam.scalar.wrap")
            if sv and not av:
                out.add("sqnorm.vec+adam.scalar")
        chunks = -(-len(self.t[0]) // _lib.FX_MT_MAX)
        out.add("mt.chunks%d" % chunks)
        return out


def _mt_norm_and_clip(B, st, scal, sq_arena, sq, what):
    """fx_mt_sqnorm + fx_clip_coef on the state's gradients; the partial sums of every tensor against float64.
    -> (coef the launch wrote, coef in float64, max chain)."""
    NB = _lib.FX_MT_BLOCKS
    B.mt_sqnorm(st.t[1], sq)
    B.clip_coef([sq], scal)
    _sync(sq.device)
    sq_arena.check((what, "sq_partials"))
    st.check(what)
    parts = sq.cpu().double().view(-1, NB).sum(1)
    total, cmax = 0.0, 8
    for i, g in enumerate(st.t[1]):
        s64 = float((g.cpu().double() ** 2).sum())
        total += s64
        # every partial is off by at most c U (its own share of sum g^2); so is their sum over the 96 blocks
        c = sqnorm_chain(g.numel(), _aligned(g))
        cmax = max(cmax, c)
        assert abs(float(parts[i]) - s64) <= c * U * s64, (what, "tensor %d of %d floats" % (i, g.numel()), c,
                                                          float(parts[i]), s64)
    mx = float(scal[_lib.SC_MAX_NORM])
    coef64 = min(1.0, mx / (math.sqrt(total) + 1e-6)) if mx > 0 else 1.0
    return float(scal[_lib.SC_CLIP]), coef64, cmax


def run_mt(case, B, dev):
    what = case["id"]
    kind = case["kind"]
    ns, p0, grads = _mt_values(case["sizes"], case["seed"])
    st = _MtState(case["sizes"], case["offs"], p0, dev)
    NB = _lib.FX_MT_BLOCKS
    sq_arena = Arena(Arena.need(len(ns) * NB), dev)
    sq = sq_arena.vec(len(ns) * NB, write=True)
    sq_arena.seal()
    scal = B.new_scalars(dev, lr=MT_LR, max_norm=_mt_max_norm(case["regime"], grads))
    ref = {dt: ([p.to(dt).clone() for p in p0], [torch.zeros(n, dtype=dt) for n in ns],
                [torch.zeros(n, dtype=dt) for n in ns]) for dt in (torch.float32, torch.float64)}
    for t in range(1, MT_STEPS + 1):
        gs = grads[t - 1]
        st.set_grads(gs)
        B.opt_begin_step(scal)
        coef, coef64, cmax = _mt_norm_and_clip(B, st, scal, sq_arena, sq, (what, t))
        if case["regime"] == "below" and sum(ns) > 0:
            # the sum of the partials is off by cmax U, its root by half of that; then fx_clip_coef's 2^-22 (group 2)
            assert coef < 1.0 and abs(coef - coef64) <= (cmax * U + 2.0 ** -22) * coef64, (what, t, coef, coef64)
        else:
            assert coef == 1.0, (what, t, coef)
        before = st.host(0)
        if kind == "adam":
            B.mt_adam(st.t[0], st.t[1], st.t[2], st.t[3], scal)
        else:
            B.mt_sgd(st.t[0], st.t[1], scal)
        _sync(dev)
        st.check((what, t))
        sq_arena.check((what, t, "sq_partials"))
        got = [st.host(r) for r in (0, 2, 3)]
        if kind == "sgd":
            scale = float(scal[_lib.SC_LR]) * coef
            for i, (was, now, g) in enumerate(zip(before, got[0], gs)):
                step = scale * g.double()
                want = was.double() - step
                # p - (lr clip) g: the rounding of the scale and of the product (2 U |step|), of the difference
                # (U |p|), or one rounding of a fused multiply-add; held at 2^-23 (|p| + 2 |step|)
                bound = 2 * U * (was.double().abs() + 2 * step.abs())
                assert bool(((now.double() - want).abs() <= bound).all()), (what, t, "sgd tensor %d" % i)
            for r in (2, 3):
                same_bits(torch.cat(st.host(r)), torch.zeros(sum(ns)), (what, t, "sgd wrote a moment"))
            continue
        for dt, cf in ((torch.float32, float(torch.tensor(coef64, dtype=torch.float32))), (torch.float64, coef64)):
            P, M, V = ref[dt]
            for p, g, m, v in zip(P, gs, M, V):
                O.adam_dense(p, g.to(dt) * cf, m, v, t, MT_LR)
        if sum(ns):
            for k, (name, floor) in enumerate((("p", 2e-6), ("m", 1e-6), ("v", 1e-6))):
                within_yardstick(torch.cat(got[k]), torch.cat(ref[torch.float32][k]), torch.cat(ref[torch.float64][k]),
                                 floor, (what, t, name))
    return st.arms(kind)


def run_mt_agree(case, B, dev):
    """An aligned and three misaligned views of the same values under the same scalars: fx_mt_adam's float4 arm and
    its scalar arm are one function of the element, so p, m and v carry the same bits after every step."""
    ns, p0, grads = _mt_values(MT_SIZES, 1)
    sts = {al: _MtState(MT_SIZES, [offs] * len(MT_SIZES), p0, dev) for al, offs in MT_ALIGN.items()}
    NB = _lib.FX_MT_BLOCKS
    sq = torch.empty(len(ns) * NB, device=dev)
    scal = B.new_scalars(dev, lr=MT_LR, max_norm=_mt_max_norm(case["regime"], grads))
    arms = set()
    for t in range(1, MT_STEPS + 1):
        for st in sts.values():
            st.set_grads(grads[t - 1])
        B.opt_begin_step(scal)
        B.mt_sqnorm(sts["aligned"].t[1], sq)
        B.clip_coef([sq], scal)
        for al, st in sts.items():
            B.mt_adam(st.t[0], st.t[1], st.t[2], st.t[3], scal)
            _sync(dev)
            st.check((case["id"], al, t))
            arms |= st.arms("adam")
        for al, st in sts.items():
            for r in (0, 2, 3):
                same_bits(torch.cat(st.host(r)), torch.cat(sts["aligned"].host(r)),
                          (case["id"], t, "%s of %s != aligned" % ("pgmv"[r], al)))
    assert (float(scal[_lib.SC_CLIP]) < 1.0) == (case["regime"] == "below")
    return arms


# =====================================================================================================================
# 2. fx_clip_coef / fx_sum_parts
# =====================================================================================================================
CLIP_LENS = [0, 1, 1023, 1025, 5000]
CLIP_CASES = (
    [dict(id="parts0-" + r, lens=[], regime=r) for r in ("off", "below")] +
    [dict(id="parts1-len%d-%s" % (n, r), lens=[n], mods=[m], regime=r)
     for n, m in ((0, 0), (1, 1), (1023, 2), (1025, 3), (5000, 1)) for r in ("off", "above", "below")] +
    [dict(id="parts16-" + r, lens=[CLIP_LENS[i % 5] for i in range(16)], mods=[i % 4 for i in range(16)], regime=r)
     for r in ("off", "above", "below")] +
    [dict(id="zeros-" + r, lens=[5, 1025], mods=[0, 1], regime=r, zeros=True) for r in ("off", "below")] +
    [dict(id="exact-1e8", lens=[1, 1023, 1025, 1024, 1024], mods=[1, 0, 2, 3, 0], regime="above", exact=True),
     dict(id="edge-total+1e-6", lens=[3, 2], mods=[1, 2], regime="edge")])
CLIP_REFUSALS = [dict(id="parts17", lens=[CLIP_LENS[1 + i % 4] for i in range(17)], mods=[i % 4 for i in range(17)])]


def _clip_parts(case, dev):
    g = torch.Generator().manual_seed(17 + len(case["lens"]))
    vals = [torch.rand(n, generator=g) * 3 for n in case["lens"]]
    if case.get("zeros"):
        vals = [torch.zeros(n) for n in case["lens"]]
    if case.get("exact"):
        # 1e8 and 4096 ones: every fp32 running sum stays at 1e8 (ulp 8); fp64 holds 100004096 exactly
        vals = [torch.full((n,), 1.0) for n in case["lens"]]
        vals[0][0] = 1e8
        assert sum(case["lens"][1:]) == 4096
    if case.get("regime") == "edge":
        vals = [torch.tensor([1.0, 4.0, 2.0]), torch.tensor([1.5, 0.5])]       # sum 9: total_norm exactly 3
    ar = Arena(Arena.need(*case["lens"]) + Arena.need(_lib.SC_WORDS, 1), dev)
    parts = [ar.vec(n, mod=m, fill=v) for n, m, v in zip(case["lens"], case["mods"], vals)] if vals else []
    return ar, parts, vals


def _clip_scal(B, ar, dev, max_norm):
    host = B.new_scalars("cpu", lr=1e-3, max_norm=max_norm)
    host[_lib.SC_LOSS] = 0.25
    scal = ar.vec(_lib.SC_WORDS, fill=host)
    for w in (_lib.SC_TOTAL_NORM, _lib.SC_CLIP):
        ar.free[ar.slots[-1][0] + w] = True            # the only two words of the block fx_clip_coef may change
    return scal


def run_clip(case, B, dev):
    what = case["id"]
    ar, parts, vals = _clip_parts(case, dev)
    sum64 = sum(float(v.double().sum()) for v in vals)
    total64 = math.sqrt(sum64)
    total32 = torch.tensor(total64, dtype=torch.float32)
    one_e6 = torch.tensor(1e-6, dtype=torch.float32)
    mx = {"off": 0.0, "above": 1e6 * max(total64, 1.0), "below": 0.37 * total64 if total64 > 0 else 2.0,
          "edge": float(total32 + one_e6)}[case["regime"]]
    scal = _clip_scal(B, ar, dev, mx)
    out = ar.vec(1, write=True)
    ar.seal()
    B.sum_parts(parts, out)
    B.clip_coef(parts, scal)
    _sync(dev)
    ar.check(what)
    got_sum, total, coef = float(out[0]), float(scal[_lib.SC_TOTAL_NORM]), float(scal[_lib.SC_CLIP])
    mx32 = float(scal[_lib.SC_MAX_NORM])
    # the sum: fp64 accumulation of fp32 terms (exact to 2^-53 per addition), one cast
    assert abs(got_sum - sum64) <= U * sum64, (what, "sum_parts", got_sum, sum64)
    # total_norm: that sum, one sqrt, one cast: relative 2^-23
    assert abs(total - total64) <= 2 * U * total64, (what, "total_norm", total, total64)
    coef64 = min(1.0, mx32 / (total64 + 1e-6)) if mx32 > 0 else 1.0
    # clip_coef: one add and one divide in fp32 on that total: relative 2^-22
    assert abs(coef - coef64) <= 4 * U * coef64, (what, "clip_coef", coef, coef64)
    if case["regime"] in ("off", "above", "edge") or sum64 == 0.0:
        assert coef == 1.0, (what, coef)
    else:
        assert coef < 1.0, (what, coef)
    if case.get("exact"):
        assert got_sum == 100004096.0, (what, got_sum)
        assert total == float(torch.tensor(math.sqrt(100004096.0), dtype=torch.float32)), (what, total)
    if case["regime"] == "edge":
        assert total == 3.0 and mx32 == float(total32 + one_e6)
    arms = {"clip.parts%d" % len(parts), "clip.max_norm_" + case["regime"]}
    arms |= {"clip.part.empty" for n in case["lens"] if n == 0}
    arms |= {"clip.part.stride" for n in case["lens"] if n > 1024}
    arms |= {"clip.part.misaligned" for p in parts if p.numel() and not _aligned(p)}
    if sum64 == 0.0 and mx32 > 0:
        arms.add("clip.zero_total")
    if case.get("exact"):
        arms.add("clip.fp64_needed")
    return arms


def run_clip_refusal(case, B, dev):
    ar, parts, _ = _clip_parts(case, dev)
    scal = _clip_scal(B, ar, dev, 1.0)
    out = ar.vec(1, write=True)
    ar.seal()
    assert len(parts) == _lib.FX_CLIP_MAX_PARTS + 1
    for call in (lambda: B.sum_parts(parts, out), lambda: B.clip_coef(parts, scal)):
        with pytest.raises(_lib.FxError):
            call()
    _sync(dev)
    ar.check(case["id"], untouched=True)
    return {"clip.refuse17"}


# =====================================================================================================================
# 3. fx_sigmoid_bce
# =====================================================================================================================
BCE_SATURATED = [s * x for x in (20.0, 40.0, 89.0, 104.0, 1e4) for s in (1.0, -1.0)]
BCE_SAT_PAIRS = [(x, t) for x in BCE_SATURATED for t in (0.0, 1.0)]
BCE_CASES = ([dict(id="B%d" % b, B=b) for b in (1, 2, 1023, 1024, 1025, 5000)] +
             [dict(id="sat%+g-y%d" % (x, t), B=1, x=x, t=t) for x, t in BCE_SAT_PAIRS])


def _bce_inputs(case):
    b = case["B"]
    if "x" in case:
        return torch.tensor([case["x"]]), torch.tensor([case["t"]])
    g = torch.Generator().manual_seed(30 + b)
    x = torch.randn(b, generator=g) * 3
    # (between about 15 and 17.4 the value of 1 - p hangs on the last bit of expf: not the kernel's business)
    x = torch.where((x.abs() > 14) & (x.abs() < 20), torch.full_like(x, 2.5), x)
    t = (torch.rand(b, generator=g) < 0.3).float()
    if b >= len(BCE_SAT_PAIRS):
        k = len(BCE_SAT_PAIRS)
        x[:k] = torch.tensor([p[0] for p in BCE_SAT_PAIRS])
        t[:k] = torch.tensor([p[1] for p in BCE_SAT_PAIRS])
    return x, t


def bce_ops64(p, t, scale=1.0):
    """The reference's two ops in float64 on given probabilities: F.binary_cross_entropy (mean; each log clamped at
    -100) and its backward (the 1e-12 floor) followed by the sigmoid backward.  -> (loss terms, dlogit)."""
    p = p.double().detach().requires_grad_(True)
    terms = torch.nn.functional.binary_cross_entropy(p, t.double(), reduction="none")
    terms.mean().backward()
    with torch.no_grad():
        return terms.detach(), p.grad * (p * (1 - p)) * scale


def run_bce(case, B, dev):
    what = case["id"]
    b = case["B"]
    x, t = _bce_inputs(case)
    ar = Arena(Arena.need(b, b, b, b, 1, b, 1, b), dev)
    xd, td = ar.vec(b, mod=1, fill=x), ar.vec(b, mod=2, fill=t)
    prob, dl, loss = ar.vec(b, mod=3, write=True), ar.vec(b, mod=1, write=True), ar.vec(1, write=True)
    prob2, loss2, dl2 = ar.vec(b, mod=2, write=True), ar.vec(1), ar.vec(b)      # the activation-only call
    ar.seal()
    B.sigmoid_bce(xd, td, prob=prob, loss=loss, dlogit=dl)
    B.sigmoid_bce(xd, None, prob=prob2)
    _sync(dev)
    ar.check(what)
    p = prob.cpu()
    same_bits(prob2, p, (what, "activation-only prob"))
    assert (p.double() - torch.sigmoid(x.double())).abs().max().item() <= 2e-7, (what, "prob")
    terms, d64 = bce_ops64(p, t)
    l64 = float(terms.mean())
    # relative 2e-6 for every B of the list.  The single saturated rows (this module's addition) can have a loss far
    # below 1: there the rounding of 1.f - p (at most U, and d log(1 - p) / dp is 1 at p ~ 0) is all that is left,
    # e.g. x = -20, y = 0: fp32 has 1 - 2e-9 == 1 and a loss of 0, float64 2e-9
    floor = U if "x" in case else 0.0
    assert abs(float(loss[0]) - l64) <= 2e-6 * abs(l64) + floor, (what, "loss", float(loss[0]), l64)
    d = dl.cpu()
    assert (d.double() - d64).abs().max().item() <= 1e-9 + 2e-6 * d64.abs().max().item(), (what, "dlogit")
    sat = (p == 0) | (p == 1)
    assert bool((d[sat] == 0).all()), (what, "dlogit of a saturated row")
    arms = {"bce.B<1024" if b < 1024 else ("bce.B=1024" if b == 1024 else "bce.B%1024"), "bce.act_only"}
    if "x" in case:
        assert bool(sat.all()) or abs(case["x"]) < 89, (what, float(p[0]))
        if bool(sat.all()):
            wrong = float(p[0]) != case["t"]
            assert float(loss[0]) == (100.0 if wrong else 0.0), (what, float(loss[0]))
            arms.add("bce.saturated.%s" % ("wrong" if wrong else "right"))
    elif b >= len(BCE_SAT_PAIRS):
        k = len(BCE_SAT_PAIRS)
        wrong = sat[:k] & (p[:k] != t[:k])
        assert int(wrong.sum()) >= 6 and bool((terms[:k][wrong] == 100.0).all()), what
        arms.add("bce.saturated.mixed")
    return arms


# =====================================================================================================================
# 4. fx_head_train
# =====================================================================================================================
HEAD_KS = [12, 256, 260, 516, 1028, 2048]
HEAD_MS = [1, 3, 5, 1021, 1030]
HEAD_SAT = [(25.0, 0.0), (25.0, 1.0), (-25.0, 0.0), (-30.0, 1.0)]        # (logit, label) of rows 0 .. 3 where M >= 5


def _head_cases():
    out = []
    for i, (K, M) in enumerate((K, M) for K in HEAD_KS for M in HEAD_MS):
        masks = [m for m in (-1, 0, 4, 256, K - 4) if m < K]
        out.append(dict(id="K%d-M%d" % (K, M), K=K, M=M, mask_from=masks[i % len(masks)], bias=i % 2 == 0,
                        add=(i // 2) % 2 == 0, scale=(1.0, 0.125)[(i // 3) % 2], dz=i % 7 != 3, db=i % 5 != 4))
    return out


HEAD_CASES = _head_cases()
HEAD_REFUSALS = [dict(id=k, kind=k) for k in ("K8", "K10", "K2052", "h_off1", "ldh", "mask2", "dz_off1")]


def head_nu(K):
    """(instantiation, float4 blocks of 256 columns a row really fills) of k_head_train."""
    nu = -(-K // 256)
    return (1 if nu <= 1 else 2 if nu <= 2 else 4 if nu <= 4 else 8), nu


def _head_values(case):
    K, M = case["K"], case["M"]
    g = torch.Generator().manual_seed(7 * K + M)
    h = torch.randn(M, K, generator=g)
    if case["mask_from"] >= 0:
        h[:, case["mask_from"]:] = torch.relu(h[:, case["mask_from"]:])
    W = torch.randn(1, K, generator=g) / K ** 0.5
    b = torch.randn(1, generator=g) * 0.5
    add = torch.randn(M, 1, generator=g) * 0.5
    y = (torch.rand(M, generator=g) > 0.6).float()
    w64 = W.double().view(-1)

    def z64():
        z = h.double() @ w64
        return z + (b.double() if case["bias"] else 0) + (add.double().view(-1) if case["add"] else 0)
    if M >= 5:
        # rows 0 .. 3: the logit moved to +-25 / -30 along w (the smallest change of the row that does it)
        for r, (target, label) in enumerate(HEAD_SAT):
            h[r] += ((target - z64()[r]) * w64 / (w64 @ w64)).float()
            y[r] = label
    z = z64()
    lo = z.abs() < 14
    assert bool((lo | (z.abs() >= 20)).all()) and (M < 5 or int((~lo).sum()) == 4), case["id"]
    return h, W, b, add, y


def _head_call(case, B, dev, vals, strided, flaw=None):
    """One fx_head_train call with every operand in an arena -> (arena, outputs, h, W, add)."""
    h, W, b, add, y = vals
    M, K = h.shape
    n_ws = B.head_train_workspace_floats(M, K)
    ar = Arena(Arena.need(M * (K + 8), M * (K + 13), 3 * M, K, 1, M, M, M, K, 1, 1, n_ws), dev)
    if flaw == "h_off1":
        hv = ar.mat(M, K, ld=K + 8, col=1, fill=h)
    elif flaw == "ldh":
        hv = ar.mat(M, K, ld=K + 6, col=0, fill=h)
    else:
        hv = ar.mat(M, K, ld=K + 8, col=4, fill=h) if strided else ar.mat(M, K, fill=h)
    Wv = ar.vec(K, fill=W).view(1, K)
    bv = ar.vec(1, fill=b) if case["bias"] else None
    av = None
    if case["add"]:
        av = (ar.mat(M, 3, fill=torch.cat([add + 1, add, add - 1], 1))[:, 1:2] if strided else ar.mat(M, 1, fill=add))
    yv = ar.vec(M, fill=y)
    o = dict(logit=ar.vec(M, mod=1, write=True), dlogit=ar.vec(M, mod=3, write=True), dz=None, db=None)
    if case["dz"]:
        if flaw == "dz_off1":
            o["dz"] = ar.mat(M, K, ld=K + 12, col=1, write=True)
        else:
            o["dz"] = ar.mat(M, K, ld=K + 12, col=4, write=True) if strided else ar.mat(M, K, write=True)
    o["dW"] = ar.vec(K, mod=1, write=True).view(1, K)
    if case["db"]:
        o["db"] = ar.vec(1, write=True)
    o["loss"] = ar.vec(1, write=True)
    ws = ar.vec(n_ws, write=True)
    ar.seal()
    mask_from = 2 if flaw == "mask2" else case["mask_from"]

    def call():
        B.head_train(hv, Wv, bv, av, yv, mask_from, case["scale"], o["logit"], o["dlogit"], o["dz"], o["dW"],
                     o["db"], o["loss"], ws)
    return ar, o, call, (hv, Wv, av)


def head_ops64(z, t, M, scale):
    """The reference's ops in float64 on logits z, with the saturation of the fp32 sigmoid (p exactly 1 from about
    17.4 up, exactly 0 below about -88.7) in place of float64's own: -> (loss terms, dlogit)."""
    p = torch.sigmoid(z.double())
    p32 = p.float()
    p = torch.where(p32 == 1, torch.ones_like(p), torch.where(p32 == 0, torch.zeros_like(p), p))
    assert z.numel() == M
    return bce_ops64(p, t, scale)


def run_head(case, B, dev):
    what = case["id"]
    K, M, scale, mask_from = case["K"], case["M"], case["scale"], case["mask_from"]
    vals = _head_values(case)
    h, W, b, add, y = vals
    ar, o, call, (hv, Wv, av) = _head_call(case, B, dev, vals, True)
    assert B.head_train_ok(hv, Wv, av)
    call()
    _sync(dev)
    ar.check(what)
    ar2, o2, call2, _ = _head_call(case, B, dev, vals, False)
    call2()
    _sync(dev)
    ar2.check((what, "contiguous"))
    for k in ("logit", "dlogit", "dz", "dW", "db", "loss"):
        if o[k] is not None:
            same_bits(o[k], o2[k], (what, "a stride changed the %s" % k))
    logit, d = o["logit"].cpu().double(), o["dlogit"].cpu().double()
    h64, w64 = h.double(), W.double().view(-1)
    # logit: a lane's chain of K / 64 fmaf's and the 6 levels of the wave butterfly (K / 64 + 8 covers both), then
    # one rounding each for the bias and the added term
    dot = h64 @ w64
    zb = dot + (b.double() if case["bias"] else 0)
    z64 = zb + (add.double().view(-1) if case["add"] else 0)
    bound = (K / 64.0 + 8) * U * (h64.abs() @ w64.abs()) + U * (zb.abs() * case["bias"] + z64.abs() * case["add"])
    assert bool(((logit - z64).abs() <= bound).all()), (what, "logit", float(((logit - z64).abs() / bound).max()))
    # dlogit from the kernel's own logit: p carries 3 roundings (expf, +, /) of a value <= 1, p - t one, the two
    # divisions / products by (1 - p) p cancel but for their 2 roundings, 1 / M and the root scale one each: 9 U
    # of |dlogit| <= scale / M.  Nowhere in (14, 20), where fp32 decides whether 1 - p is 0 (_head_values)
    terms, d64 = head_ops64(logit, y, M, scale)
    assert bool(((d - d64).abs() <= 9 * U * scale / M).all()), (what, "dlogit", float((d - d64).abs().max() * M))
    if M >= 5:
        # rows 0 and 1 (logit 25): p is exactly 1, the gradient exactly 0, the loss term of the wrong label 100
        assert float(d[0]) == 0.0 and float(d[1]) == 0.0 and float(terms[0]) == 100.0 and float(terms[1]) == 0.0, \
            (what, "saturated rows")
    if o["dz"] is not None:
        dz = o["dz"].cpu().double()
        want = d[:, None] * w64[None, :]
        if mask_from >= 0:
            want[:, mask_from:] = torch.where(h64[:, mask_from:] > 0, want[:, mask_from:], torch.zeros(()).double())
            assert bool((dz[:, mask_from:][h[:, mask_from:] <= 0] == 0).all()), (what, "dz mask")
        assert bool(((dz - want).abs() <= U * want.abs()).all()), (what, "dz")        # one product
    dW64 = (d[:, None] * h64).sum(0)
    tol = 4e-6 * max(1.0, float(dW64.abs().max())) * max(1.0, (M / 4096.0) ** 0.5)
    assert float((o["dW"].cpu().double().view(-1) - dW64).abs().max()) <= tol, (what, "dW")
    if o["db"] is not None:
        assert abs(float(o["db"][0]) - float(d.sum())) <= 1e-6, (what, "db")
    l64 = float(terms.mean())
    assert abs(float(o["loss"][0]) - l64) <= 2e-6 * max(1.0, l64), (what, "loss", float(o["loss"][0]), l64)
    inst, nu = head_nu(K)
    G = min(256, -(-M // 4))
    arms = {"head.NU%d.%s" % (inst, "full" if K == 256 * inst else "%dblocks%s" % (nu, ".partial" if K % 256 else "")),
            "head.mask_from.%s" % ("none" if mask_from < 0 else "0" if mask_from == 0 else "K-4" if mask_from == K - 4
                                   else str(mask_from)),
            "head.bias.%s" % case["bias"], "head.add.%s" % case["add"], "head.scale.%g" % scale,
            "head.strided.h", "head.G%s" % ("<256" if G < 256 else "256.idle_waves" if M < 1024 else
                                            "256.second_trip" if M > 1024 else "256")}
    arms |= {"head.strided.add"} if case["add"] else set()
    arms |= {"head.strided.dz"} if case["dz"] else {"head.dz.none"}
    arms |= {"head.saturated"} if M >= 5 else set()
    arms |= set() if case["db"] else {"head.db.none"}
    return arms


def run_head_refusal(case, B, dev):
    kind = case["kind"]
    K = {"K8": 8, "K10": 10, "K2052": 2052}.get(kind, 12)
    base = dict(id=kind, K=K, M=5, mask_from=0 if kind == "mask2" else -1, bias=True, add=True, scale=1.0, dz=True,
                db=True)
    g = torch.Generator().manual_seed(K)
    vals = (torch.randn(5, K, generator=g), torch.randn(1, K, generator=g), torch.randn(1, generator=g),
            torch.randn(5, 1, generator=g), torch.ones(5))
    ar, o, call, (hv, Wv, av) = _head_call(base, B, dev, vals, True, flaw=kind)
    with pytest.raises(_lib.FxError):
        call()
    _sync(dev)
    ar.check(kind, untouched=True)
    if kind in ("K8", "K10", "K2052", "h_off1", "ldh"):
        assert not B.head_train_ok(hv, Wv, av), kind
    return {"head.refuse." + kind}


# =====================================================================================================================
# 5. fx_colsum
# =====================================================================================================================
COLSUM_MS = [1, 15, 63, 64, 65, 257]
COLSUM_NS = [1, 3, 4, 8, 252, 256, 260]
COLSUM_LAYOUTS = ["contiguous", "slice4", "slice1", "ld+1"]
COLSUM_CASES = ([dict(id="M%d-N%d-%s" % (M, N, lay), M=M, N=N, layout=lay)
                 for M in COLSUM_MS for N in COLSUM_NS for lay in COLSUM_LAYOUTS] +
                [dict(id="M65-N8-ws_off1", M=65, N=8, layout="ws_off1")])


def colsum_chain(M):
    """The longest addition chain of an element through fx_colsum: k_colsum_stage1* gives a thread every 4th row of
    a chunk of ceil(M / 64) rows and joins the four as (a0 + a1) + (a2 + a3); fx_rowsum<float, FX_ROWS_SLICES> gives
    a wave every 4th of the 64 chunk rows (16 additions) and joins the four as (s0 + s1) + (s2 + s3)."""
    rpc = -(-max(M, 1) // _lib.FX_COLSUM_CHUNKS)
    return -(-rpc // 4) + 2 + 16 + 2


_colsum_contiguous = {}


def run_colsum(case, B, dev):
    what = case["id"]
    M, N, lay = case["M"], case["N"], case["layout"]
    key = (str(dev), B.__name__, M, N)
    if lay != "contiguous" and key not in _colsum_contiguous:
        run_colsum(dict(case, id="M%d-N%d-contiguous" % (M, N), layout="contiguous"), B, dev)
    X = torch.randn(M, N, generator=torch.Generator().manual_seed(100 * M + N))
    n_ws = _lib.FX_COLSUM_CHUNKS * N
    ar = Arena(Arena.need(M * (N + 9), N, n_ws + 1), dev)
    if lay == "slice4":
        Xv = ar.mat(M, N, ld=N + 8, col=4, fill=X)
    elif lay == "slice1":
        Xv = ar.mat(M, N, ld=N + 8, col=1, fill=X)
    elif lay == "ld+1":
        Xv = ar.mat(M, N, ld=N + 1, fill=X)
    else:
        Xv = ar.mat(M, N, fill=X)
    out = ar.vec(N, mod=3, write=True)
    ws = ar.vec(n_ws, mod=1 if lay == "ws_off1" else 0, write=True)
    ar.seal()
    B.colsum(Xv, out, ws)
    _sync(dev)
    ar.check(what)
    got = out.cpu()
    # per column: c U sum_m |X[m, n]| with c the chain through both stages
    c = colsum_chain(M)
    bound = c * U * X.double().abs().sum(0)
    assert bool(((got.double() - X.double().sum(0)).abs() <= bound).all()), (what, "c = %d" % c)
    # the float4 arm and the scalar arm add the same rows in the same order
    if lay == "contiguous":
        _colsum_contiguous[key] = got
    else:
        same_bits(got, _colsum_contiguous[key], (what, "!= the contiguous layout"))
    vec = N % 4 == 0 and Xv.stride(0) % 4 == 0 and _aligned(Xv) and _aligned(ws)
    arms = {"colsum.vec" + (".strided" if Xv.stride(0) != N else "") if vec else
            "colsum.scalar." + ("N" if N % 4 else "ld" if Xv.stride(0) % 4 else "ws" if not _aligned(ws) else "X")}
    arms.add("colsum.empty_chunks" if M < _lib.FX_COLSUM_CHUNKS else
             "colsum.chunks.%s" % ("full" if M == 64 else "ragged"))
    return arms


# =====================================================================================================================
# 6. fx_mask_mul / fx_cross_bwd_prep
# =====================================================================================================================
GLUE_SHAPES = [(1, 1), (7, 3), (300, 37)]
MASK_CASES = [dict(id="%dx%d-dy%d-y%d" % (r, c, sd, sy), rows=r, cols=c, dy_strided=sd, y_strided=sy)
              for r, c in GLUE_SHAPES for sd in (0, 1) for sy in (0, 1)]
PREP_CASES = [dict(id="%dx%d-dxn%d-init%d-add%d" % (r, c, sd, i, a), rows=r, cols=c, dxn_strided=sd, init=i, add_dxn=a)
              for r, c in GLUE_SHAPES for sd in (0, 1) for i in (0, 1) for a in (0, 1)]


def _glue_mat(ar, X, strided, col):
    r, c = X.shape
    return ar.mat(r, c, ld=c + 9, col=col, fill=X) if strided else ar.mat(r, c, fill=X)


def run_mask_mul(case, B, dev):
    what = case["id"]
    r, c = case["rows"], case["cols"]
    g = torch.Generator().manual_seed(r + c)
    dy, y = torch.randn(r, c, generator=g), torch.randn(r, c, generator=g)
    y[::2, ::3] = 0.0                                   # y == 0 masks as well (y > 0 keeps)
    ar = Arena(Arena.need(r * (c + 9), r * (c + 9), r * c), dev)
    dyv, yv = _glue_mat(ar, dy, case["dy_strided"], 5), _glue_mat(ar, y, case["y_strided"], 3)
    out = ar.mat(r, c, write=True)
    ar.seal()
    B.mask_mul(dyv, yv, out)
    _sync(dev)
    ar.check(what)
    same_bits(out, torch.where(y > 0, dy, torch.zeros(())), (what, "mask_mul is a selection: exact"))
    return {"mask_mul.dy%d.y%d" % (case["dy_strided"], case["y_strided"])}


def run_cross_prep(case, B, dev):
    what = case["id"]
    r, c = case["rows"], case["cols"]
    g = torch.Generator().manual_seed(3 * r + c)
    dxn, x0, z, dx0 = (torch.randn(r, c, generator=g) for _ in range(4))
    ar = Arena(Arena.need(r * (c + 9), r * c, r * c, r * c, r * c), dev)
    dv = _glue_mat(ar, dxn, case["dxn_strided"], 5)
    xv, zv = ar.mat(r, c, fill=x0), ar.mat(r, c, fill=z)
    tv = ar.mat(r, c, write=True)
    ov = ar.mat(r, c, write=True, fill=None if case["init"] else dx0)      # init: dx0 starts as NaN and is overwritten
    ar.seal()
    B.cross_bwd_prep(dv, xv, zv, tv, ov, init=bool(case["init"]), add_dxn=bool(case["add_dxn"]))
    _sync(dev)
    ar.check(what)
    d64 = dxn.double()
    t64 = d64 * x0.double()
    assert bool(((tv.cpu().double() - t64).abs() <= U * t64.abs()).all()), (what, "t: one product")
    # dx0: one rounding per operation — the product d z, + d (add_dxn), + dx0 (not init) — each at most U times the
    # exact value of that operation's result (1 + 3 U: the operands of the later ones carry the earlier roundings)
    prod = d64 * z.double()
    term = prod + (d64 if case["add_dxn"] else 0)
    want = term if case["init"] else dx0.double() + term
    bound = U * (prod.abs() + (term.abs() if case["add_dxn"] else 0) + (0 if case["init"] else want.abs()))
    assert bool(((ov.cpu().double() - want).abs() <= bound * (1 + 3 * U)).all()), (what, "dx0")
    return {"cross_prep.init%d.add%d" % (case["init"], case["add_dxn"]), "cross_prep.dxn%d" % case["dxn_strided"]}


# =====================================================================================================================
GROUPS = {
    "mt": (MT_CASES, run_mt), "mt_agree": (MT_AGREE_CASES, run_mt_agree),
    "clip": (CLIP_CASES, run_clip), "clip_refusal": (CLIP_REFUSALS, run_clip_refusal),
    "bce": (BCE_CASES, run_bce),
    "head": (HEAD_CASES, run_head), "head_refusal": (HEAD_REFUSALS, run_head_refusal),
    "colsum": (COLSUM_CASES, run_colsum),
    "mask_mul": (MASK_CASES, run_mask_mul), "cross_prep": (PREP_CASES, run_cross_prep),
}
COUNTS = {"mt": 34, "mt_agree": 3, "clip": 24, "clip_refusal": 1, "bce": 26, "head": 30, "head_refusal": 7,
          "colsum": 169, "mask_mul": 12, "cross_prep": 24}

# every arm the issue names, by the names the run_* functions report
ARMS = {
    "mt": {"sqnorm.vec", "sqnorm.scalar", "sqnorm.vec.wrap", "sqnorm.vec.tail", "sqnorm.scalar.wrap", "adam.vec",
           "adam.scalar", "adam.vec.wrap", "adam.vec.tail", "adam.scalar.wrap", "sqnorm.vec+adam.scalar", "sgd",
           "sgd.wrap", "mt.empty", "mt.chunks1", "mt.chunks2", "mt.chunks3"},
    "mt_agree": {"adam.vec", "adam.scalar", "adam.vec.wrap", "adam.scalar.wrap"},
    "clip": {"clip.parts0", "clip.parts1", "clip.parts16", "clip.part.empty", "clip.part.stride",
             "clip.part.misaligned", "clip.max_norm_off", "clip.max_norm_above", "clip.max_norm_below",
             "clip.max_norm_edge", "clip.zero_total", "clip.fp64_needed"},
    "clip_refusal": {"clip.refuse17"},
    "bce": {"bce.B<1024", "bce.B=1024", "bce.B%1024", "bce.act_only", "bce.saturated.wrong", "bce.saturated.right",
            "bce.saturated.mixed"},
    "head": {"head.NU1.1blocks.partial", "head.NU1.full", "head.NU2.2blocks.partial", "head.NU4.3blocks.partial",
             "head.NU8.5blocks.partial", "head.NU8.full", "head.G<256", "head.G256.idle_waves",
             "head.G256.second_trip", "head.mask_from.none", "head.mask_from.0", "head.mask_from.4",
             "head.mask_from.256", "head.mask_from.K-4", "head.bias.True", "head.bias.False", "head.add.True",
             "head.add.False", "head.scale.1", "head.scale.0.125", "head.strided.h", "head.strided.dz",
             "head.strided.add", "head.dz.none", "head.db.none", "head.saturated"},
    "head_refusal": {"head.refuse." + k for k in ("K8", "K10", "K2052", "h_off1", "ldh", "mask2", "dz_off1")},
    "colsum": {"colsum.vec", "colsum.vec.strided", "colsum.scalar.N", "colsum.scalar.X", "colsum.scalar.ld",
               "colsum.scalar.ws", "colsum.empty_chunks", "colsum.chunks.full", "colsum.chunks.ragged"},
    "mask_mul": {"mask_mul.dy%d.y%d" % (a, b) for a in (0, 1) for b in (0, 1)},
    "cross_prep": {"cross_prep.init%d.add%d" % (a, b) for a in (0, 1) for b in (0, 1)} |
                  {"cross_prep.dxn0", "cross_prep.dxn1"},
}


def ids(group):
    return [c["id"] for c in GROUPS[group][0]]


def run(group, case_id, B, dev):
    cases, fn = GROUPS[group]
    (case,) = [c for c in cases if c["id"] == case_id]
    return fn(case, B, dev)
