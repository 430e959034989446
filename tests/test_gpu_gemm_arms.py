"""Every arm of the dense GEMM dispatcher (fuxictr_amd/csrc/fx_gemm.hip) against float64, with the arm asserted.

fx_gemm_f32 chooses among the skinny kernels, the split-bf16 ("x6") kernels, the pipelined fp32-MFMA kernel on
three tiles (16-byte epilogue on or off) and the unpipelined one; fx_gemm_f32_batch tries five one-grid strategies
before it launches problem by problem.  Alignment, tile counts, split_k caps and FX_* switches (read once per
process) decide — and ops.gemm_last_strategy() says what was decided.  Each case below is the smallest shape the
dispatcher code routes to its arm; the child process (one per environment setting, one at a time) runs the cases
of its setting on NaN-filled outputs, asserts the strategy record and writes outputs and records to an .npz; the
parent re-creates the fp32 inputs from the case's seed and holds every output element, every fused row sum and
every epilogue operand to the float64 expression:

    no K split              2e-6 x max(|A| @ |B|)      (test_gemm_all_layouts)
    K-split weight gradient 3e-6 x the same bound      (test_gemm_dw_dx_pair_is_bit_identical_to_the_two_gemms)
    split-bf16 arms         1e-6 x the same bound      (test_gpu_gemm_x6.py)
    fused row sums          1e-5 x max row sum of |op(A)| (1e-6 on the split-bf16 arms, as in test_gpu_gemm_x6.py)
    head backward           1e-5 x bound for dW, 1e-6 x max|ref| for dX (test_head_backward_in_one_pass_...)

An epilogue operand adds the fp32 rounding of its own operation, one ulp (u = 2^-23) of the value it produces:
z = acc + bias within tol + u|z|, t = act(z) * mul within |mul| tol_z + u|t|, out = t + add within tol_t + u|out|.
Columns of an output buffer outside the product must still be NaN; a batch is run twice and must repeat its bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = {"default": {}, "x6off": {"FX_GEMM_BF16X6": "0"},
            "x6off_multioff": {"FX_GEMM_BF16X6": "0", "FX_GEMM_MULTI": "0"}, "pairoff": {"FX_GEMM_PAIR": "0"}}
# switches of the dispatcher that must not leak in from the caller's environment
SWITCHES = ("FX_GEMM_BF16X6", "FX_GEMM_MULTI", "FX_GEMM_PAIR", "FX_GEMM_PIPE", "FX_GEMM_TILE", "FX_GEMM_TR",
            "FX_GEMM_FWDPAIR", "FX_GEMM_EDGE_PLAIN", "FX_HEAD_FUSE", "FX_MULTI_CFG", "FX_X6_PLAN", "FX_SPLITK_V4")
U = 2.0 ** -23


class P(object):
    """One product C[M, N] = epilogue(op(A) op(B)).  epi: subset of bias relu zout mul mask add rowsum.
    cap: the split_k handed over (a workspace comes with cap > 1).  *_view = (col0, pad): the operand is the
    column slice [col0, col0 + width) of a buffer `pad` columns wider still (odd col0: base 4 bytes off).
    cbuf = (name, width, col0): the output is a column slice of a buffer shared inside the case.
    a_from = i: op(A)'s storage is problem i's; mask_from_b = i: the mask is problem i's B."""

    def __init__(self, M, N, K, ta=False, tb=False, epi=(), cap=1, a_view=(0, 0), b_view=(0, 0), c_view=(0, 0),
                 cbuf=None, a_from=None, mask_from_b=None):
        self.M, self.N, self.K, self.ta, self.tb = M, N, K, ta, tb
        self.epi, self.cap = tuple(epi), cap
        self.a_view, self.b_view, self.c_view, self.cbuf = a_view, b_view, c_view, cbuf
        self.a_from, self.mask_from_b = a_from, mask_from_b


def L(arm, bm, bn, sk, tr, **kw):
    return dict(arm=arm, bm=bm, bn=bn, split_k=sk, tr=bool(tr), **kw)


class Case(object):
    def __init__(self, name, probs, expect, batch=None):
        self.name, self.probs, self.expect = name, probs, expect       # expect: {setting: (strategy, [L...])}
        self.batch = len(probs) > 1 if batch is None else batch
        self.seed = sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


# ---- the split rules of fx_gemm.hip, for the single launches of a batch -------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def splitk_rule_x6(K, cap):
    return 1 if cap <= 1 else max(1, min((K + 512) // 1024, cap))


def splitk_rule64(M, N, K, cap):
    if cap <= 1:
        return 1
    tiles = _cdiv(M, 64) * _cdiv(N, 64)
    s = 1
    if tiles >= 768:
        s = 1
    elif tiles <= 4:
        s = min(_cdiv(512, tiles), 256)
    else:
        want = 1024.0 / tiles
        while s * 1.5 < want:
            s *= 2
        s = min(s, 16)
    return max(1, min(s, K // 256, cap))


def batch_wants_x6(p):
    if not (p.M >= 128 and p.N >= 128 and p.K >= 64) or ("rowsum" in p.epi and not p.ta):
        return False
    return _cdiv(p.M, 128) * _cdiv(p.N, 128) * splitk_rule_x6(p.K, p.cap) >= 96


def prepared_split(K, sk):
    """fx_gemm_prepare: slabs start on a k-tile (32) boundary."""
    kc = max(32, _cdiv(_cdiv(K, sk), 32) * 32)
    return _cdiv(max(K, 1), kc)


def single_split(p):
    """The K slabs of problem p when fx_gemm_f32_batch launches it on its own (x6 enabled)."""
    return prepared_split(p.K, splitk_rule_x6(p.K, p.cap) if batch_wants_x6(p) else splitk_rule64(p.M, p.N, p.K, p.cap))


# ---- the cases ----------------------------------------------------------------------------------------------------
def dw_dx(M, N, K, cap, epi_dx=("mask", "add")):
    """The gradient pair of a layer K -> N on M rows: dW[N, K] = dz^T x (K slabs, fused bias gradient) and
    dX[M, K] = dz W, sharing dz."""
    return [P(N, K, M, ta=True, epi=("rowsum",), cap=cap), P(M, K, N, epi=epi_dx, a_from=0)]


def _cases():
    cs = []
    pipe64 = ("PIPE", [L("PIPE", 64, 64, 1, True)])
    # split bf16: exactly 96 workgroups, all four layouts; one tile column short of it: refused
    for ta, tb in ((False, True), (False, False), (True, False), (True, True)):
        cs.append(Case("x6_96wg_%d%d" % (ta, tb), [P(1536, 1024, 64, ta, tb)],
                       {"default": ("X6", [L("X6", 128, 128, 1, True)]), "x6off": pipe64}))
    cs.append(Case("x6_84wg_refused", [P(1536, 896, 64, tb=True, epi=("bias", "relu"))], {"default": pipe64}))
    # pipelined fp32 MFMA: 64x64, 128x64 (N <= 64 only), 128x128 (>= 1024 workgroups of it) — 16-byte epilogue on
    cs.append(Case("pipe64_tr", [P(256, 256, 128, tb=True, epi=("bias", "zout", "mul", "add"))], {"default": pipe64}))
    for M, N, K in ((1000, 64, 64), (130, 48, 72)):
        cs.append(Case("pipe12864_tr_%d" % M, [P(M, N, K, tb=True, epi=("bias", "relu"))],
                       {"default": ("PIPE", [L("PIPE", 128, 64, 1, True)])}))
    cs.append(Case("pipe128_tr", [P(16384, 1024, 64, tb=True, epi=("bias", "relu"))],
                   {"x6off": ("PIPE", [L("PIPE", 128, 128, 1, True)])}))
    cs.append(Case("pipe128_one_wg_short", [P(11904, 1408, 64, tb=True)], {"x6off": pipe64}))      # 93 x 11 = 1023
    # ... and off: N % 4 == 2, or an output whose base is 4 bytes off
    cs.append(Case("pipe64_notr_n1030", [P(512, 1030, 64, tb=True, epi=("bias", "relu", "mask"))],
                   {"default": ("PIPE", [L("PIPE", 64, 64, 1, False)])}))
    cs.append(Case("pipe64_notr_cbase", [P(256, 256, 128, tb=True, epi=("bias", "zout", "mul", "add"), c_view=(1, 3))],
                   {"default": ("PIPE", [L("PIPE", 64, 64, 1, False)])}))
    cs.append(Case("pipe12864_notr_n62", [P(300, 62, 64, tb=True, epi=("bias", "relu"))],
                   {"default": ("PIPE", [L("PIPE", 128, 64, 1, False)])}))
    cs.append(Case("pipe128_notr_n1030", [P(16384, 1030, 64, tb=True, epi=("bias",))],
                   {"default": ("PIPE", [L("PIPE", 128, 128, 1, False)])}))
    # a K-split single launch on the pipelined kernel, fused row sums (2 slabs of 96 + 40)
    cs.append(Case("pipe64_split", [P(256, 136, 136, ta=True, epi=("rowsum",), cap=2)],
                   {"default": ("PIPE", [L("PIPE", 64, 64, 2, True)])}))
    # the unpipelined kernel: an operand that cannot be read as 16-byte vectors
    plain = lambda av, bv: ("PLAIN", [L("PLAIN", 64, 64, 1, False, av=av, bv=bv)])
    cs.append(Case("plain_ktail", [P(200, 136, 70, tb=True, epi=("bias", "relu"))], {"default": plain(False, False)}))
    cs.append(Case("plain_av", [P(200, 136, 70, ta=True, tb=True)], {"default": plain(True, False)}))
    cs.append(Case("plain_bv", [P(200, 136, 70, epi=("mask", "add"))], {"default": plain(False, True)}))
    cs.append(Case("plain_ragged_mn", [P(201, 137, 72, ta=True)], {"default": plain(False, False)}))
    cs.append(Case("plain_a_slice", [P(200, 136, 72, tb=True, a_view=(1, 3))], {"default": plain(False, True)}))
    cs.append(Case("plain_b_slice", [P(200, 136, 72, tb=True, b_view=(3, 1), epi=("bias", "zout", "mul", "add"))],
                   {"default": plain(True, False)}))
    cs.append(Case("plain_ab_slices_lda_odd", [P(200, 136, 72, a_view=(2, 3), b_view=(1, 1))],
                   {"default": plain(False, False)}))
    # skinny kernels and the fused head backward
    cs.append(Case("skinny_k3", [P(300, 64, 3, tb=True, epi=("bias",))], {"default": ("SKINNY", [L("SKINNY", 0, 0, 1, False)])}))
    cs.append(Case("head_bwd", [P(1, 64, 1000, ta=True, epi=("rowsum",), cap=16),
                                P(1000, 64, 1, a_from=0, epi=("mask",), mask_from_b=0)],
                   {"default": ("HEAD_BWD", None)}))
    # one grid of fp32-MFMA tiles IN THE DEFAULT PROCESS: the split-bf16 grid refuses a list with an N = 96 problem
    # (dW / dX of 4096-row layers 1024 -> 1024 and 96 -> 1024: 256 + 256 + 32 + 32 workgroups, both tiles, 4 slabs)
    m4 = [P(1024, 1024, 4096, ta=True, epi=("rowsum",), cap=8), P(4096, 1024, 1024, epi=("mask", "add")),
          P(1024, 96, 4096, ta=True, epi=("rowsum",), cap=8), P(4096, 96, 1024)]
    m4_multi = ("MULTI_F32", [L("MULTI_F32", 128, 128, 4, True), L("MULTI_F32", 128, 128, 1, True),
                              L("MULTI_F32", 128, 64, 4, True), L("MULTI_F32", 128, 64, 1, True)])
    cs.append(Case("multi_n96", m4, {"default": m4_multi, "x6off": m4_multi,
                                     "pairoff": ("SINGLES", [L("X6", 128, 128, "rule", True), L("X6", 128, 128, "rule", True),
                                                             L("PIPE", 64, 64, "rule", True), L("PIPE", 64, 64, "rule", True)])}))
    # ... or one whose only obstacle is a row sum over a k-contiguous op(A) (256 + 256 workgroups)
    rs = [P(4096, 1024, 128, tb=True, epi=("rowsum", "bias")), P(2048, 2048, 128, ta=True, cap=2)]
    rs_multi = ("MULTI_F32", [L("MULTI_F32", 128, 128, 1, True), L("MULTI_F32", 128, 128, 1, True)])
    cs.append(Case("multi_rowsum_kc", rs, {"default": rs_multi, "x6off": rs_multi,
                                           "pairoff": ("SINGLES", [L("PIPE", 64, 64, "rule", True), L("X6", 128, 128, "rule", True)])}))
    # the floor of the fp32 grid: 480 + 32 = 512 workgroups of 128x128 stay, 497 + 14 = 511 go to the 64x64 pair
    cs.append(Case("multi_floor_512", dw_dx(256, 3840, 2048, 2),
                   {"x6off": ("MULTI_F32", [L("MULTI_F32", 128, 128, 1, True), L("MULTI_F32", 128, 128, 1, True)])}))
    pair = lambda sk: ("PAIR_BWD", [L("PAIR_BWD", 64, 64, sk, True), L("PAIR_BWD", 64, 64, 1, True)])
    cs.append(Case("multi_floor_511", dw_dx(256, 9088, 896, 2), {"x6off": pair(1)}))
    # the split-bf16 grid itself (64 + 32 workgroups before the planner's slabs)
    cs.append(Case("multi_x6", dw_dx(512, 1024, 1024, 4),
                   {"default": ("MULTI_X6", [L("MULTI_X6", 128, 128, None, True), L("MULTI_X6", 128, 128, 1, True)])}))
    # the 64x64 backward pair
    cs.append(Case("pair_bwd_2048", dw_dx(2048, 512, 128, 8),
                   {"x6off_multioff": pair(8),
                    "pairoff": ("SINGLES", [L("PIPE", 64, 64, "rule", True), L("PIPE", 64, 64, "rule", True)])}))
    cs.append(Case("pair_bwd_ragged", dw_dx(1000, 256, 136, 4), {"x6off_multioff": pair(3)}))
    # the 64x64 forward pair: CrossNet epilogue and bias + ReLU into one strided buffer, heavier problem second / first
    cross = P(1000, 624, 624, tb=True, epi=("bias", "zout", "mul", "add"), cbuf=("out", 1648, 0))
    deep = P(1000, 1024, 624, tb=True, epi=("bias", "relu"), cbuf=("out", 1648, 624))
    fwd = ("PAIR_FWD", [L("PAIR_FWD", 64, 64, 1, True), L("PAIR_FWD", 64, 64, 1, True)])
    singles = ("SINGLES", [L("PIPE", 64, 64, "rule", True), L("PIPE", 64, 64, "rule", True)])
    cs.append(Case("pair_fwd_swap", [cross, deep], {"x6off": fwd + (True,), "pairoff": singles}))
    cs.append(Case("pair_fwd_noswap", [deep, cross], {"x6off": fwd + (False,), "pairoff": singles}))
    return cs


CASES = _cases()
BY_NAME = dict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)


def make_inputs(case):
    """The fp32 inputs of a case on the host, from its seed alone (the child and the parent call this)."""
    g = torch.Generator().manual_seed(case.seed)
    data = []
    for p in case.probs:
        d = {}

        def stored(rows, cols, view):
            buf = torch.randn(rows, view[0] + cols + view[1], generator=g)
            return buf, buf[:, view[0]:view[0] + cols]
        if p.a_from is None:
            d["A_buf"], d["A"] = stored(p.K if p.ta else p.M, p.M if p.ta else p.K, p.a_view)
        else:
            d["A_buf"], d["A"] = data[p.a_from]["A_buf"], data[p.a_from]["A"]
        d["B_buf"], d["B"] = stored(p.N if p.tb else p.K, p.K if p.tb else p.N, p.b_view)
        if "bias" in p.epi:
            d["bias"] = torch.randn(p.N, generator=g)
        for k in ("mul", "mask", "add"):
            if k in p.epi:
                d[k] = torch.randn(p.M, p.N, generator=g)
        if p.mask_from_b is not None:
            d["mask"] = data[p.mask_from_b]["B"]
        data.append(d)
    return data


# ---- the child: run the cases of one setting on the GPU -----------------------------------------------------------
def _child_main(setting, out_path):
    sys.path.insert(0, ROOT)
    from fuxictr_amd import ops
    dev = torch.device("cuda:0")
    out, wrong = {}, []
    for case in CASES:
        if setting not in case.expect:
            continue
        data = make_inputs(case)
        on_dev = {}

        def dv(t):        # (a view moves with its whole buffer: strides and base offsets are what is tested)
            if t is None:
                return None
            key = t.untyped_storage().data_ptr()
            if key not in on_dev:
                base = torch.empty(t.untyped_storage().nbytes() // 4, dtype=torch.float32)
                base.set_(t.untyped_storage())
                on_dev[key] = base.to(dev)
            return on_dev[key].as_strided(t.size(), t.stride(), t.storage_offset())
        runs = []
        for rep in range(2 if case.batch else 1):
            bufs, probs, outs = {}, [], []
            for i, (p, d) in enumerate(zip(case.probs, data)):
                if p.cbuf:
                    name, width, col0 = p.cbuf
                    if name not in bufs:
                        bufs[name] = torch.full((p.M, width), float("nan"), device=dev)
                    cb, C = bufs[name], bufs[name][:, col0:col0 + p.N]
                    key = "cbuf_" + name
                else:
                    cb = torch.full((p.M, p.c_view[0] + p.N + p.c_view[1]), float("nan"), device=dev)
                    C = cb[:, p.c_view[0]:p.c_view[0] + p.N]
                    key = "%d/C" % i
                o = {key: cb}
                kw = dict(transa=p.ta, transb=p.tb, bias=dv(d.get("bias")), act=1 if "relu" in p.epi else 0,
                          mul=dv(d.get("mul")), mask=dv(d.get("mask")), add=dv(d.get("add")), split_k=p.cap)
                if "zout" in p.epi:
                    kw["zout"] = o["%d/zout" % i] = torch.full((p.M, p.N), float("nan"), device=dev)
                if "rowsum" in p.epi:
                    kw["rowsum"] = o["%d/rowsum" % i] = torch.full((p.M,), float("nan"), device=dev)
                if p.cap > 1:
                    kw["workspace"] = torch.full((ops.gemm_workspace_floats(p.M, p.N, p.cap),), float("nan"), device=dev)
                probs.append((dv(d["A"]), dv(d["B"]), C, kw))
                outs.append(o)
            if case.batch:
                ops.gemm_batch([ops.gemm_problem(A, B, C, **kw) for A, B, C, kw in probs])
            else:
                A, B, C, kw = probs[0]
                ops.gemm(A, B, C, **kw)
            rec = ops.gemm_last_strategy()
            torch.cuda.synchronize()
            runs.append(dict((k, v.cpu().numpy()) for o in outs for k, v in o.items()))
        if len(runs) == 2:
            for k in runs[0]:
                if not np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)):
                    wrong.append("%s: %s differs between two runs" % (case.name, k))
        for k, v in runs[0].items():
            out["%s/%s" % (case.name, k)] = v
        out[case.name + "/rec"] = np.array([ops.GEMM_STRATEGIES.index(rec.strategy), rec.n_problems, int(rec.swapped)] +
                                           [x for l in rec.launches for x in
                                            (ops.GEMM_STRATEGIES.index(l["arm"]), l["bm"], l["bn"], l["split_k"],
                                             int(l["tr"]), int(l["av"]), int(l["bv"]))], dtype=np.int64)
        why = check_record(case, setting, out[case.name + "/rec"])
        if why:
            wrong.append("%s [%s]: %s; the record: %r" % (case.name, setting, why, rec))
    np.savez(out_path, **out)
    assert not wrong, "\n".join(wrong)


def decode_record(arr):
    from fuxictr_amd import ops
    names = ops.GEMM_STRATEGIES
    launches = [dict(arm=names[r[0]], bm=int(r[1]), bn=int(r[2]), split_k=int(r[3]), tr=bool(r[4]), av=bool(r[5]),
                     bv=bool(r[6])) for r in np.asarray(arr[3:]).reshape(-1, 7)]
    return names[arr[0]], int(arr[1]), bool(arr[2]), launches


def expected_launches(case, setting):
    """[(arm, split_k or None)] per problem: the arm whose tolerance applies."""
    exp = case.expect[setting]
    if exp[1] is None:
        return [(exp[0], None)] * len(case.probs)
    return [(l["arm"], single_split(p) if l["split_k"] == "rule" else l["split_k"]) for l, p in zip(exp[1], case.probs)]


def check_record(case, setting, arr):
    """-> None, or what differs between the strategy record and what the case expects."""
    strategy, n_problems, swapped, launches = decode_record(arr)
    exp = case.expect[setting]
    if strategy != exp[0]:
        return "strategy %s, expected %s" % (strategy, exp[0])
    if n_problems != len(case.probs):
        return "%d problems recorded" % n_problems
    if len(exp) > 2 and swapped != exp[2]:
        return "swapped = %s" % swapped
    if exp[1] is None:
        return None
    if len(launches) != len(exp[1]):
        return "%d launches recorded, expected %d" % (len(launches), len(exp[1]))
    for i, (got, want, p) in enumerate(zip(launches, exp[1], case.probs)):
        want = dict(want)
        if want["split_k"] == "rule":
            want["split_k"] = single_split(p)
        elif want["split_k"] is None:                       # the split-bf16 planner's choice: within the cap
            if not 1 <= got["split_k"] <= p.cap:
                return "problem %d: %d slabs, cap %d" % (i, got["split_k"], p.cap)
            want["split_k"] = got["split_k"]
        for k, v in want.items():
            if got[k] != v:
                return "problem %d: %s = %r, expected %r" % (i, k, got[k], v)
    return None


# ---- the parent ---------------------------------------------------------------------------------------------------
_results, _refs = {}, {}


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("gemm_arms")


def results(setting, child_dir):
    if setting not in _results:
        # a child that died of a signal, hung or reported a device fault: no further child is started on that GPU
        for s, (rc, err, _) in _results.items():
            assert rc in (0, 1) and "illegal memory access" not in err, "the %s child faulted: %s" % (s, err)
        out = str(child_dir / (setting + ".npz"))
        env = dict((k, v) for k, v in os.environ.items() if k not in SWITCHES)
        env.update(SETTINGS[setting])
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), setting, out], env=env,
                               capture_output=True, text=True, timeout=600)
            rc, err = p.returncode, p.stderr[-4000:]
        except subprocess.TimeoutExpired:
            rc, err = 124, "the %s child hung" % setting
        _results[setting] = (rc, err, np.load(out) if rc in (0, 1) and os.path.exists(out) else None)
    return _results[setting]


def reference(case):
    """float64 of every output of the case, with the quantities its bounds are made of (computed once)."""
    if case.name in _refs:
        return _refs[case.name]
    ref = []
    for p, d in zip(case.probs, make_inputs(case)):
        a = (d["A"].t() if p.ta else d["A"]).double()
        b = (d["B"].t() if p.tb else d["B"]).double()
        r = dict(acc=a @ b, bound=(a.abs() @ b.abs()).max().item(), rowsum=a.sum(1), rowbound=a.abs().sum(1).max().item())
        for k in ("bias", "mul", "mask", "add"):
            if k in d:
                r[k] = d[k].double()
        ref.append(r)
    _refs[case.name] = ref
    return ref


def _ratio(got, want, tol):
    """max |got - want| / tol (tol a number or elementwise); NaN / Inf in got count as infinite."""
    err = (torch.from_numpy(np.ascontiguousarray(got)).double() - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return (err / tol).max().item()


PAIRS = [(s, c.name) for c in CASES for s in SETTINGS if s in c.expect]


@pytest.mark.parametrize("setting,name", PAIRS, ids=["%s-%s" % sc for sc in PAIRS])
def test_gemm_arm_against_float64(setting, name, child_dir):
    """One case in one setting: the strategy record, NaN outside the outputs, every output against float64.
    Prints the worst error / bound per output ("[arms] ...").  Measured on an MI355X: products 0.02 - 0.15 of
    their bound on every arm (X6 0.06 - 0.10, PIPE 0.04 - 0.12, PLAIN 0.06 - 0.09, MULTI_F32 0.03 - 0.15, PAIR_BWD
    0.02 - 0.14, PAIR_FWD 0.12 - 0.13, SKINNY 0.03, HEAD_BWD 0.002 / 0.04), outputs behind the four-operand
    CrossNet epilogue 0.23 - 0.45, pre-activation outputs 0.08 - 0.15, fused row sums at most 0.02.  No arm
    needed the fp32-chain yardstick."""
    case = BY_NAME[name]
    rc, err, z = results(setting, child_dir)
    assert z is not None and (name + "/rec") in z.files, err
    why = check_record(case, setting, z[name + "/rec"])
    assert why is None, (why, decode_record(z[name + "/rec"]))
    worst = {}
    covered = {}
    for i, (p, r, (arm, sk)) in enumerate(zip(case.probs, reference(case), expected_launches(case, setting))):
        x6 = arm in ("X6", "MULTI_X6")
        f = 1e-6 if x6 else 1e-5 if (arm == "HEAD_BWD" and p.ta) else 3e-6 if (sk or 1) > 1 else 2e-6
        tol = f * r["bound"]
        z64 = r["acc"]
        if arm == "HEAD_BWD" and not p.ta:
            tol = 1e-6 * z64.abs().max().item()
        if "bias" in r:
            z64 = z64 + r["bias"]
            tol = tol + U * z64.abs()
        if "zout" in p.epi:
            worst["%d/zout" % i] = _ratio(z["%s/%d/zout" % (name, i)], z64, tol)
        t = z64.clamp(min=0) if "relu" in p.epi else z64
        if "mul" in r:
            t = t * r["mul"]
            tol = tol * r["mul"].abs() + U * t.abs()
        if "mask" in r:
            t = torch.where(r["mask"] > 0, t, torch.zeros_like(t))
        if "add" in r:
            t = t + r["add"]
            tol = tol + U * t.abs()
        if p.cbuf:
            bname, width, col0 = p.cbuf
            buf = z["%s/cbuf_%s" % (name, bname)]
            covered.setdefault(bname, np.zeros(width, dtype=bool))[col0:col0 + p.N] = True
        else:
            buf, col0 = z["%s/%d/C" % (name, i)], p.c_view[0]
            outside = np.ones(buf.shape[1], dtype=bool)
            outside[col0:col0 + p.N] = False
            assert np.isnan(buf[:, outside]).all(), (name, i, "columns outside the output were written")
        worst["%d/C" % i] = _ratio(buf[:, col0:col0 + p.N], t, tol)
        if "rowsum" in p.epi:
            worst["%d/rowsum" % i] = _ratio(z["%s/%d/rowsum" % (name, i)], r["rowsum"], (1e-6 if x6 else 1e-5) * r["rowbound"])
    for bname, cov in covered.items():
        assert np.isnan(z["%s/cbuf_%s" % (name, bname)][:, ~cov]).all(), (name, bname)
    print("[arms] %-15s %-24s %s  worst error / bound: %s" % (
        setting, name, decode_record(z[name + "/rec"])[0],
        "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    bad = dict((k, v) for k, v in worst.items() if not v <= 1.0)
    assert not bad, (setting, name, bad)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_child_asserted_every_strategy_and_repeated_its_bits(setting, child_dir):
    """The child's own assertions: ops.gemm_last_strategy() after every case, equal bits from two runs of a batch."""
    rc, err, z = results(setting, child_dir)
    assert rc == 0, err


def test_same_fp32_grid_with_and_without_the_x6_switch(child_dir):
    """The lists the split-bf16 grid refuses run on k_gemm_f32_multi whatever FX_GEMM_BF16X6 says: same bits."""
    a, b = results("default", child_dir)[2], results("x6off", child_dir)[2]
    assert a is not None and b is not None
    n = 0
    for k in a.files:
        if k.startswith(("multi_n96/", "multi_rowsum_kc/")):
            assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                  b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k
            n += 1
    assert n >= 10


def test_every_strategy_is_asserted_somewhere():
    from fuxictr_amd import ops
    seen = set()
    for c in CASES:
        for exp in c.expect.values():
            seen.add(exp[0])
            seen.update(l["arm"] for l in (exp[1] or []))
    assert seen == set(ops.GEMM_STRATEGIES) - {"NONE"}


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
