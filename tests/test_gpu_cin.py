"""Every kernel arm behind fx_cin_fwd / fx_cin_bwd (csrc/fx_cin.hip, csrc/fx_cin_mfma.hip), one layer per call,
against an fp64 restatement of compressed_interaction_net.py:54-76 on the same fp32 inputs.

Bound (derived, one helper, never widened per case): for each output element
    |got - ref64| <= n * 2^-24 * A
with A the same expression evaluated on the absolute values of the inputs (fp64) and n the length of the
element's accumulation chain -- the first-order bound of an fp32 FMA chain (every product of the sum passes
through at most n roundings of relative size 2^-24; the kernels use fp32 FMA and v_mfma_f32_16x16x4_f32 only):
    Xn   F0*Mi + 2          pool  F0*Mi + 2 + D
    dX0  O*Mi + Mi + 1      dXi   O*F0 + F0 + 4
    dW, dbias  B*D + G      (G = fx_cin_workgroups() rows of `partial`, summed here in fp64)
test_bound_holds_for_an_fp32_einsum checks on the host that a plain fp32 einsum of every case stays inside it."""
import functools

import pytest
import torch

from fuxictr_amd import _lib, ops

gpu = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
NAN = float("nan")
SENT = 12345.0          # what surrounds every output; must still be there afterwards

# (F0, Mi, O, D): the smallest shapes that select each arm of the dispatcher (fx_cin_fwd / fx_cin_bwd); the
# arms a shape is expected to take are named beside it.  B = 1, 3, 9 unless the entry names its own.
DEFAULT_B = (1, 3, 9)
CASES = [
    # matrix cores, Mi <= 16: k_cin_fwd_mfma<4>, k_cin_dx_mfma<1>, k_cin_dw_mfma<1>
    ((39, 16, 16, 16), (1, 3, 9, 15, 17, 33)),
    ((11, 5, 3, 16), (1, 3, 9, 15, 17, 33)),
    ((10, 16, 1, 16), (1, 3, 9, 15, 17, 33)),         # F0 = exactly one block of 10 rows
    ((7, 9, 16, 16), (9, 4096 + 37)),                 # the grid-stride loop: 256 workgroups x 16 samples, twice
    # matrix cores, 17 <= Mi <= 40: k_cin_fwd_mfma<10>, k_cin_dx_mfma<3>, k_cin_dw_mfma<3>
    ((39, 39, 16, 16), DEFAULT_B),
    ((10, 17, 1, 16), DEFAULT_B),
    ((1, 40, 16, 16), DEFAULT_B),
    ((40, 40, 13, 16), DEFAULT_B),
    # D = 16 just outside the matrix-core class
    ((41, 16, 16, 16), DEFAULT_B),                    # F0 = 41: fwd2<16>, dx2<16,16>, dw2<16>
    ((8, 41, 16, 16), DEFAULT_B),                     # Mi = 41: fwd2<64>, dx2<64,16>, dw2<64>
    ((12, 12, 17, 16), DEFAULT_B),                    # O = 17:  fwd2<16>, dx2<16,32>, dw2<16>
    # 41 <= Mi <= 64
    ((5, 64, 7, 8), DEFAULT_B),                       # fwd2<64>, dx2<64,16>, dw2<64>
    ((6, 41, 20, 12), DEFAULT_B),                     # fwd2<64>, dx2<64,32>, dw2<64>
    # 17 <= O <= 32
    ((39, 13, 32, 4), DEFAULT_B),                     # fwd2<16>, dx2<16,32>, k_cin_bwd_dw (O*F0 = 1248)
    # Mi > 64: k_cin_fwd, k_cin_bwd_dx, k_cin_bwd_dw
    ((3, 65, 5, 8), DEFAULT_B),
    # past the second generation's LDS budget with the largest W: k_cin_fwd, k_cin_bwd_dx, dw2<40>
    ((39, 39, 16, 41), DEFAULT_B),
    # generic dX: O > 32; D > 64 (Dp = 128 != D; Dp = 256, one h-group)
    ((4, 4, 33, 8), DEFAULT_B),                       # fwd2<16>, k_cin_bwd_dx, dw2<16>
    ((3, 5, 4, 65), DEFAULT_B),                       # fwd2<16>, k_cin_bwd_dx, dw2<16>
    ((2, 2, 2, 256), DEFAULT_B),                      # fwd2<16>, k_cin_bwd_dx, dw2<16>
    # generic dW: O*F0 > 1024
    ((33, 2, 32, 4), DEFAULT_B),                      # fwd2<16>, dx2<16,32>, k_cin_bwd_dw
    ((26, 26, 40, 4), DEFAULT_B),                     # fwd2<40>, k_cin_bwd_dx, k_cin_bwd_dw
    # second generation past one round of 256 workgroups x 4 samples: fwd2<16>, dx2<16,16>, dw2<16>
    ((9, 12, 6, 8), (9, 1024 + 5)),
    # O*F0*Mi + O = 30720 floats, the limit itself: k_cin_fwd, k_cin_bwd_dx, k_cin_bwd_dw
    ((15, 17, 120, 8), DEFAULT_B),
]
SHAPES = [c[0] for c in CASES]
SHAPE_B = [(c[0], b) for c in CASES for b in c[1]]


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _chain(F0, Mi, O, D, B, G):
    n = {"xn": F0 * Mi + 2, "pool": F0 * Mi + 2 + D, "dx0": O * Mi + Mi + 1, "dxi": O * F0 + F0 + 4}
    n["dw"] = n["db"] = B * D + G
    return n


@functools.lru_cache(maxsize=None)
def _inputs(shape, B):
    """fp32 host tensors of one case; built once, never modified (callers clone what they change)."""
    F0, Mi, O, D = shape
    g = torch.Generator().manual_seed(1000 * F0 + 100 * Mi + 10 * O + D + B)
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    return {"x0": r(B, F0, D), "xi": r(B, Mi, D), "W": r(O, F0 * Mi) / (F0 * Mi) ** 0.5, "bias": r(O),
            "dxn": r(B, O, D), "dpool": r(B, O), "init": r(B, F0, D)}


def _fwd_vals(x0, xi, W, bias):
    B, _, D = x0.shape
    had = torch.einsum("bhd,bmd->bhmd", x0, xi).reshape(B, -1, D)
    xn = torch.einsum("oc,bcd->bod", W, had) + bias.view(1, -1, 1)
    return {"xn": xn, "pool": xn.sum(-1)}


def _bwd_vals(x0, xi, W, dxn, dpool, init):
    B, F0, D = x0.shape
    Mi = xi.shape[1]
    g = torch.zeros(B, W.shape[0], D, dtype=x0.dtype)
    if dxn is not None:
        g = g + dxn
    if dpool is not None:
        g = g + dpool[..., None]
    T = torch.einsum("bod,oc->bcd", g, W).view(B, F0, Mi, D)
    dx0 = (T * xi[:, None]).sum(2)
    if init is not None:
        dx0 = dx0 + init
    dxi = (T * x0[:, :, None]).sum(1)
    had = torch.einsum("bhd,bmd->bhmd", x0, xi).reshape(B, -1, D)
    return {"dx0": dx0, "dxi": dxi, "dw": torch.einsum("bod,bcd->oc", g, had), "db": g.sum((0, 2))}


def _apply(fn, args, conv):
    return fn(*[None if a is None else conv(a) for a in args])


@functools.lru_cache(maxsize=None)
def _reference(shape, B, use_dxn, use_dpool, acc, G):
    """-> {name: (ref64, bound)} of one case and mode; computed once and shared."""
    i = _inputs(shape, B)
    n = _chain(*shape, B, G)
    fa = (i["x0"], i["xi"], i["W"], i["bias"])
    ba = (i["x0"], i["xi"], i["W"], i["dxn"] if use_dxn else None, i["dpool"] if use_dpool else None,
          i["init"] if acc else None)
    ref = dict(_apply(_fwd_vals, fa, lambda t: t.double()), **_apply(_bwd_vals, ba, lambda t: t.double()))
    mag = dict(_apply(_fwd_vals, fa, lambda t: t.double().abs()), **_apply(_bwd_vals, ba, lambda t: t.double().abs()))
    return {k: (ref[k], n[k] * U * mag[k]) for k in ref}


def _check(tag, name, got, ref, bound):
    assert bool(torch.isfinite(got).all()), (tag, name, "not finite")
    err = (got.double() - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        k = int((err - bound).argmax())
        raise AssertionError("%s %s: %d of %d outside the bound; worst |err| %.3e > %.3e at flat index %d" % (
            tag, name, int(bad.sum()), err.numel(), float(err.flatten()[k]), float(bound.flatten()[k]), k))


def _split_partial(partial, O, C):
    s = partial.double().sum(0)
    return s[:O * C].view(O, C), s[O * C:O * C + O]


# ---- the host check of the bound --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", SHAPE_B, ids=_id)
def test_bound_holds_for_an_fp32_einsum(shape, B):
    """A plain fp32 einsum of the same inputs stays inside the bound the kernels are held to."""
    i = _inputs(shape, B)
    for use_dxn, use_dpool, acc in [(True, False, False), (False, True, True), (True, True, True)]:
        want = _reference(shape, B, use_dxn, use_dpool, acc, 256)
        got = _fwd_vals(i["x0"], i["xi"], i["W"], i["bias"])
        got.update(_bwd_vals(i["x0"], i["xi"], i["W"], i["dxn"] if use_dxn else None,
                             i["dpool"] if use_dpool else None, i["init"] if acc else None))
        for k, (ref, bound) in want.items():
            _check((shape, B, "fp32 einsum"), k, got[k], ref, bound)


# ---- device plumbing --------------------------------------------------------------------------------------------
class _Slot(object):
    """A [rows, width] view (row stride ld, first column col) inside a larger buffer that holds `around`
    everywhere else: 16 floats in front, the gaps between the rows, 16 floats behind."""

    def __init__(self, rows, width, ld=None, col=0, fill=NAN, around=SENT):
        ld = width if ld is None else ld
        assert col + width <= ld
        self.base = torch.full((32 + rows * ld,), around, device=DEV)
        self.span = (rows, width, ld, col)
        self.view = self._view(self.base)
        self.view.fill_(fill)

    def _view(self, base):
        rows, width, ld, col = self.span
        return base[16:16 + rows * ld].view(rows, ld)[:, col:col + width]

    def put(self, t):
        self.view.copy_(t.reshape(self.view.shape).to(DEV))
        return self

    def as3(self, rows, D):
        return self.view.view(self.view.shape[0], rows, D)

    def intact(self):
        c = self.base.clone()
        self._view(c).fill_(SENT)
        return bool((c == SENT).all())

    def cpu(self):
        return self.view.cpu()


def _ld(width, kind):
    if kind is None:
        return width
    if kind == "odd":
        return width + 1 + width % 2
    return (width // 4 + 1) * 4          # "four": the next multiple of 4 above width


def _image(shape, W_dev):
    F0, Mi, O, D = shape
    n = ops.cin_wimg_floats(F0, Mi, D, O)
    if not n:
        return None
    img = torch.empty(n, device=DEV)
    ops.cin_pack_w([(W_dev, F0, Mi, img)], D)
    return img


def _run(shape, i, use_dxn=True, use_dpool=True, acc=True, pool=True, img=False, ld=None, finite=True, tag=""):
    """One fx_cin_fwd and one fx_cin_bwd call.  ld: None (contiguous samples), "odd" or "four" (every sample-strided
    operand is a view of a [B, ld] buffer, inputs with NaN between the rows).  Outputs start as NaN (dX0 as
    i["init"] when it is accumulated into), live inside sentinel-filled buffers, and come back as host tensors."""
    F0, Mi, O, D = shape
    B, C = i["x0"].shape[0], F0 * Mi
    G, need = ops.cin_workgroups(), O * C + O
    gap = 5 if ld else 0
    x0 = _Slot(B, F0 * D, _ld(F0 * D, ld), around=NAN).put(i["x0"]).as3(F0, D)
    xi = _Slot(B, Mi * D, _ld(Mi * D, ld), around=NAN).put(i["xi"]).as3(Mi, D)
    W, bias = i["W"].to(DEV), i["bias"].to(DEV)
    dxn = i["dxn"].to(DEV) if use_dxn else None
    dpool = _Slot(B, O, O + gap, gap // 2, around=NAN).put(i["dpool"]).view if use_dpool else None
    w_img = _image(shape, W) if img else None
    out = {"xn": _Slot(B, O * D),
           "pool": _Slot(B, O, O + 5, 2) if pool else None,
           "dx0": _Slot(B, F0 * D, _ld(F0 * D, ld)),
           "dxi": _Slot(B, Mi * D, _ld(Mi * D, ld)),
           "partial": _Slot(G, need, need + (7 if ld else 0), 3 if ld else 0)}
    if acc:
        out["dx0"].put(i["init"])
    ops.cin_fwd(x0, xi, W, bias, out["xn"].as3(O, D), out["pool"].view if pool else None, w_img)
    ops.cin_bwd(x0, xi, W, dxn, dpool, out["dx0"].as3(F0, D), acc, out["dxi"].as3(Mi, D), out["partial"].view,
                w_img)
    torch.cuda.synchronize()
    res = {}
    for k, s in out.items():
        if s is None:
            continue
        assert s.intact(), (tag, k, "wrote outside its rows")
        res[k] = s.cpu()
        if finite:
            assert bool(torch.isfinite(res[k]).all()), (tag, k, "left unwritten or not finite")
    return res


def _compare(tag, shape, B, res, use_dxn, use_dpool, acc):
    F0, Mi, O, D = shape
    want = _reference(shape, B, use_dxn, use_dpool, acc, ops.cin_workgroups())
    dw, db = _split_partial(res["partial"], O, F0 * Mi)
    got = {"xn": res["xn"].view(B, O, D), "pool": res.get("pool"), "dx0": res["dx0"].view(B, F0, D),
           "dxi": res["dxi"].view(B, Mi, D), "dw": dw, "db": db}
    for k, (ref, bound) in want.items():
        if got[k] is not None:
            _check(tag, k, got[k], ref, bound)


def _has_image(shape):
    F0, Mi, O, D = shape
    return ops.cin_wimg_floats(F0, Mi, D, O) > 0


# ---- the kernels against fp64 -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,B", SHAPE_B, ids=_id)
def test_cin_layer_matches_fp64_in_every_mode(shape, B):
    """dXn only / dpool only / both, dX0 written and accumulated into, pool absent and a column slice, W image given
    and gathered by the kernels: every output within the bound, nothing unwritten, nothing written outside."""
    i = _inputs(shape, B)
    for img in ([True, False] if _has_image(shape) else [False]):
        for use_dxn, use_dpool in [(True, False), (False, True), (True, True)]:
            for acc in (False, True):
                pool = acc != use_dxn            # both values with each gradient mode's pair of runs
                tag = (shape, B, "dxn" if use_dxn else "", "dpool" if use_dpool else "", "acc" if acc else "",
                       "pool" if pool else "", "img" if img else "")
                res = _run(shape, i, use_dxn, use_dpool, acc, pool, img, tag=tag)
                _compare(tag, shape, B, res, use_dxn, use_dpool, acc)


@gpu
@pytest.mark.parametrize("ld", ["odd", "four"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_cin_sample_strides_give_the_contiguous_bits(shape, ld):
    """include/fxctr.h: x0_ld, xi_ld, dx0_ld, dxi_ld, pool_ld, dpool_ld, partial_ld.  X0, Xi, dX0, dXi as views of
    [B, ld] buffers (NaN between the input rows), dpool / pool / partial as column slices: the same bits as the
    contiguous call, and within the bound."""
    B = 9
    i = _inputs(shape, B)
    img = _has_image(shape)
    plain = _run(shape, i, img=img, tag=(shape, "contiguous"))
    strided = _run(shape, i, img=img, ld=ld, tag=(shape, "ld " + ld))
    _compare((shape, "ld " + ld), shape, B, strided, True, True, True)
    for k in plain:
        assert torch.equal(plain[k], strided[k]), (shape, ld, k)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_cin_samples_do_not_see_each_other(shape):
    """Sample 4 of X0, Xi, dXn and dpool set to NaN: Xn, pool, dX0 and dXi of the other eight samples keep their bits."""
    B = 9
    i = _inputs(shape, B)
    bad = {k: v.clone() for k, v in i.items()}
    for k in ("x0", "xi", "dxn", "dpool"):
        bad[k][4] = NAN
    for img in ([True, False] if _has_image(shape) else [False]):
        clean = _run(shape, i, img=img, tag=(shape, "clean"))
        dirty = _run(shape, bad, img=img, finite=False, tag=(shape, "sample 4 NaN"))
        keep = [0, 1, 2, 3, 5, 6, 7, 8]
        for k in ("xn", "pool", "dx0", "dxi"):
            assert bool(torch.isfinite(dirty[k][keep]).all()), (shape, k, "NaN leaked out of sample 4")
            assert torch.equal(clean[k][keep], dirty[k][keep]), (shape, k)


@gpu
@pytest.mark.parametrize("shape,B", [(c[0], c[1][-1]) for c in CASES], ids=_id)
def test_cin_is_deterministic(shape, B):
    """Fixed reduction order: the same call twice, identical bits in every output, `partial` included."""
    i = _inputs(shape, B)
    a = _run(shape, i, img=_has_image(shape))
    b = _run(shape, i, img=_has_image(shape))
    for k in a:
        assert torch.equal(a[k], b[k]), (shape, B, k)


@gpu
@pytest.mark.parametrize("shape,short_partial", [((15, 17, 121, 8), False), ((1, 1, 1, 257), False),
                                                 ((5, 4, 3, 8), True)], ids=_id)
def test_cin_rejections_launch_nothing(shape, short_partial):
    """One float past the LDS-resident limit, D = 257, partial_ld < O*F0*Mi + O: an error through ops.check, and
    every output as it was."""
    F0, Mi, O, D = shape
    B, G, need = 3, ops.cin_workgroups(), O * F0 * Mi + O
    i = _inputs(shape, B)
    dev = {k: v.to(DEV) for k, v in i.items()}
    out = {"xn": _Slot(B, O * D), "pool": _Slot(B, O), "dx0": _Slot(B, F0 * D), "dxi": _Slot(B, Mi * D),
           "partial": _Slot(G, need)}
    partial = out["partial"].view
    if short_partial:
        partial = torch.as_strided(out["partial"].base, (G, need), (need - 1, 1), 16)
    else:
        with pytest.raises(_lib.FxError):
            ops.cin_fwd(dev["x0"], dev["xi"], dev["W"], dev["bias"], out["xn"].as3(O, D), out["pool"].view)
    with pytest.raises(_lib.FxError):
        ops.cin_bwd(dev["x0"], dev["xi"], dev["W"], dev["dxn"], dev["dpool"], out["dx0"].as3(F0, D), False,
                    out["dxi"].as3(Mi, D), partial)
    torch.cuda.synchronize()
    for k, s in out.items():
        assert s.intact() and bool(torch.isnan(s.view).all()), (shape, k)


# ---- stacks whose layers are wider than one call ----------------------------------------------------------------
def _stack_reference(x0, wb, gy, G, n_calls):
    """fp64 forward and backward of a CIN stack with the per-layer bound chained: a layer's bound is its own
    n * 2^-24 * A plus, to first order, what the errors of its inputs (the previous layer's Xn on the way up, the
    next layer's dXi on the way down) become in its outputs -- the same expressions on (|.|, error) operands.
    -> pooled, dX0, [dW_i, dbias_i ...] as (ref64, bound) pairs."""
    d, ab = (lambda t: t.double()), (lambda t: t.double().abs())
    B, F0, D = x0.shape
    n = len(wb) // 2
    X0 = d(x0)
    xs, exs, pooled = [X0], [torch.zeros_like(X0)], []
    for l in range(n):
        W, b = d(wb[2 * l])[:, :, 0], d(wb[2 * l + 1])
        O, Mi = W.shape[0], xs[l].shape[1]
        ch = _chain(F0, Mi, O, D, B, G)
        val, mag = _fwd_vals(X0, xs[l], W, b), _fwd_vals(X0.abs(), xs[l].abs() + exs[l], W.abs(), b.abs())
        prop = _fwd_vals(X0.abs(), exs[l], W.abs(), torch.zeros_like(b))
        xs.append(val["xn"])
        exs.append(ch["xn"] * U * mag["xn"] + prop["xn"])
        pooled.append((val["pool"], ch["pool"] * U * mag["pool"] + prop["pool"]))
    pool_ref = torch.cat([p[0] for p in pooled], 1), torch.cat([p[1] for p in pooled], 1)
    dx0, edx0, mdx0 = torch.zeros_like(X0), torch.zeros_like(X0), torch.zeros_like(X0)
    dxn, edxn, grads, off = None, None, [None] * (2 * n), pool_ref[0].shape[1]
    for l in range(n - 1, -1, -1):
        W = d(wb[2 * l])[:, :, 0]
        O, Mi = W.shape[0], xs[l].shape[1]
        off -= O
        dpool = d(gy)[:, off:off + O]
        ch = _chain(F0, Mi, O, D, B, G)
        val = _bwd_vals(X0, xs[l], W, dxn, dpool, None)
        mag = _bwd_vals(X0.abs(), xs[l].abs() + exs[l], W.abs(), None if dxn is None else dxn.abs() + edxn,
                        dpool.abs(), None)
        # what the errors of g (edxn) and of Xi (exs[l]) become; dXi does not read Xi
        pg = _bwd_vals(X0.abs(), xs[l].abs(), W.abs(), edxn, None, None) if edxn is not None else None
        px = _bwd_vals(X0.abs(), exs[l], W.abs(), None if dxn is None else dxn.abs() + edxn, dpool.abs(), None)
        err = {}
        for k in ("dx0", "dxi", "dw", "db"):
            extra = n_calls[l] if k in ("dx0", "dxi") else 0        # the adds that join a split layer's calls
            err[k] = (ch[k] + extra) * U * mag[k]
            if pg is not None:
                err[k] = err[k] + pg[k]
            if k in ("dx0", "dw"):
                err[k] = err[k] + px[k]
        dx0, edx0, mdx0 = dx0 + val["dx0"], edx0 + err["dx0"], mdx0 + mag["dx0"]
        grads[2 * l] = (val["dw"].unsqueeze(-1), err["dw"].unsqueeze(-1))
        grads[2 * l + 1] = (val["db"], err["db"])
        dxn, edxn = val["dxi"], err["dxi"]
        last_mag = mag["dxi"]
    # dX0 = (sum over the layers) + dXi of layer 1: one more rounded add
    dx0_ref = (dx0 + dxn, edx0 + edxn + U * (mdx0 + last_mag))
    return pool_ref, dx0_ref, grads


# (F0, units, D, B, calls per layer)
STACKS = [(39, [21, 32], 4, 9, [2, 1]),          # 21*39*39 + 21 = 31962 floats: maps 0-10 and 11-20; 26240 fit
          (15, [121], 8, 3, [1]),                # 121*15*15 + 121 = 27346 floats fit one call (generic kernels)
          (39, [32, 32, 32], 16, 9, [2, 2, 2])]  # the reference's default CIN: two matrix-core calls of 16 maps each


def _stack_inputs(F0, units, D, B):
    g = torch.Generator().manual_seed(F0 + D + B + sum(units))
    x0 = torch.randn(B, F0, D, generator=g) * 0.5
    wb, prev = [], F0
    for u in units:
        wb += [torch.randn(u, F0 * prev, 1, generator=g) / (F0 * prev) ** 0.5, torch.randn(u, generator=g) * 0.1]
        prev = u
    return x0, wb, torch.randn(B, sum(units), generator=g)


def _stack_run(x0, wb, gy, device):
    from fuxictr_amd import layers as L
    leaves = [t.clone().to(device).requires_grad_(True) for t in [x0] + wb]
    pooled = L._CINFn.apply(*leaves)
    pooled.backward(gy.to(device))
    return pooled.detach().cpu(), [t.grad.cpu() for t in leaves]


@gpu
@pytest.mark.parametrize("F0,units,D,B,calls", STACKS, ids=_id)
def test_cin_stack_splits_layers_wider_than_one_call(F0, units, D, B, calls, monkeypatch):
    """_CINFn on layers whose O*F0*Mi + O exceeds ops.CIN_MAX_W_FLOATS: pooled outputs and every gradient within
    the chained bound of the fp64 reference, on the device and through the host emulation of the same calls."""
    x0, wb, gy = _stack_inputs(F0, units, D, B)
    n_calls = [len(ops.cin_chunks(F0, m, u)) for u, m in zip(units, [F0] + units)]
    assert n_calls == calls
    pool_ref, dx0_ref, grad_refs = _stack_reference(x0, wb, gy, ops.cin_workgroups(), n_calls)
    runs = [("device", _stack_run(x0, wb, gy, DEV))]
    import _cpu_emul
    _cpu_emul.install(monkeypatch)
    runs.append(("emulation", _stack_run(x0, wb, gy, "cpu")))
    for where, (pooled, grads) in runs:
        _check((where, F0, units), "pooled", pooled, *pool_ref)
        _check((where, F0, units), "dX0", grads[0], *dx0_ref)
        for k, (got, (ref, bound)) in enumerate(zip(grads[1:], grad_refs)):
            _check((where, F0, units), "grad %d" % k, got, ref, bound)


@gpu
def test_reference_default_cin_trains_a_step():
    """CompressedInteractionNet(39, [32, 32, 32]) (xDeepFM_default's cin_hidden_units): forward, backward and an SGD
    step on the device; the loss of the same batch goes down."""
    from fuxictr_amd import layers as L
    g = torch.Generator().manual_seed(7)
    cin = L.CompressedInteractionNet(39, [32, 32, 32]).to(DEV)
    x = (torch.randn(64, 39, 16, generator=g) * 0.3).to(DEV)
    y = torch.randn(64, 1, generator=g).to(DEV)
    opt = torch.optim.SGD(cin.parameters(), lr=1e-2)
    losses = []
    for _ in range(2):
        opt.zero_grad()
        loss = ((cin(x) - y) ** 2).mean()
        loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in cin.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[1] < losses[0], losses
