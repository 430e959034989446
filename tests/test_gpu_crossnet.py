"""DCN's kernels (csrc/fx_crossnet.hip) alone, through fuxictr_amd.ops, on a real MI355X against an fp64
torch-autograd restatement of the plain layer loop (tests/test_dcn_host.py):
    x_{l+1} = x_l + ((w_l . x_l) * x_0 + b_l),   s_l = w_l . x_l
    forward   out = x_L and the stash s [rows, L]
    backward  dx0 (= | +=), dw [L, cols], db [L, cols] from dout, x0, w, b and s

The tolerance is the yardstick of tests/test_gpu_layernorm.py (`compare`, `f32_exact`): the same formulas in fp32
torch on the CPU have an error e32 against the fp64 result, per output tensor (max |.|); the HIP result must lie
within
    4 * e32 + 1e-6 * max|ref|.
Every case prints its observed ratio err / bound.  The inputs are fp32 numbers, so all three computations start from
the same values.  No element is left out of any comparison.  Where dx0 is ADDED to a buffer that holds 3.0 and the
3.0 is taken off again here, that round trip's one rounding (2^-22 max(1, |.|)) is allowed for, as
test_gpu_gatecross.py does.

Every matrix is handed over as the columns [off, off + cols) of wider rows with `tail` more columns behind them, the
packed arrays (w, b, s, dw, db, the workspace) as the elements [off, off + n) of longer ones, sentinels outside: off 0
/ tail 0 is the packed case (the 16-byte arm when cols % 4 == 0), off 4 the 16-byte arm through row strides, off 1 a
base that is only 4-byte aligned and tail 3 a row stride that is no multiple of 4 (the scalar arm whatever cols is).
The shapes come from ops.cross_net_limits(): the edges of a lane's and a wave's chunks of a row, the widest rows,
one row below, at and above a workgroup's tile, and more row tiles than the grid cap has workgroups."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fuxictr_amd import ops  # noqa: E402
from test_dcn_host import cross_net_fwd_reference, cross_net_reference  # noqa: E402
from test_gpu_layernorm import compare, f32_exact  # noqa: E402

DEV = "cuda:0"
LIM = ops.cross_net_limits()
TILE, CAP, MAXC, MAXL = LIM["tile_rows"], LIM["max_wg"], LIM["max_cols"], LIM["max_layers"]

# (rows, cols, L).  The widths: the edges of the 4-byte and 16-byte chunks of a lane (1, 3, 4, 5), of a wave's sweep
# (63 .. 65 and 255 .. 260 floats), a production width and the widest rows; L cycles through 1, 2, 3 and the most
# layers so that each of them runs on the 16-byte arm (cols 256, 64 / MAXC, 4 / 260, 624) and on the scalar arm
COLS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 624, MAXC - 1, MAXC]
SHAPES = [(5, c, (1, 2, 3, MAXL)[i % 4]) for i, c in enumerate(COLS)]
# one row, and one row below, at and above a workgroup's tile of rows, and two tiles and a row: both arms
SHAPES += [(r, c, L) for r in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1) for c, L in ((6, 3), (8, 2))]
# more tiles than workgroups: the row loop under the grid cap runs twice, the reduction sees the most partials
SHAPES += [(CAP * TILE + 3, 8, 2)]
LAYOUTS = [(off, tail) for off in (0, 1, 4) for tail in (0, 3)]


def make_inputs(shape, seed):
    rows, cols, L = shape
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s, scale=1.0):
        return f32_exact(scale * torch.randn(*s, generator=gen, dtype=torch.float64))
    return dict(x0=rnd(rows, cols), w=rnd(L, cols, scale=0.5 * cols ** -0.5), b=rnd(L, cols, scale=0.3),
                dout=rnd(rows, cols))


def run_torch(inp, dtype):
    t = {k: v.to(dtype).clone() for k, v in inp.items()}
    for k in ("x0", "w", "b"):
        t[k].requires_grad_(True)
    out = cross_net_reference(t["x0"], t["w"], t["b"])
    dx0, dw, db = torch.autograd.grad(out, [t["x0"], t["w"], t["b"]], t["dout"])
    with torch.no_grad():
        s = cross_net_fwd_reference(t["x0"], t["w"], t["b"])[1]
    return {"out": out.detach().double(), "s": s.double(), "dx0 1": dx0.double(), "dx0 0": dx0.double(),
            "dw": dw.double(), "db": db.double()}


def run_hip(inp, off=0, tail=0):
    rows, cols = inp["x0"].shape
    L = inp["w"].shape[0]
    held, flats = [], []

    def wide(fill, src=None):
        buf = torch.full((rows, off + cols + tail), fill, dtype=torch.float32, device=DEV)
        view = buf[:, off:off + cols]
        if src is not None:
            view.copy_(src.float())
        held.append((buf, fill))
        return view

    def flat(shape, fill, src=None):
        n = shape[0] * shape[1] if len(shape) == 2 else shape[0]
        buf = torch.full((off + n + tail,), fill, dtype=torch.float32, device=DEV)
        view = buf[off:off + n].view(*shape)
        if src is not None:
            view.copy_(src.float())
        flats.append((buf, n, fill))
        return view
    x0, dout = wide(7.5, inp["x0"]), wide(9.0, inp["dout"])
    w, b = flat((L, cols), 6.0, inp["w"]), flat((L, cols), 6.5, inp["b"])
    out, s = wide(5.0), flat((rows, L), 5.5)
    ops.cross_net_fwd(x0, w, b, out, s)
    bare = wide(5.0)
    ops.cross_net_fwd(x0, w, b, bare, None)                     # no stash: the same bits
    assert torch.equal(bare, out)
    res = {"out": out.contiguous(), "s": s.clone()}
    ws = flat((ops.cross_net_workspace_floats(rows, cols, L),), 2.0)
    for init in (True, False):
        dx0, dw, db = wide(3.0), flat((L, cols), 4.0), flat((L, cols), 4.5)
        ops.cross_net_bwd(dout, x0, w, b, s, dx0, dw, db, init, ws)
        res["dx0 %d" % init] = dx0.contiguous() if init else dx0 - 3.0
        if "dw" in res:
            assert torch.equal(res["dw"], dw) and torch.equal(res["db"], db)     # the flag does not touch them
        res["dw"], res["db"] = dw.clone(), db.clone()
    torch.cuda.synchronize()
    for buf, fill in held:                                      # nobody's columns
        assert bool((buf[:, :off] == fill).all()) and bool((buf[:, off + cols:] == fill).all())
    for buf, n, fill in flats:
        assert bool((buf[:off] == fill).all()) and bool((buf[off + n:] == fill).all())
    # the inputs are read only, the stash and the packed weights in the backward too
    for view, src in ((x0, "x0"), (dout, "dout"), (w, "w"), (b, "b")):
        assert torch.equal(view.cpu(), inp[src].float()), src
    assert torch.equal(s, res["s"])
    return res


def check(tag, inp, ref, f32, **layout):
    got = run_hip(inp, **layout)
    assert sorted(got) == sorted(ref)
    # (3 + dx0) - 3 in fp32: one rounding at magnitude <= 4 max(1, |dx0|)
    extra = {"dx0 0": 2.0 ** -22 * max(1.0, float(ref["dx0 0"].abs().max()))}
    compare(tag, got, ref, f32, extra=extra)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d-c%d-L%d" % s)
def test_forward_and_gradients_within_the_fp32_yardstick_in_every_layout(shape):
    inp = make_inputs(shape, seed=41 + 3 * shape[0] + shape[1] + 7 * shape[2])
    ref, f32 = run_torch(inp, torch.float64), run_torch(inp, torch.float32)
    for off, tail in LAYOUTS:
        tag = "cross_net %s off %d tail %d" % (shape, off, tail)
        first = check(tag, inp, ref, f32, off=off, tail=tail)
        if (off, tail) in ((0, 0), (1, 3)):
            again = run_hip(inp, off=off, tail=tail)                    # the same inputs: the same bits
            for name in first:
                assert torch.equal(first[name], again[name]), name


def test_every_layer_count_runs_on_both_arms():
    """The claim of the shape list, checked: L = 1, 2, 3 and the most layers each meet a width that is a multiple of 4
    (the 16-byte arm at off 0 / tail 0) and one that is not."""
    for L in (1, 2, 3, MAXL):
        assert any(c % 4 == 0 for _, c, n in SHAPES if n == L) and any(c % 4 for _, c, n in SHAPES if n == L), L
    assert MAXC >= 1248 and MAXL >= 3 and (CAP * TILE + 3, 8, 2) in SHAPES


def test_bad_arguments_are_rejected_before_the_launch():
    from fuxictr_amd._lib import FxError
    x = torch.zeros(4, 8, device=DEV)
    w = torch.zeros(2, 8, device=DEV)
    s = torch.zeros(4, 2, device=DEV)
    ws = torch.empty(ops.cross_net_workspace_floats(4, 8, 2), device=DEV)
    out = torch.full((4, 8), 5.0, device=DEV)
    with pytest.raises(AssertionError):                                  # w, b of another width than x0
        ops.cross_net_fwd(x, torch.zeros(2, 12, device=DEV), torch.zeros(2, 12, device=DEV), out)
    with pytest.raises(AssertionError):
        ops.cross_net_bwd(x, x, w[:, :4].contiguous(), w[:, :4].contiguous(), s, torch.empty_like(x),
                          torch.empty_like(w), torch.empty_like(w), True, ws)
    deep = torch.zeros(MAXL + 1, 8, device=DEV)                          # more layers than the limit
    with pytest.raises(FxError, match="L="):
        ops.cross_net_fwd(x, deep, deep, out)
    with pytest.raises(FxError, match="L="):
        ops.cross_net_bwd(x, x, deep, deep, torch.zeros(4, MAXL + 1, device=DEV), torch.empty_like(x),
                          torch.empty_like(deep), torch.empty_like(deep), True,
                          torch.empty(4 * (MAXL + 3) * 8, device=DEV))
    wide = torch.zeros(2, MAXC + 4, device=DEV)                          # wider rows than the limit
    with pytest.raises(FxError, match="cols="):
        ops.cross_net_fwd(wide, wide, wide, torch.empty_like(wide))
    with pytest.raises(FxError, match="GPU"):
        ops.cross_net_fwd(x.cpu(), w.cpu(), w.cpu(), torch.empty(4, 8))
    with pytest.raises(FxError, match="GPU"):
        ops.cross_net_bwd(x.cpu(), x.cpu(), w.cpu(), w.cpu(), s.cpu(), torch.empty(4, 8), torch.empty(2, 8),
                          torch.empty(2, 8), True, ws.cpu())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())                                      # nothing was launched
