"""Thin tensor-level wrappers over the C-ABI (include/fxctr.h).

torch is plumbing here: it owns device memory and the stream; every computation below is a call
into libfxctr.so.  All functions require CUDA(HIP) fp32/int32 contiguous tensors and raise
otherwise — there is no CPU path.
"""
import ctypes as C
import os
from collections import OrderedDict

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr, vp

_DT = {torch.float32: _lib.FX_F32, torch.float64: _lib.FX_F64,
       torch.int32: _lib.FX_I32, torch.int64: _lib.FX_I64}


class KernelTimer(object):
    """Opt-in kernel timing for bench.py's roofline objects, off (zero cost) otherwise.

    Per-launch HIP events are useless at this kernel size on this platform: an event pair around
    one launch adds ~10 us (measured: 87.7 us for a GEMM rocprofv3 times at 75 us, 12.5 us for the
    8.5 us gather, even with the stream kept busy).  So the launches of eager training steps are
    RECORDED (entry point + its live arguments, tagged with the step they belong to) and then each
    recorded launch group is REPLAYED `reps` times back to back between one event pair:
    average = kernel duration + the ~1.3 us dependent-launch boundary — what rocprofv3's kernel
    trace reports, within a few per cent.

    HBM-bound groups (`multi_step`: the sparse path, the gather on its own) are replayed ROUND-ROBIN over
    ALL recorded steps — each step holds its own batch, ids, de-dup result and gradients — so that a
    launch meets rows it has not seen for (steps - 1) other batches, as inside the training step; a
    single batch replayed back to back would find its rows in the 256 MB Infinity Cache.
    MFMA-bound groups (one GEMM shape) use the first recorded step only.

    The replay RE-EXECUTES the recorded launches with their live arguments: the optimizer step counter
    advances, row updates are applied again, outputs are overwritten.  The model / optimizer state is
    no longer the trained trajectory afterwards — bench.py discards the model after this pass."""
    recording = False
    calls = []       # (name, group, work, fn, args, kwargs, step)
    step = 0
    multi_step = ("sparse_path",)

    @classmethod
    def note(cls, name, group, work, fn, args, kwargs):
        if cls.step > 0 and not ((group or name) in cls.multi_step or name.endswith("@alone")):
            return                     # MFMA-bound groups: the first recorded step is enough
        cls.calls.append((name, group, work, fn, args, kwargs, cls.step))

    @classmethod
    def next_step(cls):
        cls.step += 1

    @classmethod
    def replay(cls, reps=20):
        """-> name/group -> dict(launches, total_ms, avg_us, work) PER RECORDED STEP.
        The recorded launches of one group (a GEMM shape, the sparse path) are captured, in step
        order, into ONE hipGraph; the graph is replayed `reps` times between one event pair.  That
        is how the timed region itself executes them (graph launch, dependent boundaries, the same
        mix of shapes following each other), so the averages line up with rocprofv3's kernel trace
        of the timed region."""
        was, cls.recording = cls.recording, False
        groups = {}
        for c in cls.calls:
            groups.setdefault(c[1] or c[0], []).append(c)
        out = {}
        try:
            side = torch.cuda.Stream()
            for key, calls in groups.items():
                steps = sorted(set(c[6] for c in calls))
                if not (key in cls.multi_step or key.endswith("@alone")):
                    calls = [c for c in calls if c[6] == steps[0]]
                    steps = steps[:1]
                for c in calls:                                      # warm (allocations, caches)
                    c[3](*c[4], **c[5])
                torch.cuda.synchronize()
                # a group of ONE launch: ten copies of it in the graph, so that the graph launch itself
                # (several us) does not sit in a 10-us kernel's figure
                copies = 10 if len(calls) == 1 else 1
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    for _ in range(copies):
                        for c in calls:
                            c[3](*c[4], **c[5])
                g.replay()
                torch.cuda.synchronize()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                per_call_ms = e0.elapsed_time(e1) / reps / (len(calls) * copies)
                if not key.endswith("@alone"):
                    # every launch of one step, whatever its group: bench.py's `kernel_sum_us`
                    tot = out.setdefault("__step__", {"launches": 0.0, "total_ms": 0.0, "work": 0.0,
                                                      "steps": 1})
                    tot["launches"] += len(calls) / float(len(steps))
                    tot["total_ms"] += per_call_ms * len(calls) / len(steps)
                for c in calls:
                    for k in (c[0], c[1]):
                        if k is None:
                            continue
                        o = out.setdefault(k, {"launches": 0.0, "total_ms": 0.0, "work": 0.0,
                                               "steps": len(steps)})
                        o["launches"] += 1.0 / len(steps)
                        o["total_ms"] += per_call_ms / len(steps)
                        o["work"] += float(c[2]) / len(steps)
                del g
        finally:
            cls.recording = was
        for o in out.values():
            o["avg_us"] = 1e3 * o["total_ms"] / max(o["launches"], 1e-9)
        return out

    @classmethod
    def reset(cls):
        cls.calls = []
        cls.step = 0


def _timed(name, group=None, work=None, alone=False):
    """Decorator: when KernelTimer is recording, note this C-ABI call (it still runs normally).
    alone: besides its group, time the call on its own under `name` (idempotent calls only)."""
    def deco(fn):
        def wrapper(*a, **kw):
            if KernelTimer.recording:
                w = work(*a, **kw) if work else 0
                KernelTimer.note(name, group, w, fn, a, kw)
                if alone and group:
                    KernelTimer.note(name + "@alone", None, w, fn, a, kw)
            return fn(*a, **kw)
        wrapper.__name__ = fn.__name__
        wrapper.__doc__ = fn.__doc__
        wrapper.__wrapped__ = fn
        return wrapper
    return deco


def _need_cuda(t, name):
    if not t.is_cuda:
        raise _lib.FxError("%s must live on the GPU: the native path has no CPU fallback "
                           "(got device %s)" % (name, t.device))


# worst relative error of a table entry (against the directly summed series) that the catch-up accepts: the
# replay it replaces carries ~2e-7 from its approximate reciprocals
SERIES_MAX_ERR = 2.5e-7
_series_cache = {}          # (device, beta1, beta2) -> (tcap, table words incl. header) of a checked table


def series_tcap(beta1, beta2):
    """Entries of the Adam series table: one per step until both bias corrections are 1 in fp32."""
    import math
    if not (0.0 < beta1 < 1.0 and 0.0 < beta2 < 1.0):
        return 0
    t = max(math.log(2.0 ** -26) / math.log(beta1), math.log(2.0 ** -26) / math.log(beta2))
    t = int(math.ceil(t / 1024.0)) * 1024
    return t if 256 <= t <= (1 << 20) else 0


def new_scalars(device, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, series=False):
    """Allocate and initialise a device-resident fx_scalars block (16 x 4-byte words).  series=True (the
    exact-mode Adam of the tables): the block is followed, in the same allocation, by the Adam series table
    of (beta1, beta2) — fx_adam_series_build; FX_CATCHUP_SERIES=0 leaves it out (the step-by-step replay)."""
    host = torch.zeros(_lib.SC_WORDS, dtype=torch.float32)
    host[_lib.SC_LR] = lr
    host[_lib.SC_BETA1] = beta1
    host[_lib.SC_BETA2] = beta2
    host[_lib.SC_EPS] = eps
    host[_lib.SC_CLIP] = 1.0
    host[_lib.SC_MAX_NORM] = max_norm
    device = torch.device(device)
    tcap = series_tcap(beta1, beta2) if series and os.environ.get("FX_CATCHUP_SERIES", "1") != "0" else 0
    if tcap == 0 or device.type != "cuda":
        return host.to(device)
    lib = _lib.load()
    words = int(lib.fx_adam_series_words(tcap))
    buf = torch.zeros(_lib.SC_WORDS + words, dtype=torch.float32, device=device)
    scal = buf[:_lib.SC_WORDS]              # (a view: the table lives as long as the block)
    scal.copy_(host)
    key = (str(device), float(host[_lib.SC_BETA1]), float(host[_lib.SC_BETA2]))      # (as fp32 holds them)
    hit = _series_cache.get(key)
    if hit is None:
        check(lib.fx_adam_series_build(ptr(scal), tcap, stream_ptr(device)), "fx_adam_series_build")
        err = float(buf[_lib.SC_WORDS + 2].item())          # one host sync per (device, betas)
        ok = err <= SERIES_MAX_ERR
        _series_cache[key] = (tcap, buf[_lib.SC_WORDS:].clone() if ok else None, err)
        if not ok:
            import logging
            logging.warning("Adam series table for betas (%g, %g): worst entry error %.2e > %.1e - the "
                            "exact-mode catch-up keeps the step-by-step replay", beta1, beta2, err,
                            SERIES_MAX_ERR)
            scal.view(torch.int32)[_lib.SC_SERIES_TCAP:_lib.SC_SERIES_TCAP + 1].fill_(0)
    elif hit[1] is not None:
        buf[_lib.SC_WORDS:].copy_(hit[1])
        scal.view(torch.int32)[_lib.SC_SERIES_TCAP:_lib.SC_SERIES_TCAP + 1].fill_(tcap)
    return scal


def series_error(scal):
    """Worst entry error the builder measured for the table behind `scal` (None: no table)."""
    if int(scal.view(torch.int32)[_lib.SC_SERIES_TCAP].item()) == 0:
        return None
    hit = _series_cache.get((str(scal.device), float(scal[_lib.SC_BETA1].item()), float(scal[_lib.SC_BETA2].item())))
    return None if hit is None else hit[2]


@_timed("pack_columns", "other")
def pack_columns(cols, out, out_col0=0):
    """cols: list of [B] or [B, w] device tensors -> out[:, out_col0:...] (int32 or float32)."""
    lib = _lib.load()
    B = out.shape[0]
    i = 0
    col = out_col0
    while i < len(cols):
        chunk = cols[i:i + _lib.FX_PACK_MAX_COLS]
        keep = []
        dts, ws = [], []
        for t in chunk:
            _need_cuda(t, "input column")
            if t.dtype not in _DT:
                raise _lib.FxError("unsupported input dtype %s" % t.dtype)
            if not t.is_contiguous():
                t = t.contiguous()
            if t.shape[0] != B:
                raise _lib.FxError("input column has %d rows, expected %d" % (t.shape[0], B))
            keep.append(t)
            dts.append(_DT[t.dtype])
            ws.append(1 if t.dim() == 1 else int(t.shape[1]))
        check(lib.fx_pack_columns(_lib.ptr_array(keep), _lib.i32_array(dts), _lib.i32_array(ws),
                                  len(keep), B, _DT[out.dtype], ptr(out), out.stride(0), col,
                                  stream_ptr(out.device)), "fx_pack_columns")
        col += sum(ws)
        i += len(chunk)
    return out


def _gather_bytes(table, D, ids, col_row_base, col_vocab, col_out_off, dense, num_w,
                  num_out_off, out, scal, n_cols=None):
    # algorithmic bytes: rows + ids + dense in, the [B,F,D] record out
    B = out.shape[0]
    C_ = 0 if ids is None else (ids.shape[1] if n_cols is None else n_cols)
    Fd = 0 if dense is None else dense.shape[1]
    return B * (C_ * (4 * D + 4) + Fd * 4 + (C_ + Fd) * 4 * D)


def _row_ld(table):
    """Row stride in elements of a [rows, D] table that may be a field of a row record (0: packed)."""
    if table is None or table.dim() != 2:
        return 0
    assert table.stride(1) == 1, "table rows must be contiguous"
    return int(table.stride(0))


@_timed("k_emb_gather_fwd", "sparse_path", _gather_bytes)
def emb_gather_fwd(table, D, ids, col_row_base, col_vocab, col_out_off, dense, num_w,
                   num_out_off, out, scal, n_cols=None):
    """n_cols: gather only the first n_cols id columns (the rest are pooled sequences)."""
    lib = _lib.load()
    B = out.shape[0]
    C_ = 0 if ids is None else (ids.shape[1] if n_cols is None else n_cols)
    Fd = 0 if dense is None else dense.shape[1]
    check(lib.fx_emb_gather_fwd(ptr(table), D, ptr(ids), 0 if ids is None else ids.stride(0),
                                ptr(col_row_base), ptr(col_vocab), ptr(col_out_off), C_,
                                ptr(dense), 0 if dense is None else dense.stride(0), ptr(num_w),
                                ptr(num_out_off), Fd, ptr(out), out.stride(0), B, ptr(scal),
                                _row_ld(table), stream_ptr(out.device)), "fx_emb_gather_fwd")
    return out


POOL_SUM, POOL_MEAN = 0, 1


@_timed("emb_seq_pool_fwd", "sparse_path")
def emb_seq_pool_fwd(table, D, ids, col_row_base, col_vocab, seq_col0, seq_len, seq_mode,
                     seq_out_off, out, denom, scal):
    """Pooled sequence features -> their slots of the record `out`; denom [B, n_seq] out."""
    lib = _lib.load()
    B, n_seq = denom.shape
    check(lib.fx_emb_seq_pool_fwd(ptr(table), D, ptr(ids), ids.stride(0), ptr(col_row_base),
                                  ptr(col_vocab), ptr(seq_col0), ptr(seq_len), ptr(seq_mode),
                                  ptr(seq_out_off), n_seq, ptr(out), out.stride(0), ptr(denom),
                                  B, ptr(scal), _row_ld(table), stream_ptr(out.device)),
          "fx_emb_seq_pool_fwd")
    return out


def dedup_workspace_bytes(n):
    lib = _lib.load()
    nbytes = lib.fx_dedup_workspace_bytes(n)
    if nbytes == 0:
        check(1, "fx_dedup_workspace_bytes")
    return int(nbytes)


class DedupResult(object):
    """Unique rows of a batch's lookups (device resident; count stays on the device)."""
    __slots__ = ("sorted_key", "sorted_pos", "uniq_row", "seg_start", "n_unique", "n_max", "C",
                 "sorted_uid")

    def __init__(self, n, C_, device, want_uid=False):
        self.sorted_uid = torch.empty(n, dtype=torch.int32, device=device) if want_uid else None
        self.sorted_key = torch.empty(n, dtype=torch.int32, device=device)
        self.sorted_pos = torch.empty(n, dtype=torch.int32, device=device)
        self.uniq_row = torch.empty(n, dtype=torch.int32, device=device)
        self.seg_start = torch.empty(n + 1, dtype=torch.int32, device=device)
        self.n_unique = torch.empty(1, dtype=torch.int32, device=device)   # always written by fx_dedup
        self.n_max = n
        self.C = C_


@_timed("dedup", "sparse_path")
def dedup(ids, col_row_base, col_vocab, col_pad, total_rows, workspace, result=None,
          n_shards=1, want_uid=False, columns_sorted=False, begin_scal=None, grouped=False):
    """grouped: ascending unique rows are not needed (fx_dedup's columns_sorted = 2: the bucketed in-LDS path)."""
    lib = _lib.load()
    B, C_ = ids.shape
    if result is None:
        result = DedupResult(B * C_, C_, ids.device, want_uid=want_uid)
    mode = 0
    if n_shards == 1:
        if columns_sorted and B <= 8192 and C_ <= 256:
            mode = 1
        elif grouped:
            mode = 2
    check(lib.fx_dedup(ptr(ids), ids.stride(0), B, C_, ptr(col_row_base), ptr(col_vocab),
                       ptr(col_pad), total_rows, ptr(workspace), workspace.numel(),
                       ptr(result.sorted_key), ptr(result.sorted_pos), ptr(result.uniq_row),
                       ptr(result.seg_start), ptr(result.n_unique), ptr(result.sorted_uid),
                       n_shards, mode, ptr(begin_scal),
                       stream_ptr(ids.device)),
          "fx_dedup")
    return result


@_timed("dedup_sorted_runs", "sparse_path")
def dedup_sorted_runs(ids, n_runs, vocab, pad, workspace, result=None):
    """De-dup of `n_runs` consecutive ascending runs of ids of one table (rows [0, vocab), `pad`
    marks empty entries at each run's tail): a merge by rank counting, no sort."""
    lib = _lib.load()
    n = ids.numel()
    assert ids.is_contiguous() and n % n_runs == 0
    if result is None:
        result = DedupResult(n, 1, ids.device)
    check(lib.fx_dedup_sorted_runs(ptr(ids), n_runs, n // n_runs, vocab, pad, ptr(workspace),
                                   workspace.numel(), ptr(result.sorted_key),
                                   ptr(result.sorted_pos), ptr(result.uniq_row),
                                   ptr(result.seg_start), ptr(result.n_unique),
                                   ptr(result.sorted_uid), stream_ptr(ids.device)),
          "fx_dedup_sorted_runs")
    return result


def shard_plan_workspace_ints(n_lookups, n_shards):
    return int(_lib.load().fx_shard_plan_workspace_ints(n_lookups, n_shards))


@_timed("shard_plan", "other")
def shard_plan(dd, n_shards, total_rows, cap, send_idx, uniq_slot, lookup_slot, scal,
               global_keys=False, workspace=None, slot_uniq=None):
    """slot_uniq [n_shards * cap] (out, optional): unique index held by every exchange slot, -1 = empty."""
    check(_lib.load().fx_shard_plan(ptr(dd.uniq_row), ptr(dd.n_unique), ptr(dd.sorted_pos),
                                    ptr(dd.sorted_uid), dd.n_max, n_shards, total_rows, cap,
                                    ptr(send_idx), ptr(uniq_slot), ptr(lookup_slot), ptr(scal),
                                    1 if global_keys else 0, ptr(workspace), ptr(slot_uniq),
                                    stream_ptr(send_idx.device)), "fx_shard_plan")


def _gx_arrays(tables):
    """tables: [(tensor or None, D, column offset)] -> host arrays of the exchange-block entry points."""
    n = len(tables)
    ptrs = _lib.ptr_array([t for t, _, _ in tables])
    return ptrs, (C.c_int32 * n)(*[int(d) for _, d, _ in tables]), \
        (C.c_int32 * n)(*[int(o) for _, _, o in tables]), n


@_timed("fill_grad_block", "other")
def fill_grad_block(tables, slot_uniq, block):
    """tables: [(G [n_max, D] or None, D, column offset)]; block [n_slots, ld] is written densely."""
    ptrs, ds, offs, n = _gx_arrays(tables)
    check(_lib.load().fx_fill_grad_block(ptrs, ds, offs, n, ptr(slot_uniq), block.shape[0], ptr(block),
                                         block.stride(0), stream_ptr(block.device)),
          "fx_fill_grad_block")


def owner_grad_reduce_partials(n_max):
    return int(_lib.load().fx_owner_grad_reduce_partials(n_max))


@_timed("owner_grad_reduce", "other")
def owner_grad_reduce(grecv, dd, tables, sq_partials):
    """tables: [(G_out [n_max, D] or None, D, column offset)] of the received block grecv [n, ld]."""
    ptrs, ds, offs, n = _gx_arrays(tables)
    check(_lib.load().fx_owner_grad_reduce(ptr(grecv), grecv.stride(0), ptr(dd.sorted_pos),
                                           ptr(dd.seg_start), ptr(dd.n_unique), dd.n_max, ptrs, ds,
                                           offs, n, ptr(sq_partials), stream_ptr(grecv.device)),
          "fx_owner_grad_reduce")


@_timed("scatter_rows", "other")
def scatter_rows(src, row_map, n_rows, n_max, D, dst):
    """dst: [*, >= D] (a column range of a wider block is fine: its row stride is used)."""
    check(_lib.load().fx_scatter_rows(ptr(src), ptr(row_map), ptr(n_rows), n_max, D, ptr(dst),
                                      dst.stride(0), stream_ptr(dst.device)), "fx_scatter_rows")


@_timed("split_rows", "other")
def split_rows(src, n_rows, parts, zero_tail_rows=0):
    """parts: [(column offset, dst [n_rows + zero_tail_rows, width] contiguous)], one launch."""
    n = len(parts)
    dsts = _lib.ptr_array([d for _, d in parts])
    offs = (C.c_int32 * n)(*[o for o, _ in parts])
    widths = (C.c_int32 * n)(*[d.shape[1] for _, d in parts])
    check(_lib.load().fx_split_rows(ptr(src), src.stride(0), n_rows, n, dsts, offs, widths,
                                    zero_tail_rows, stream_ptr(src.device)), "fx_split_rows")


@_timed("sum_parts", "other")
def sum_parts(parts, out):
    check(_lib.load().fx_sum_parts(_lib.ptr_array(parts), _lib.i64_array([p.numel() for p in parts]),
                                   len(parts), ptr(out), stream_ptr(out.device)), "fx_sum_parts")


def emb_grad_reduce_partials(n_max, D):
    return int(_lib.load().fx_emb_grad_reduce_partials(n_max, D))


def emb_grad_reduce_scratch_ints(n_max):
    return int(_lib.load().fx_emb_grad_reduce_scratch_ints(n_max))


@_timed("emb_grad_reduce", "sparse_path")
def emb_grad_reduce(dout, dout_ld, col_out_off, C_, D, dd, G, sq_partials, scratch,
                    col_denom=None, denom=None):
    """col_denom / denom: per-column index into the [B, n_seq] pooling denominators (mean-pooled
    sequence columns), see fx_emb_grad_reduce_scaled."""
    lib = _lib.load()
    if col_denom is None:
        check(lib.fx_emb_grad_reduce(ptr(dout), dout_ld, ptr(col_out_off), C_, D,
                                     ptr(dd.sorted_pos), ptr(dd.seg_start), ptr(dd.n_unique),
                                     dd.n_max, ptr(G), ptr(sq_partials), ptr(scratch),
                                     stream_ptr(dout.device)), "fx_emb_grad_reduce")
        return
    check(lib.fx_emb_grad_reduce_scaled(ptr(dout), dout_ld, ptr(col_out_off), ptr(col_denom),
                                        ptr(denom), denom.stride(0), C_, D, ptr(dd.sorted_pos),
                                        ptr(dd.seg_start), ptr(dd.n_unique), dd.n_max, ptr(G),
                                        ptr(sq_partials), ptr(scratch), stream_ptr(dout.device)),
          "fx_emb_grad_reduce_scaled")


@_timed("emb_numeric_grad", "other")
def emb_numeric_grad(dout, dout_ld, num_out_off, dense, D, dnum_w):
    lib = _lib.load()
    B, Fd = dense.shape
    ws = torch.empty(_lib.FX_NUMGRAD_CHUNKS * Fd * D, dtype=torch.float32, device=dout.device)
    check(lib.fx_emb_numeric_grad(ptr(dout), dout_ld, ptr(num_out_off), ptr(dense),
                                  dense.stride(0), Fd, D, B, ptr(dnum_w), ptr(ws),
                                  stream_ptr(dout.device)), "fx_emb_numeric_grad")


@_timed("opt_begin_step", "other")
def opt_begin_step(scal):
    check(_lib.load().fx_opt_begin_step(ptr(scal), stream_ptr(scal.device)), "fx_opt_begin_step")


@_timed("clip_coef", "other")
def clip_coef(parts, scal):
    """parts: list of fp32 device tensors holding partial sums of squared gradient norms."""
    lib = _lib.load()
    if len(parts) > _lib.FX_CLIP_MAX_PARTS:
        raise _lib.FxError("too many partial-norm arrays (%d)" % len(parts))
    check(lib.fx_clip_coef(_lib.ptr_array(parts), _lib.i64_array([p.numel() for p in parts]),
                           len(parts), ptr(scal), stream_ptr(scal.device)), "fx_clip_coef")


def reg_stats(x, scal, partials):
    """partials [3 * FX_REG_BLOCKS]: sum p^2 | sum |p| | sum r(p)^2 over the flat tensor x."""
    check(_lib.load().fx_reg_stats(ptr(x), x.numel(), ptr(scal), ptr(partials),
                                   stream_ptr(x.device)), "fx_reg_stats")


def reg_cross(table, D, dd, G, scal, partials):
    check(_lib.load().fx_reg_cross(ptr(table), D, ptr(dd.uniq_row), ptr(dd.n_unique), dd.n_max,
                                   ptr(G), ptr(scal), ptr(partials), stream_ptr(table.device)),
          "fx_reg_cross")


def reg_dense_update(table, m, v, last_step, D, adam, scal):
    check(_lib.load().fx_reg_dense_update(ptr(table), ptr(m), ptr(v), ptr(last_step),
                                          table.shape[0], D, 1 if adam else 0, ptr(scal),
                                          stream_ptr(table.device)), "fx_reg_dense_update")


def _chunks(n):
    i = 0
    while i < n:
        yield i, min(n, i + _lib.FX_MT_MAX)
        i += _lib.FX_MT_MAX


@_timed("mt_sqnorm", "other")
def mt_sqnorm(grads, sq_partials):
    """sq_partials: fp32 [len(grads) * FX_MT_BLOCKS]."""
    lib = _lib.load()
    sizes = [g.numel() for g in grads]
    for a, b in _chunks(len(grads)):
        out = sq_partials[a * _lib.FX_MT_BLOCKS:]
        check(lib.fx_mt_sqnorm(_lib.ptr_array(grads[a:b]), _lib.i64_array(sizes[a:b]), b - a,
                               ptr(out), stream_ptr(sq_partials.device)), "fx_mt_sqnorm")


@_timed("mt_adam", "other")
def mt_adam(params, grads, ms, vs, scal):
    lib = _lib.load()
    sizes = [p.numel() for p in params]
    for a, b in _chunks(len(params)):
        check(lib.fx_mt_adam(_lib.ptr_array(params[a:b]), _lib.ptr_array(grads[a:b]),
                             _lib.ptr_array(ms[a:b]), _lib.ptr_array(vs[a:b]),
                             _lib.i64_array(sizes[a:b]), b - a, ptr(scal),
                             stream_ptr(scal.device)), "fx_mt_adam")


@_timed("mt_sgd", "other")
def mt_sgd(params, grads, scal):
    lib = _lib.load()
    sizes = [p.numel() for p in params]
    for a, b in _chunks(len(params)):
        check(lib.fx_mt_sgd(_lib.ptr_array(params[a:b]), _lib.ptr_array(grads[a:b]),
                            _lib.i64_array(sizes[a:b]), b - a, ptr(scal),
                            stream_ptr(scal.device)), "fx_mt_sgd")


def fm_fwd(emb, F, D, addend, out):
    B = emb.shape[0]
    check(_lib.load().fx_fm_fwd(ptr(emb), emb.stride(0), F, D, ptr(addend), ptr(out), B,
                                stream_ptr(emb.device)), "fx_fm_fwd")
    return out


def fm_bwd(emb, F, D, g, demb, accumulate=False):
    B = emb.shape[0]
    check(_lib.load().fx_fm_bwd(ptr(emb), emb.stride(0), F, D, ptr(g), ptr(demb), demb.stride(0),
                                1 if accumulate else 0, B, stream_ptr(emb.device)), "fx_fm_bwd")
    return demb


@_timed("lr_fwd", "sparse_path")
def lr_fwd(table1, ids, col_row_base, col_vocab, dense, num_w1, bias, out, scal):
    B = out.shape[0]
    C_ = 0 if ids is None else ids.shape[1]
    Fd = 0 if dense is None else dense.shape[1]
    check(_lib.load().fx_lr_fwd(ptr(table1), ptr(ids), 0 if ids is None else ids.stride(0),
                                ptr(col_row_base), ptr(col_vocab), C_, ptr(dense),
                                0 if dense is None else dense.stride(0), ptr(num_w1), Fd,
                                ptr(bias), ptr(out), B, ptr(scal), _row_ld(table1),
                                stream_ptr(out.device)), "fx_lr_fwd")
    return out


def gemm_workspace_floats(M, N, split_k):
    """Floats of split-K workspace for an [M, N] product: split_k slabs of the product + split_k vectors of
    M partial row sums (the fused bias gradient), as include/fxctr.h's fx_gemm_problem comment says
    (ws[split_k * M * N + z * M + m]), + 64 floats of alignment slack."""
    return split_k * M * (N + 1) + 64


def gemm(A, B_, C_, transa=False, transb=False, bias=None, act=0, zout=None, mul=None, mask=None,
         add=None, split_k=1, workspace=None, rowsum=None):
    """C = epilogue(op(A) . op(B)).  A, B, C: 2-D fp32 with unit inner stride."""
    if KernelTimer.recording:
        M_, N_ = C_.shape
        K_ = A.shape[0] if transa else A.shape[1]
        KernelTimer.note("k_gemm_f32", "gemm %dx%dx%d" % (M_, N_, K_), 2.0 * M_ * N_ * K_, _gemm,
                         (A, B_, C_, transa, transb, bias, act, zout, mul, mask, add, split_k,
                          workspace, rowsum), {})
    return _gemm(A, B_, C_, transa, transb, bias, act, zout, mul, mask, add, split_k, workspace,
                 rowsum)


def _epilogue(bias=None, act=0, zout=None, mul=None, mask=None, add=None, rowsum=None):
    epi = _lib.GemmEpilogue()
    epi.bias = bias.data_ptr() if bias is not None else None
    epi.act = act
    if zout is not None:
        epi.zout, epi.ldz = zout.data_ptr(), zout.stride(0)
    if mul is not None:
        epi.mul, epi.ldmul = mul.data_ptr(), mul.stride(0)
    if mask is not None:
        epi.mask, epi.ldmask = mask.data_ptr(), mask.stride(0)
    if add is not None:
        epi.add, epi.ldadd = add.data_ptr(), add.stride(0)
    if rowsum is not None:
        epi.rowsum = rowsum.data_ptr()
    return epi


def gemm_dw_dx(dz, x, W, dW, dx, split_k=1, workspace=None, rowsum=None, mask=None, add=None):
    """The two gradient GEMMs of a Linear / CrossNet layer in ONE launch (fx_gemm_f32_batch):
    dW[N, K] = dz^T x (split-K, `rowsum` = column sums of dz = bias gradient) and
    dx[M, K] = dz W with the `mask` / `add` epilogue.  Same results as the two gemm() calls."""
    if KernelTimer.recording:
        M_, N_ = dz.shape
        K_ = x.shape[1]
        KernelTimer.note("k_gemm_f32", "gemm2 %dx%dx%d" % (M_, N_, K_), 4.0 * M_ * N_ * K_,
                         _gemm_dw_dx, (dz, x, W, dW, dx, split_k, workspace, rowsum, mask, add), {})
    return _gemm_dw_dx(dz, x, W, dW, dx, split_k, workspace, rowsum, mask, add)


class _GemmProblem(object):
    """One GEMM of a batch: keeps the tensors (and the epilogue struct the C struct points at) alive."""

    def __init__(self, A, B_, C_, transa, transb, split_k, workspace, epi, keep):
        M, N = C_.shape
        K = A.shape[0] if transa else A.shape[1]
        self.M, self.N, self.K = M, N, K
        self.epi, self.keep = epi, keep
        self.struct = _lib.GemmProblem(1 if transa else 0, 1 if transb else 0, M, N, K, ptr(A),
                                       A.stride(0), ptr(B_), B_.stride(0), ptr(C_), C_.stride(0),
                                       C.pointer(epi), split_k, ptr(workspace))
        self.device = C_.device


def gemm_problem(A, B_, C_, transa=False, transb=False, bias=None, act=0, zout=None, mul=None,
                 mask=None, add=None, split_k=1, workspace=None, rowsum=None):
    """-> one entry for gemm_batch(); same arguments as gemm().  split_k is the LARGEST number of K slabs
    `workspace` holds (gemm_workspace_floats(M, N, split_k)); the library chooses the actual split."""
    epi = _epilogue(bias, act, zout, mul, mask, add, rowsum)
    return _GemmProblem(A, B_, C_, transa, transb, split_k, workspace, epi,
                        (A, B_, C_, bias, zout, mul, mask, add, workspace, rowsum))


def gemm_batch(problems):
    """Independent GEMMs in as few launches as possible (fx_gemm_f32_batch): up to four aligned problems
    leave as ONE grid on 128-row tiles, two workgroups per CU."""
    if not problems:
        return
    if KernelTimer.recording:
        KernelTimer.note("k_gemm_f32", "gemmN " + "+".join("%dx%dx%d" % (p.M, p.N, p.K) for p in problems),
                         sum(2.0 * p.M * p.N * p.K for p in problems), _gemm_batch, (problems,), {})
    return _gemm_batch(problems)


def _gemm_batch(problems):
    arr = (_lib.GemmProblem * len(problems))()
    for i, p in enumerate(problems):
        arr[i] = p.struct
    check(_lib.load().fx_gemm_f32_batch(arr, len(problems), stream_ptr(problems[0].device)),
          "fx_gemm_f32_batch")


def _gemm_dw_dx(dz, x, W, dW, dx, split_k, workspace, rowsum, mask, add):
    M, N = dz.shape
    K = x.shape[1]
    e1, e2 = _epilogue(rowsum=rowsum), _epilogue(mask=mask, add=add)
    probs = (_lib.GemmProblem * 2)()
    probs[0] = _lib.GemmProblem(1, 0, N, K, M, ptr(dz), dz.stride(0), ptr(x), x.stride(0), ptr(dW),
                                dW.stride(0), C.pointer(e1), split_k, ptr(workspace))
    probs[1] = _lib.GemmProblem(0, 0, M, K, N, ptr(dz), dz.stride(0), ptr(W), W.stride(0), ptr(dx),
                                dx.stride(0), C.pointer(e2), 1, None)
    check(_lib.load().fx_gemm_f32_batch(probs, 2, stream_ptr(dz.device)), "fx_gemm_f32_batch")


def _gemm(A, B_, C_, transa, transb, bias, act, zout, mul, mask, add, split_k, workspace, rowsum):
    lib = _lib.load()
    M, N = C_.shape
    K = A.shape[0] if transa else A.shape[1]
    epi = _epilogue(bias, act, zout, mul, mask, add, rowsum)
    check(lib.fx_gemm_f32(1 if transa else 0, 1 if transb else 0, M, N, K, ptr(A), A.stride(0),
                          ptr(B_), B_.stride(0), ptr(C_), C_.stride(0), C.byref(epi), split_k,
                          ptr(workspace), stream_ptr(C_.device)), "fx_gemm_f32")
    return C_


GEMM_STRATEGIES = ("NONE", "SKINNY", "X6", "PIPE", "PLAIN", "MULTI_X6", "MULTI_F32", "PAIR_BWD", "HEAD_BWD",
                   "PAIR_FWD", "SINGLES")


class GemmStrategy(object):
    """What fx_gemm_last_strategy reports.  strategy: a name of GEMM_STRATEGIES; launches: one dict per
    problem in the caller's order (arm, bm, bn, split_k, tr = 16-byte epilogue, av / bv = 16-byte operand
    loads of the PLAIN arm); swapped: a forward pair ran its second problem first."""

    def __init__(self, rec):
        self.strategy = GEMM_STRATEGIES[rec.strategy]
        self.n_problems = rec.n_problems
        self.swapped = bool(rec.swapped)
        self.launches = [dict(arm=GEMM_STRATEGIES[rec.arm[i]], bm=rec.tile_bm[i], bn=rec.tile_bn[i],
                              split_k=rec.split_k[i], tr=bool(rec.tr[i]), av=bool(rec.plain_vec[i] & 1),
                              bv=bool(rec.plain_vec[i] & 2)) for i in range(rec.n)]

    def __repr__(self):
        return "GemmStrategy(%s, %r%s)" % (self.strategy, self.launches, ", swapped" if self.swapped else "")


def gemm_last_strategy():
    """Which kernels the last gemm() / gemm_dw_dx() / gemm_batch() call of this thread launched
    (fx_gemm_last_strategy).  For tests and diagnosis only: nothing may branch on it."""
    rec = _lib.GemmStrategyRecord()
    _lib.load().fx_gemm_last_strategy(C.byref(rec))
    return GemmStrategy(rec)


@_timed("colsum", "other")
def colsum(X, out, workspace):
    M, N = X.shape
    check(_lib.load().fx_colsum(ptr(X), X.stride(0), M, N, ptr(out), ptr(workspace),
                                stream_ptr(X.device)), "fx_colsum")
    return out


@_timed("mask_mul", "other")
def mask_mul(dy, y, out):
    """dy: [rows, cols] with unit inner stride (a column slice of a wider tensor is read in place)."""
    rows, cols = dy.shape
    check(_lib.load().fx_mask_mul(ptr(dy), dy.stride(0), ptr(y), y.stride(0), ptr(out), rows, cols,
                                  stream_ptr(dy.device)), "fx_mask_mul")
    return out


@_timed("cross_bwd_prep", "other")
def cross_bwd_prep(dxn, x0, z, t, dx0, init, add_dxn):
    rows, cols = dxn.shape
    check(_lib.load().fx_cross_bwd_prep(ptr(dxn), dxn.stride(0), ptr(x0), ptr(z), ptr(t), ptr(dx0),
                                        rows, cols, 1 if init else 0, 1 if add_dxn else 0,
                                        stream_ptr(dxn.device)), "fx_cross_bwd_prep")


@_timed("sigmoid_bce", "other")
def sigmoid_bce(logit, y, prob=None, loss=None, dlogit=None):
    check(_lib.load().fx_sigmoid_bce(ptr(logit), ptr(y), logit.numel(), ptr(prob), ptr(loss),
                                     ptr(dlogit), stream_ptr(logit.device)), "fx_sigmoid_bce")


def head_train_workspace_floats(M, K):
    return int(_lib.load().fx_head_train_workspace(M, K))


def head_train_ok(h, W, out_add=None):
    """The shapes / alignments fx_head_train takes (else the caller keeps the three-kernel path)."""
    K = W.shape[1]
    return (W.shape[0] == 1 and K % 4 == 0 and 8 < K <= 2048 and h.dim() == 2 and h.stride(1) == 1
            and h.stride(0) % 4 == 0 and h.data_ptr() % 16 == 0 and W.is_contiguous()
            and W.data_ptr() % 16 == 0
            and (out_add is None or (out_add.numel() == h.shape[0] and out_add.dim() <= 2)))


@_timed("head_train", "other")
def head_train(h, W, bias, out_add, y, mask_from, root_scale, logit, dlogit, dz, dW, db, loss, workspace):
    """Head forward + sigmoid / BCE + head backward in one pass (fx_head_train).  h: [M, K]; W: [1, K];
    out_add / y / logit / dlogit: M elements; dz: [M, K] or None; dW: [1, K]; db: [1] or None; loss: [];
    mask_from: -1 no ReLU mask on dz, else the first masked column (0: all of them)."""
    M, K = h.shape
    check(_lib.load().fx_head_train(ptr(h), h.stride(0), ptr(W), ptr(bias), ptr(out_add),
                                    (out_add.stride(0) if out_add is not None else 0), ptr(y), M, K,
                                    int(mask_from), float(root_scale), ptr(logit), ptr(dlogit), ptr(dz),
                                    (dz.stride(0) if dz is not None else 0), ptr(dW), ptr(db), ptr(loss),
                                    ptr(workspace), stream_ptr(h.device)), "fx_head_train")


# ---- DIN attention / Dice ---------------------------------------------------------------------
def _k_strides(K):
    """K: [B, L, E] with unit stride in E (a strided view of the gather record is fine)."""
    if K.stride(2) != 1:
        K = K.contiguous()
    return K, K.stride(0), K.stride(1)


def din_concat_fwd(q, K, out):
    K, sb, sl = _k_strides(K)
    B, L, E = K.shape
    check(_lib.load().fx_din_concat_fwd(ptr(q), q.stride(0), ptr(K), sb, sl, B, L, E, ptr(out),
                                        stream_ptr(out.device)), "fx_din_concat_fwd")
    return out


def din_concat_bwd(dx, q, K, dq, dK):
    K, sb, sl = _k_strides(K)
    B, L, E = K.shape
    check(_lib.load().fx_din_concat_bwd(ptr(dx), ptr(q), q.stride(0), ptr(K), sb, sl, B, L, E,
                                        ptr(dq), ptr(dK), dK.stride(0), dK.stride(1), 0,
                                        stream_ptr(dx.device)), "fx_din_concat_bwd")


def din_pool_fwd(w, ids, K, out):
    K, sb, sl = _k_strides(K)
    B, L, E = K.shape
    check(_lib.load().fx_din_pool_fwd(ptr(w), ptr(ids), ids.stride(0), ptr(K), sb, sl, B, L, E,
                                      ptr(out), stream_ptr(out.device)), "fx_din_pool_fwd")
    return out


def din_pool_bwd(w, ids, K, dout, dw, dK):
    K, sb, sl = _k_strides(K)
    B, L, E = K.shape
    check(_lib.load().fx_din_pool_bwd(ptr(w), ptr(ids), ids.stride(0), ptr(K), sb, sl, ptr(dout),
                                      B, L, E, ptr(dw), ptr(dK), dK.stride(0), dK.stride(1),
                                      stream_ptr(dout.device)), "fx_din_pool_bwd")


def dice_workspace_floats(H):
    return int(_lib.load().fx_dice_workspace_floats(H))


def dice_fwd(Z, alpha, eps, momentum, training, running_mean, running_var, stats, Y, workspace):
    N, H = Z.shape
    check(_lib.load().fx_dice_fwd(ptr(Z), N, H, ptr(alpha), eps, momentum, 1 if training else 0,
                                  ptr(running_mean), ptr(running_var), ptr(stats), ptr(Y),
                                  ptr(workspace), stream_ptr(Z.device)), "fx_dice_fwd")
    return Y


def dice_bwd(Z, dY, alpha, eps, training, stats, dZ, dalpha, workspace):
    N, H = Z.shape
    check(_lib.load().fx_dice_bwd(ptr(Z), ptr(dY), N, H, ptr(alpha), eps, 1 if training else 0,
                                  ptr(stats), ptr(dZ), ptr(dalpha), ptr(workspace),
                                  stream_ptr(Z.device)), "fx_dice_bwd")


def dice_local_sums(Z, sums, workspace):
    N, H = Z.shape
    check(_lib.load().fx_dice_local_sums(ptr(Z), N, H, ptr(sums), ptr(workspace),
                                         stream_ptr(Z.device)), "fx_dice_local_sums")


def dice_fwd_from_sums(Z, alpha, eps, momentum, sums, n_total, running_mean, running_var, stats, Y):
    N, H = Z.shape
    check(_lib.load().fx_dice_fwd_from_sums(ptr(Z), N, H, ptr(alpha), eps, momentum, ptr(sums),
                                            n_total, ptr(running_mean), ptr(running_var),
                                            ptr(stats), ptr(Y), stream_ptr(Z.device)),
          "fx_dice_fwd_from_sums")
    return Y


def dice_bwd_local_sums(Z, dY, alpha, eps, stats, sums3, workspace):
    N, H = Z.shape
    check(_lib.load().fx_dice_bwd_local_sums(ptr(Z), ptr(dY), N, H, ptr(alpha), eps, ptr(stats),
                                             ptr(sums3), ptr(workspace), stream_ptr(Z.device)),
          "fx_dice_bwd_local_sums")


def dice_bwd_from_sums(Z, dY, alpha, eps, stats, sums3, n_total, dZ):
    N, H = Z.shape
    check(_lib.load().fx_dice_bwd_from_sums(ptr(Z), ptr(dY), N, H, ptr(alpha), eps, ptr(stats),
                                            ptr(sums3), n_total, ptr(dZ), stream_ptr(Z.device)),
          "fx_dice_bwd_from_sums")


# ---- DIN attention with the attention MLP fused in (fx_din_attn.hip) --------------------------------
DIN_ATTN_MAX_E, DIN_ATTN_MAX_H = 16, 64


def _din_attn_flops(n_eval):
    def work(q, K, W1, *a, **kw):
        B, L, E = K.shape
        return 2.0 * n_eval * B * L * 4 * E * W1.shape[0]
    return work


def din_attn_workspace_floats(B, L, E, H):
    return int(_lib.load().fx_din_attn_workspace_floats(B, L, E, H))


def _din_attn_head(q, K):
    K, sb, sl = _k_strides(K)
    B, L, E = K.shape
    return K, (ptr(q), q.stride(0), ptr(K), sb, sl, B, L, E)


@_timed("din_attn_stats", "din_attention", _din_attn_flops(0))
def din_attn_stats(q, K, W1, b1, sums, workspace, stats=None, momentum=0.0, running_mean=None,
                   running_var=None, num_batches_tracked=None):
    """sums[2H] = [sum h | sum h^2] over the B*L positions, h = W1 [q,k,q-k,q*k] + b1.  stats given (one
    rank): dice_stats_from_sums(training) over these B*L rows rides in the same launch."""
    K, head = _din_attn_head(q, K)
    H = W1.shape[0]
    check(_lib.load().fx_din_attn_stats(*head, ptr(W1), ptr(b1), H,
                                        ptr(sums), ptr(workspace), ptr(stats), momentum,
                                        ptr(running_mean) if stats is not None else None,
                                        ptr(running_var) if stats is not None else None,
                                        ptr(num_batches_tracked) if stats is not None else None,
                                        stream_ptr(q.device)),
          "fx_din_attn_stats")


def dice_stats_from_sums(sums, H, n_total, momentum, training, running_mean, running_var, stats,
                         num_batches_tracked=None):
    """num_batches_tracked (int64[1], training only): += 1 in the same launch."""
    check(_lib.load().fx_dice_stats_from_sums(ptr(sums) if sums is not None else None, H, n_total,
                                              momentum, 1 if training else 0, ptr(running_mean),
                                              ptr(running_var),
                                              ptr(num_batches_tracked) if training else None, ptr(stats),
                                              stream_ptr(stats.device)), "fx_dice_stats_from_sums")


@_timed("din_attn_fwd", "din_attention", _din_attn_flops(1))
def din_attn_fwd(q, K, W1, b1, alpha, eps, stats, W2, b2, mask, a_out, out):
    """a_out[B, L] = attention logits (before the mask), out[B, E] = sum_l a mask k."""
    K, head = _din_attn_head(q, K)
    H = W1.shape[0]
    check(_lib.load().fx_din_attn_fwd(*head, ptr(W1), ptr(b1), H, ptr(alpha), eps, ptr(stats),
                                      ptr(W2), ptr(b2), ptr(mask),
                                      mask.stride(0) if mask is not None else 0, ptr(a_out),
                                      ptr(out), out.stride(0), stream_ptr(q.device)),
          "fx_din_attn_fwd")
    return out


@_timed("din_attn_bwd_sums", "din_attention", _din_attn_flops(0))
def din_attn_bwd_sums(q, K, W1, b1, alpha, eps, stats, W2, mask, dout, da, sums5, workspace):
    """da[B, L] = mask (dout . k);  sums5[5H] = [dalpha | sum dzhat | sum dzhat*zhat | dW2 | db2, 0...]."""
    K, head = _din_attn_head(q, K)
    H = W1.shape[0]
    check(_lib.load().fx_din_attn_bwd_sums(*head, ptr(W1), ptr(b1), H, ptr(alpha), eps, ptr(stats),
                                           ptr(W2), ptr(mask),
                                           mask.stride(0) if mask is not None else 0, ptr(dout),
                                           dout.stride(0), ptr(da), ptr(sums5), ptr(workspace),
                                           stream_ptr(q.device)), "fx_din_attn_bwd_sums")


@_timed("din_attn_bwd", "din_attention", _din_attn_flops(2))
def din_attn_bwd(q, K, W1, b1, alpha, eps, training, stats, W2, mask, a_logit, dout, da, sums5,
                 n_total, dq, dK, dW1b1, workspace, dq_accumulate=False):
    """dq_accumulate: dq += (the rows already hold another share of the target's gradient)."""
    K, head = _din_attn_head(q, K)
    H = W1.shape[0]
    check(_lib.load().fx_din_attn_bwd(*head, ptr(W1), ptr(b1), H, ptr(alpha), eps,
                                      1 if training else 0, ptr(stats), ptr(W2), ptr(mask),
                                      mask.stride(0) if mask is not None else 0, ptr(a_logit),
                                      ptr(dout), dout.stride(0), ptr(da), ptr(sums5), n_total,
                                      ptr(dq), dq.stride(0), 1 if dq_accumulate else 0, ptr(dK),
                                      dK.stride(0), dK.stride(1),
                                      ptr(dW1b1), ptr(workspace), stream_ptr(q.device)),
          "fx_din_attn_bwd")


def dot_interact_fwd(emb, F, D, out, tail=0):
    """out[:, :P] = pairwise dots (rows of out may be wider: out.stride(0)); tail: see fx_dot_interact_fwd."""
    B = emb.shape[0]
    check(_lib.load().fx_dot_interact_fwd(ptr(emb), emb.stride(0), F, D, B, ptr(out), out.stride(0), tail,
                                          stream_ptr(emb.device)), "fx_dot_interact_fwd")
    return out


def dot_interact_bwd(emb, g, F, D, demb, tail=0):
    B = emb.shape[0]
    check(_lib.load().fx_dot_interact_bwd(ptr(emb), emb.stride(0), ptr(g), g.stride(0), tail, F, D, B,
                                          ptr(demb), demb.stride(0), stream_ptr(emb.device)),
          "fx_dot_interact_bwd")
    return demb


# ---- CIN ------------------------------------------------------------------------------------------
# the limits of one fx_cin_fwd / fx_cin_bwd call (include/fxctr.h:640 "Limits", csrc/fx_cin.hip fx_cin_check)
CIN_MAX_W_FLOATS = 30720     # O*F0*Mi + O: the LDS-resident W
CIN_MAX_TILE = 4096          # F0*D, Mi*D and O*D of one call (a sample's staged tiles)
CIN_MAX_D = 256


def cin_chunks(F0, Mi, O):
    """[(o0, o1)]: the output maps of a CIN layer cut into the fewest, equal-as-possible runs whose
    W fits one call (CIN_MAX_W_FLOATS).  A function of (F0, Mi, O) alone."""
    per_call = CIN_MAX_W_FLOATS // (F0 * Mi + 1)
    if per_call < 1:
        raise ValueError("CIN layer: one output map of F0*Mi = %d weights exceeds the %d floats of a call"
                         % (F0 * Mi, CIN_MAX_W_FLOATS))
    n = -(-O // per_call)
    size = -(-O // n)
    return [(o0, min(o0 + size, O)) for o0 in range(0, O, size)]


def cin_workgroups():
    return int(_lib.load().fx_cin_workgroups())


def cin_wimg_floats(F0, Mi, D, O):
    """Floats of the packed LDS images of W the matrix-core CIN kernels copy (0: this shape runs on
    the VALU kernels, no image)."""
    return int(_lib.load().fx_cin_wimg_floats(F0, Mi, D, O))


def cin_pack_w(layers, D):
    """layers: [(W [O, F0*Mi], F0, Mi, w_img)] (<= 4): every W laid out as its kernels' LDS images in ONE
    launch, once per step; cin_fwd / cin_bwd take the w_img."""
    import ctypes as C
    n = len(layers)
    Ws = (C.c_void_p * n)(*[ptr(t[0]) for t in layers])
    imgs = (C.c_void_p * n)(*[ptr(t[3]) for t in layers])
    F0s = (C.c_int32 * n)(*[t[1] for t in layers])
    Mis = (C.c_int32 * n)(*[t[2] for t in layers])
    Os = (C.c_int32 * n)(*[t[0].shape[0] for t in layers])
    check(_lib.load().fx_cin_pack_w(n, Ws, F0s, Mis, D, Os, imgs, stream_ptr(layers[0][0].device)),
          "fx_cin_pack_w")


def _cin_flops(X0, Xi, W, *a, **kw):
    # the compress product of one pass: 2 * O * F0 * Mi * D flops per sample
    return 2.0 * X0.shape[0] * W.shape[0] * X0.shape[1] * Xi.shape[1] * X0.shape[2]


@_timed("cin_fwd", "cin", _cin_flops)
def cin_fwd(X0, Xi, W, bias, Xn, pool, w_img=None):
    """X0 [B,F0,D], Xi [B,Mi,D] contiguous; W [O, F0*Mi]; Xn [B,O,D]; pool: [B,O] view (stride ok)."""
    B, F0, D = X0.shape
    Mi, O = Xi.shape[1], W.shape[0]
    check(_lib.load().fx_cin_fwd(ptr(X0), X0.stride(0), F0, ptr(Xi), Xi.stride(0), Mi, D, ptr(W),
                                 ptr(bias), O, ptr(Xn), ptr(pool),
                                 0 if pool is None else pool.stride(0), B, ptr(w_img),
                                 stream_ptr(X0.device)), "fx_cin_fwd")


@_timed("cin_bwd", "cin", lambda *a, **kw: 2.0 * _cin_flops(*a, **kw))     # dX and dW passes
def cin_bwd(X0, Xi, W, dXn, dpool, dX0, accumulate_dx0, dXi, partial, w_img=None):
    """partial: [G, O*F0*Mi + O] (a column slice of a wider [G, .] buffer is written in place)."""
    B, F0, D = X0.shape
    Mi, O = Xi.shape[1], W.shape[0]
    check(_lib.load().fx_cin_bwd(ptr(X0), X0.stride(0), F0, ptr(Xi), Xi.stride(0), Mi, D, ptr(W), O,
                                 ptr(dXn), ptr(dpool), 0 if dpool is None else dpool.stride(0),
                                 ptr(dX0), dX0.stride(0), 1 if accumulate_dx0 else 0, ptr(dXi),
                                 dXi.stride(0), ptr(partial), partial.stride(0), B, ptr(w_img),
                                 stream_ptr(X0.device)),
          "fx_cin_bwd")


# ---- multi-head self-attention over the fields (AutoInt) -------------------------------------------
MHSA_MAX = 64        # F, D_in, A of fx_mhsa_*


def _mhsa_flops(X, Wq, *a, **kw):
    # per sample: 3 (+1) projections 2 F D A each, scores and P V 2 F F A each
    B, F, D = X.shape
    A = Wq.shape[0]
    return 2.0 * B * F * A * (3 * D + 2 * F)


def mhsa_workspace_floats(B, D_in, A, has_wres):
    return int(_lib.load().fx_mhsa_workspace_floats(B, D_in, A, 1 if has_wres else 0))


def _mhsa_x(X):
    """X [B, F, D] as the kernels address it: unit stride over d, D over f, any sample stride."""
    assert X.dim() == 3 and X.stride(2) == 1 and (X.shape[1] == 1 or X.stride(1) == X.shape[2])
    return X.stride(0) if X.shape[0] > 1 else X.shape[1] * X.shape[2]


@_timed("mhsa_fwd", "mhsa", _mhsa_flops)
def mhsa_fwd(X, Wq, Wk, Wv, Wres, H, use_scale, residual, relu, Y):
    """One self-attention layer: Y [B, F, A] contiguous."""
    _need_cuda(X, "X")
    B, F, D = X.shape
    check(_lib.load().fx_mhsa_fwd(ptr(X), _mhsa_x(X), B, F, D, ptr(Wq), ptr(Wk), ptr(Wv), ptr(Wres),
                                  Wq.shape[0], H, 1 if use_scale else 0, 1 if residual else 0,
                                  1 if relu else 0, ptr(Y), stream_ptr(X.device)), "fx_mhsa_fwd")
    return Y


@_timed("mhsa_bwd", "mhsa", lambda *a, **kw: 3.0 * _mhsa_flops(*a, **kw))   # recompute + dX + dW passes
def mhsa_bwd(X, Wq, Wk, Wv, Wres, H, use_scale, residual, relu, Y, dY, dX, dW, workspace,
             dx_accumulate=False):
    """dX [B, F, D] (sample stride free), dW [3 | 4, A, D] = dWq | dWk | dWv (| dWres); dY contiguous."""
    _need_cuda(X, "X")
    B, F, D = X.shape
    check(_lib.load().fx_mhsa_bwd(ptr(X), _mhsa_x(X), B, F, D, ptr(Wq), ptr(Wk), ptr(Wv), ptr(Wres),
                                  Wq.shape[0], H, 1 if use_scale else 0, 1 if residual else 0,
                                  1 if relu else 0, ptr(Y), ptr(dY), ptr(dX), _mhsa_x(dX),
                                  1 if dx_accumulate else 0, ptr(dW), ptr(workspace),
                                  stream_ptr(X.device)), "fx_mhsa_bwd")
    return dX, dW


# ---- FiBiNET: squeeze-excitation and bilinear interaction -------------------------------------------
BILINEAR_MAX = 64    # F, D (and the excitation's hidden width) of fx_senet_* / fx_bilinear_*
BILINEAR_TYPES = {"field_all": 0, "field_each": 1, "field_interaction": 2}
SENET_ACTS = {"relu": 0, "sigmoid": 1}


def senet_workspace_floats(B, F, R):
    return int(_lib.load().fx_senet_workspace_floats(B, F, R))


def bilinear_workspace_floats(B, F, D):
    return int(_lib.load().fx_bilinear_workspace_floats(B, F, D))


@_timed("senet_fwd", "senet", lambda X, W1, *a, **kw: 4.0 * X.shape[0] * W1.numel())
def senet_fwd(X, W1, W2, act, A, V=None):
    """A [B, F] = act(W2 relu(W1 mean_d X)); V [B, F, D] = X * A[:, :, None] only when a tensor is given."""
    _need_cuda(X, "X")
    B, F, D = X.shape
    check(_lib.load().fx_senet_fwd(ptr(X), _mhsa_x(X), B, F, D, ptr(W1), ptr(W2), W1.shape[0], act, ptr(A),
                                   ptr(V), stream_ptr(X.device)), "fx_senet_fwd")
    return A


@_timed("senet_bwd", "senet", lambda X, W1, *a, **kw: 12.0 * X.shape[0] * W1.numel())
def senet_bwd(X, W1, W2, act, A, dA, dV, dX, dW1, dW2, workspace, dx_accumulate=False):
    """From dA [B, F] and / or dV [B, F, D] (None: absent): dX (sample stride free), dW1 [R, F], dW2 [F, R]."""
    _need_cuda(X, "X")
    B, F, D = X.shape
    check(_lib.load().fx_senet_bwd(ptr(X), _mhsa_x(X), B, F, D, ptr(W1), ptr(W2), W1.shape[0], act, ptr(A),
                                   ptr(dA), ptr(dV), ptr(dX), _mhsa_x(dX), 1 if dx_accumulate else 0,
                                   ptr(dW1), ptr(dW2), ptr(workspace), stream_ptr(X.device)), "fx_senet_bwd")
    return dX, dW1, dW2


def _bilinear_flops(X, *a, **kw):
    B, F, D = X.shape
    return 2.0 * B * (F * (F - 1) // 2) * D * D


def _rows(buf):
    """A [B, n] buffer as the kernels address it: unit stride over the columns, any row stride."""
    assert buf.dim() == 2 and buf.stride(1) == 1
    return buf.stride(0) if buf.shape[0] > 1 else buf.shape[1]


@_timed("bilinear_fwd", "bilinear", _bilinear_flops)
def bilinear_fwd(X, W, kind, A, out, out_col=0):
    """out[:, out_col : out_col + P*D] = the bilinear interaction of A[:, :, None] * X (A None: of X), pairs in
    triu order; `out` is a [B, >= out_col + P*D] buffer that other columns may share."""
    _need_cuda(X, "X")
    B, F, D = X.shape
    assert out.shape[0] == B and out.shape[1] >= out_col + (F * (F - 1) // 2) * D
    check(_lib.load().fx_bilinear_fwd(ptr(X), _mhsa_x(X), B, F, D, ptr(W), kind, ptr(A), ptr(out), _rows(out),
                                      out_col, stream_ptr(X.device)), "fx_bilinear_fwd")
    return out


@_timed("bilinear_bwd", "bilinear", lambda *a, **kw: 3.0 * _bilinear_flops(*a, **kw))
def bilinear_bwd(X, W, kind, A, dOut, dX, dA, dW, workspace, dout_col=0, dx_accumulate=False):
    """dOut in the layout of the forward's `out`; dX (sample stride free), dA [B, F] (with A), dW like W."""
    _need_cuda(X, "X")
    B, F, D = X.shape
    assert dOut.shape[0] == B and dOut.shape[1] >= dout_col + (F * (F - 1) // 2) * D
    check(_lib.load().fx_bilinear_bwd(ptr(X), _mhsa_x(X), B, F, D, ptr(W), kind, ptr(A), ptr(dOut), _rows(dOut),
                                      dout_col, ptr(dX), _mhsa_x(dX), 1 if dx_accumulate else 0, ptr(dA),
                                      ptr(dW), ptr(workspace), stream_ptr(X.device)), "fx_bilinear_bwd")
    return dX, dA, dW


# ---- MaskNet: grouped LayerNorm (+ ReLU) and the mask's gradient toward V_hidden --------------------
LAYERNORM_MAX_N = 8192    # elements of one normalised group
LAYERNORM_MAX_G = 64      # groups per row (fields of emb_norm)


def layernorm_check(G, N, who="layernorm"):
    """The limits of fx_layernorm_*, raised here before anything is launched."""
    if not 1 <= N <= LAYERNORM_MAX_N:
        raise NotImplementedError("{}: N={}, the kernel's limit is 1 <= N <= {}".format(who, N, LAYERNORM_MAX_N))
    if not 1 <= G <= LAYERNORM_MAX_G:
        raise NotImplementedError("{}: G={}, the kernel's limit is 1 <= G <= {}".format(who, G, LAYERNORM_MAX_G))


def layernorm_workspace_floats(rows, G, N):
    return int(_lib.load().fx_layernorm_workspace_floats(rows, G, N))


def _ln_bytes_fwd(X, G, N, *a, **kw):
    return 4.0 * (2.0 * X.shape[0] * G * N + 2.0 * G * N + 2.0 * X.shape[0] * G)     # x, y; gamma, beta; stats


def _ln_bytes_bwd(X, G, N, gamma, relu, *a, **kw):
    # x and dY twice (dX pass, dgamma / dbeta pass), Y's sign twice with the ReLU, dX once
    return 4.0 * X.shape[0] * G * N * (5.0 + (2.0 if relu else 0.0) + (1.0 if kw.get("dx_accumulate") else 0.0))


@_timed("layernorm_fwd", "layernorm", _ln_bytes_fwd)
def layernorm_fwd(X, G, N, gamma, beta, eps, relu, Y, stats, y_col=0):
    """Y[:, y_col : y_col + G*N] = LayerNorm over every one of the G groups of N columns of X[:, :G*N] (+ ReLU);
    X, Y: [rows, >= ...] with unit column stride and any row stride; gamma, beta: G*N floats; stats: rows*G*2."""
    _need_cuda(X, "X")
    layernorm_check(G, N)
    assert X.shape[1] >= G * N and Y.shape[0] == X.shape[0] and Y.shape[1] >= y_col + G * N
    assert gamma.is_contiguous() and beta.is_contiguous() and gamma.numel() == G * N == beta.numel()
    check(_lib.load().fx_layernorm_fwd(ptr(X), _rows(X), X.shape[0], G, N, ptr(gamma), ptr(beta), eps,
                                       1 if relu else 0, ptr(Y), _rows(Y), y_col, ptr(stats),
                                       stream_ptr(X.device)), "fx_layernorm_fwd")
    return Y


@_timed("layernorm_bwd", "layernorm", _ln_bytes_bwd)
def layernorm_bwd(X, G, N, gamma, relu, Y, stats, dY, dX, dgamma, dbeta, workspace, y_col=0, dy_col=0,
                  dx_accumulate=False):
    """dY in the layout of the forward's Y (its own column offset); dX [rows, >= G*N] (any row stride, added to
    when dx_accumulate); dgamma, dbeta: G*N floats.  Y (None without the ReLU) is read for its sign."""
    _need_cuda(X, "X")
    layernorm_check(G, N)
    assert dY.shape[0] == X.shape[0] and dY.shape[1] >= dy_col + G * N and dX.shape[1] >= G * N
    assert dgamma.is_contiguous() and dbeta.is_contiguous() and gamma.is_contiguous()
    check(_lib.load().fx_layernorm_bwd(ptr(X), _rows(X), X.shape[0], G, N, ptr(gamma), 1 if relu else 0,
                                       ptr(Y) if relu else None, _rows(Y) if relu else 0, y_col, ptr(stats),
                                       ptr(dY), _rows(dY), dy_col, ptr(dX), _rows(dX),
                                       1 if dx_accumulate else 0, ptr(dgamma), ptr(dbeta), ptr(workspace),
                                       stream_ptr(X.device)), "fx_layernorm_bwd")
    return dX, dgamma, dbeta


@_timed("mask_grad", "layernorm", lambda dM, Vmask, H, nb, out, **kw: 4.0 * dM.shape[0] * H * (2.0 * nb + 1.0))
def mask_grad(dM, Vmask, H, nb, out, accumulate=False):
    """out[:, :H] (+)= sum_k dM[:, k*H:(k+1)*H] * Vmask[:, k*H:(k+1)*H]; every tensor [rows, >= ...] with unit
    column stride and any row stride."""
    _need_cuda(dM, "dM")
    assert dM.shape[1] >= nb * H and Vmask.shape[1] >= nb * H and out.shape[1] >= H
    check(_lib.load().fx_mask_grad(ptr(dM), _rows(dM), ptr(Vmask), _rows(Vmask), dM.shape[0], H, nb, ptr(out),
                                   _rows(out), 1 if accumulate else 0, stream_ptr(dM.device)), "fx_mask_grad")
    return out


# ---- FinalMLP: the two feature gates and the aggregation head ---------------------------------------
def finalmlp_slab_rows(B):
    """Rows of one slab of the backward kernels' sums over the batch."""
    return int(_lib.load().fx_finalmlp_slab_rows(B))


def gate2_workspace_floats(B, W):
    return int(_lib.load().fx_gate2_workspace_floats(B, W))


def biagg_workspace_floats(B, dx, dy):
    return int(_lib.load().fx_biagg_workspace_floats(B, dx, dy))


def _gate_ld(Z, B):
    """Row stride of a gate's Z / dZ: 0 for the one row of a gate without context features."""
    assert Z.dim() == 2 and Z.stride(1) == 1 and Z.shape[0] in (1, B)
    return 0 if (Z.shape[0] == 1 and B > 1) else _rows(Z)


def _gate_bytes_fwd(E, Z1, Z2, *a, **kw):
    B, W = E.shape
    n = 1 if Z2 is None else 2
    return 4.0 * (B * W * (1.0 + n) + sum(z.numel() for z in (Z1, Z2) if z is not None))     # E, F; Z


def _gate_bytes_bwd(dF1, dF2, E, Z1, Z2, *a, **kw):
    B, W = E.shape
    n = 1 if Z2 is None else 2
    per = sum(z.shape[0] == B and B > 1 for z in (Z1, Z2) if z is not None)     # Z read, dZ written
    return 4.0 * B * W * (2.0 + n + 2.0 * per + (1.0 if kw.get("de_accumulate") else 0.0))   # E, dE; dF


@_timed("gate2_fwd", "finalmlp", _gate_bytes_fwd)
def gate2_fwd(E, Z1, Z2, F1, F2):
    """F1 = E * 2 sigmoid(Z1), F2 = E * 2 sigmoid(Z2) (Z2 None: one gate).  E, F: [B, W] with unit column stride
    and any row stride; Z: [B, W] or [1, W] (one row for every sample)."""
    _need_cuda(E, "E")
    B, W = E.shape
    assert Z1.shape[1] == W and tuple(F1.shape) == (B, W)
    assert Z2 is None or (Z2.shape[1] == W and tuple(F2.shape) == (B, W))
    two = Z2 is not None
    check(_lib.load().fx_gate2_fwd(ptr(E), _rows(E), B, W, ptr(Z1), _gate_ld(Z1, B), ptr(Z2) if two else None,
                                   _gate_ld(Z2, B) if two else 0, ptr(F1), _rows(F1), ptr(F2) if two else None,
                                   _rows(F2) if two else 0, stream_ptr(E.device)), "fx_gate2_fwd")
    return F1, F2


@_timed("gate2_bwd", "finalmlp", _gate_bytes_bwd)
def gate2_bwd(dF1, dF2, E, Z1, Z2, dE, dZ1, dZ2, workspace, de_accumulate=False):
    """dE (+)= dF1 * 2 sigma(Z1) + dF2 * 2 sigma(Z2); dZi in the shape of Zi (a [1, W] gate's summed over the
    batch through `workspace`, gate2_workspace_floats(B, W) floats)."""
    _need_cuda(E, "E")
    B, W = E.shape
    two = Z2 is not None
    assert tuple(dF1.shape) == (B, W) and tuple(dE.shape) == (B, W) and dZ1.shape == Z1.shape
    assert not two or (tuple(dF2.shape) == (B, W) and dZ2.shape == Z2.shape)
    check(_lib.load().fx_gate2_bwd(ptr(dF1), _rows(dF1), ptr(dF2) if two else None, _rows(dF2) if two else 0,
                                   ptr(E), _rows(E), B, W, ptr(Z1), _gate_ld(Z1, B), ptr(Z2) if two else None,
                                   _gate_ld(Z2, B) if two else 0, ptr(dE), _rows(dE), 1 if de_accumulate else 0,
                                   ptr(dZ1), _gate_ld(dZ1, B), ptr(dZ2) if two else None,
                                   _gate_ld(dZ2, B) if two else 0, ptr(workspace), stream_ptr(E.device)),
          "fx_gate2_bwd")
    return dE, dZ1, dZ2


@_timed("biagg_fwd", "finalmlp", lambda X, Y, *a, **kw: 4.0 * X.shape[0] * (X.shape[1] + 2.0 * Y.shape[1] + 1.0))
def biagg_fwd(X, Y, T, w_x, w_y, b_x, b_y, out_add, out):
    """out[b] = b_x + b_y + X[b] . w_x + Y[b] . (w_y + T[b]) (+ out_add[b]).  X [B, dx], Y and T [B, dy] with unit
    column stride and any row stride; w_x, w_y contiguous; b_x, b_y one float each or None; out, out_add: B
    contiguous floats."""
    _need_cuda(X, "X")
    B, dx = X.shape
    dy = Y.shape[1]
    assert Y.shape[0] == B and tuple(T.shape) == (B, dy) and out.numel() == B and out.is_contiguous()
    assert w_x.is_contiguous() and w_y.is_contiguous() and w_x.numel() == dx and w_y.numel() == dy
    assert out_add is None or (out_add.numel() == B and out_add.is_contiguous())
    check(_lib.load().fx_biagg_fwd(ptr(X), _rows(X), ptr(Y), _rows(Y), ptr(T), _rows(T), B, dx, dy, ptr(w_x),
                                   ptr(w_y), ptr(b_x), ptr(b_y), ptr(out_add), ptr(out), stream_ptr(X.device)),
          "fx_biagg_fwd")
    return out


@_timed("biagg_bwd", "finalmlp",
        lambda g, X, Y, T, w_x, w_y, dT, dY, dXr, *a, **kw:
        4.0 * X.shape[0] * (X.shape[1] * (1.0 if dXr is None else 2.0) + 4.0 * Y.shape[1] + 1.0))
def biagg_bwd(g, X, Y, T, w_x, w_y, dT, dY, dXr, dw_x, dw_y, db, workspace):
    """From g = dout [B]: dT = g * Y, dY = g * (w_y + T), dXr = g w_x^T (None: not wanted), dw_x = X^T g,
    dw_y = Y^T g, db[0] = db[1] = sum g.  workspace: biagg_workspace_floats(B, dx, dy) floats."""
    _need_cuda(X, "X")
    B, dx = X.shape
    dy = Y.shape[1]
    assert g.numel() == B and g.is_contiguous() and tuple(dT.shape) == (B, dy) and tuple(dY.shape) == (B, dy)
    assert dXr is None or tuple(dXr.shape) == (B, dx)
    assert dw_x.is_contiguous() and dw_y.is_contiguous() and dw_x.numel() == dx and dw_y.numel() == dy
    assert db.is_contiguous() and db.numel() == 2
    check(_lib.load().fx_biagg_bwd(ptr(g), ptr(X), _rows(X), ptr(Y), _rows(Y), ptr(T), _rows(T), B, dx, dy,
                                   ptr(w_x), ptr(w_y), ptr(dT), _rows(dT), ptr(dY), _rows(dY), ptr(dXr),
                                   _rows(dXr) if dXr is not None else 0, ptr(dw_x), ptr(dw_y), ptr(db),
                                   ptr(workspace), stream_ptr(X.device)), "fx_biagg_bwd")
    return dT, dY, dXr, dw_x, dw_y, db


# ---- GDCN: the element-wise half of the gated cross layer ----------------------------------------------
def gate_cross_tile_rows():
    """Rows of one workgroup's tile in the two kernels."""
    return int(_lib.load().fx_gate_cross_tile_rows())


@_timed("gate_cross_fwd", "gatecross", lambda h, *a, **kw: 4.0 * h.shape[0] * (h.shape[1] // 2) * 5.0)   # h, x0, xi; xn
def gate_cross_fwd(h, x0, xi, b, xn):
    """xn = x0 * (h[:, :cols] + b) * sigmoid(h[:, cols:]) + xi.  h: [rows, 2 cols]; x0, xi, xn: [rows, cols]; unit
    column stride and any row stride each (xn may be a column range of a wider buffer)."""
    _need_cuda(h, "h")
    rows, cols = x0.shape
    assert tuple(h.shape) == (rows, 2 * cols) and tuple(xi.shape) == (rows, cols) and tuple(xn.shape) == (rows, cols)
    assert b.numel() == cols and b.is_contiguous()
    check(_lib.load().fx_gate_cross_fwd(ptr(h), _rows(h), ptr(x0), _rows(x0), ptr(xi), _rows(xi), ptr(b), ptr(xn),
                                        _rows(xn), rows, cols, stream_ptr(h.device)), "fx_gate_cross_fwd")
    return xn


@_timed("gate_cross_bwd", "gatecross",
        lambda dxn, h, x0, b, dh, dx0, init, add_dxn:                       # dxn, h, x0; dh, dx0 (read when added to)
        4.0 * h.shape[0] * (h.shape[1] // 2) * (7.0 if init else 8.0))
def gate_cross_bwd(dxn, h, x0, b, dh, dx0, init, add_dxn):
    """With u = h[:, :cols] + b and g = sigmoid(h[:, cols:]): dh[:, :cols] = dxn * x0 * g, dh[:, cols:] =
    dxn * x0 * u * g * (1 - g), dx0 (= when init, += otherwise) dxn * u * g (+ dxn when add_dxn).  dxn is read in
    place through its row stride (a column slice of a wider gradient)."""
    _need_cuda(h, "h")
    rows, cols = x0.shape
    assert tuple(h.shape) == (rows, 2 * cols) and tuple(dh.shape) == (rows, 2 * cols)
    assert tuple(dxn.shape) == (rows, cols) and tuple(dx0.shape) == (rows, cols)
    assert b.numel() == cols and b.is_contiguous()
    check(_lib.load().fx_gate_cross_bwd(ptr(dxn), _rows(dxn), ptr(h), _rows(h), ptr(x0), _rows(x0), ptr(b), ptr(dh),
                                        _rows(dh), ptr(dx0), _rows(dx0), rows, cols, 1 if init else 0,
                                        1 if add_dxn else 0, stream_ptr(h.device)), "fx_gate_cross_bwd")
    return dh, dx0


# ---- DCN: the rank-1 cross network, the whole stack per call ---------------------------------------------
def cross_net_limits():
    """The native envelope of cross_net_fwd / cross_net_bwd and their geometry, stated once: cols <= max_cols,
    1 <= L <= max_layers; a workgroup owns tile_rows rows at a time and at most max_wg workgroups stride over the
    row tiles."""
    lim = (C.c_int32 * 4)()
    _lib.load().fx_cross_net_limits(lim)
    return dict(zip(("max_cols", "max_layers", "tile_rows", "max_wg"), (int(v) for v in lim)))


def cross_net_workspace_floats(rows, cols, L):
    return int(_lib.load().fx_cross_net_workspace_floats(rows, cols, L))


def _cross_net_wb(w, b, cols):
    L = w.shape[0]
    assert w.dim() == 2 and tuple(w.shape) == (L, cols) and tuple(b.shape) == (L, cols), \
        "w / b must be [L, %d], got %s / %s" % (cols, tuple(w.shape), tuple(b.shape))
    assert w.is_contiguous() and b.is_contiguous()
    return L


@_timed("cross_net_fwd", "crossnet", lambda x0, *a, **kw: 4.0 * x0.shape[0] * x0.shape[1] * 2.0)     # x0; out
def cross_net_fwd(x0, w, b, out, s=None):
    """out = x_L of x_{l+1} = x_l + ((w_l . x_l) * x_0 + b_l), l < L, in one launch.  x0, out: [rows, cols], unit
    column stride and any row stride each (out may be the left column range of a wider buffer); w, b: [L, cols]
    contiguous; s: [rows, L] contiguous, receives w_l . x_l for the backward (None: not wanted)."""
    _need_cuda(x0, "x0")
    rows, cols = x0.shape
    L = _cross_net_wb(w, b, cols)
    assert tuple(out.shape) == (rows, cols)
    assert s is None or (tuple(s.shape) == (rows, L) and s.is_contiguous())
    check(_lib.load().fx_cross_net_fwd(ptr(x0), _rows(x0), ptr(w), ptr(b), ptr(out), _rows(out), ptr(s), rows, cols,
                                       L, stream_ptr(x0.device)), "fx_cross_net_fwd")
    return out


@_timed("cross_net_bwd", "crossnet",
        lambda dout, x0, w, b, s, dx0, dw, db, init, workspace:                 # dout, x0; dx0 (read when added to)
        4.0 * x0.shape[0] * x0.shape[1] * (3.0 if init else 4.0))
def cross_net_bwd(dout, x0, w, b, s, dx0, dw, db, init, workspace):
    """From dout = dL/dx_L and the forward's s: dx0 (= when init, += otherwise), dw and db [L, cols], in two launches;
    x_l is recomputed from x0, s and b.  dout is read in place through its row stride (a column slice of a wider
    gradient).  workspace: cross_net_workspace_floats(rows, cols, L) floats."""
    _need_cuda(x0, "x0")
    rows, cols = x0.shape
    L = _cross_net_wb(w, b, cols)
    assert tuple(dout.shape) == (rows, cols) and tuple(dx0.shape) == (rows, cols)
    assert tuple(s.shape) == (rows, L) and s.is_contiguous()
    assert tuple(dw.shape) == (L, cols) and tuple(db.shape) == (L, cols) and dw.is_contiguous() and db.is_contiguous()
    assert workspace.is_contiguous() and workspace.numel() >= cross_net_workspace_floats(rows, cols, L)
    check(_lib.load().fx_cross_net_bwd(ptr(dout), _rows(dout), ptr(x0), _rows(x0), ptr(w), ptr(b), ptr(s), ptr(dx0),
                                       _rows(dx0), ptr(dw), ptr(db), ptr(workspace), rows, cols, L,
                                       1 if init else 0, stream_ptr(x0.device)), "fx_cross_net_bwd")
    return dx0, dw, db


# ---- AFM: pairwise attention over the gather record ---------------------------------------------------
def afm_attn_limits():
    """The native envelope of afm_attn_fwd / afm_attn_bwd, stated once: F >= F_min, F * D <= FD_max,
    F (F - 1) / 2 <= P_max, D <= D_max, A <= A_max."""
    lim = (C.c_int32 * 5)()
    _lib.load().fx_afm_attn_limits(lim)
    return dict(zip(("F_min", "FD_max", "P_max", "D_max", "A_max"), (int(v) for v in lim)))


def afm_attn_in_envelope(F, D, A):
    lim = afm_attn_limits()
    return (F >= lim["F_min"] and F * D <= lim["FD_max"] and F * (F - 1) // 2 <= lim["P_max"]
            and 1 <= D <= lim["D_max"] and 1 <= A <= lim["A_max"])


def afm_attn_tile_rows(F=2, D=1, A=1):
    """Samples one workgroup owns at a time (one wave each): 4, fewer for a shape whose backward image would not
    fit the LDS with 4."""
    return int(_lib.load().fx_afm_attn_tile_rows(F, D, A))


def afm_attn_workspace_floats(B, F, D, A):
    """Floats of afm_attn_bwd's workspace: the per-workgroup rows of weight gradient + the reduce's own."""
    return int(_lib.load().fx_afm_attn_workspace_floats(B, F, D, A))


def afm_attn_grad_floats(D, A):
    """grads of afm_attn_bwd: [dW1 (A * D) | db1 (A) | dw2 (A) | dwp (D)]."""
    return A * D + 2 * A + D


def _afm_flops(rec, F, D, W1, *a, **kw):
    return 2.0 * rec.shape[0] * (F * (F - 1) // 2) * D * W1.shape[0]       # the hidden product E W1^T


def _afm_check(rec, F, D, W1, b1, w2, wp):
    _need_cuda(rec, "rec")
    A = W1.shape[0]
    assert rec.dim() == 2 and rec.shape[1] == F * D and rec.stride(1) == 1 and rec.dtype == torch.float32
    assert afm_attn_in_envelope(F, D, A), "afm_attn: F %d, D %d, A %d outside %s" % (F, D, A, afm_attn_limits())
    assert tuple(W1.shape) == (A, D) and W1.is_contiguous()
    assert b1.numel() == A and w2.numel() == A and wp.numel() == D
    assert b1.is_contiguous() and w2.is_contiguous() and wp.is_contiguous()
    return rec.shape[0], A


@_timed("afm_attn_fwd", "afm", _afm_flops)
def afm_attn_fwd(rec, F, D, W1, b1, w2, wp, addend, out, stats):
    """out [B, 1] = sum_p softmax_p(w2 . relu(W1 e_p + b1)) (wp . e_p) (+ addend [B, 1]), e_p = x_i * x_j over the
    pairs i < j of the sample's F fields; rec: [B, F * D] with unit column stride and any row stride.  stats [B, 3]:
    the softmax's max and denominator and the result without the addend, for afm_attn_bwd."""
    B, A = _afm_check(rec, F, D, W1, b1, w2, wp)
    assert out.numel() == B and out.is_contiguous() and tuple(stats.shape) == (B, 3) and stats.is_contiguous()
    assert addend is None or (addend.numel() == B and addend.is_contiguous())
    check(_lib.load().fx_afm_attn_fwd(ptr(rec), _rows(rec), B, F, D, ptr(W1), ptr(b1), ptr(w2), ptr(wp), A,
                                      ptr(addend), ptr(out), ptr(stats), stream_ptr(rec.device)), "fx_afm_attn_fwd")
    return out, stats


@_timed("afm_attn_bwd", "afm", lambda g, rec, F, D, W1, *a, **kw: 3.0 * _afm_flops(rec, F, D, W1))
def afm_attn_bwd(g, rec, F, D, W1, b1, w2, wp, stats, drec, grads, workspace):
    """From g = dout [B, 1] and the forward's stats: drec [B, F * D] (own row stride) and grads
    [afm_attn_grad_floats(D, A)] = [dW1 | db1 | dw2 | dwp] summed over the batch (per-workgroup partial rows in
    workspace, then the fixed-order column sums).  workspace: afm_attn_workspace_floats(B, F, D, A) floats."""
    B, A = _afm_check(rec, F, D, W1, b1, w2, wp)
    assert g.numel() == B and g.is_contiguous() and tuple(stats.shape) == (B, 3) and stats.is_contiguous()
    assert tuple(drec.shape) == (B, F * D) and drec.stride(1) == 1
    assert grads.numel() == afm_attn_grad_floats(D, A) and grads.is_contiguous()
    assert workspace.numel() >= afm_attn_workspace_floats(B, F, D, A) and workspace.is_contiguous()
    check(_lib.load().fx_afm_attn_bwd(ptr(g), ptr(rec), _rows(rec), B, F, D, ptr(W1), ptr(b1), ptr(w2), ptr(wp), A,
                                      ptr(stats), ptr(drec), _rows(drec), ptr(grads), ptr(workspace),
                                      stream_ptr(rec.device)), "fx_afm_attn_bwd")
    return drec, grads


# ---- FwFM / FmFM: the field-pair interaction with a parameter per pair ---------------------------------
PAIRFM_MODES = {"scalar": 0, "vector": 1, "matrix": 2}


def pairfm_limits():
    """The native envelope of pairfm_fwd / pairfm_bwd, stated once: F >= F_min, F * D <= FD_max, D <= D_max."""
    lim = (C.c_int32 * 3)()
    _lib.load().fx_pairfm_limits(lim)
    return dict(zip(("F_min", "FD_max", "D_max"), (int(v) for v in lim)))


def pairfm_in_envelope(F, D):
    lim = pairfm_limits()
    return F >= lim["F_min"] and F * D <= lim["FD_max"] and 1 <= D <= lim["D_max"]


def pairfm_tile_rows(mode="matrix", F=2, D=1):
    """Samples one workgroup owns at a time: 16, 8 for a record too wide for 16 of them in the LDS."""
    return int(_lib.load().fx_pairfm_tile_rows(PAIRFM_MODES[mode], F, D))


def pairfm_workspace_floats(mode, B, F, D):
    """Floats of pairfm_bwd's workspace: one row of weight gradient per slab of samples + the reduce's own (a
    single slab writes straight into grads)."""
    return int(_lib.load().fx_pairfm_workspace_floats(PAIRFM_MODES[mode], B, F, D))


def pairfm_weight_floats(mode, F, D):
    P = F * (F - 1) // 2
    return P * (D * D if mode == "matrix" else D if mode == "vector" else 1)


def pairfm_grad_floats(mode, F, D, wlin=False, bias=False):
    """grads of pairfm_bwd: [dW | dwlin (F * D, with wlin) | dbias (1, with bias)]."""
    return pairfm_weight_floats(mode, F, D) + (F * D if wlin else 0) + (1 if bias else 0)


def _pairfm_flops(rec, F, D, mode, *a, **kw):
    return 2.0 * rec.shape[0] * pairfm_weight_floats(mode, F, D) + 2.0 * rec.shape[0] * (F * (F - 1) // 2) * D


def _pairfm_check(rec, F, D, mode, W, wlin):
    _need_cuda(rec, "rec")
    assert mode in PAIRFM_MODES, mode
    assert rec.dim() == 2 and rec.shape[1] == F * D and rec.stride(1) == 1 and rec.dtype == torch.float32
    assert W.numel() == pairfm_weight_floats(mode, F, D) and W.is_contiguous() and W.dtype == torch.float32
    assert wlin is None or (wlin.numel() == F * D and wlin.is_contiguous())
    return rec.shape[0]


@_timed("pairfm_fwd", "pairfm", _pairfm_flops)
def pairfm_fwd(rec, F, D, mode, W, wlin, bias, addend, out):
    """out [B, 1] = sum_p u_p(x_i) . x_j (+ wlin . x) (+ bias) (+ addend [B, 1]) over the pairs i < j of the sample's
    F fields, u_p(x) = r_p x ("scalar", W [P]), w_p * x ("vector", W [P, D]) or x^T M_p ("matrix", W [P, D, D]);
    rec: [B, F * D] with unit column stride and any row stride.  A shape outside pairfm_limits() is the library's
    invalid-argument error."""
    B = _pairfm_check(rec, F, D, mode, W, wlin)
    assert out.numel() == B and out.is_contiguous()
    assert bias is None or bias.numel() == 1
    assert addend is None or (addend.numel() == B and addend.is_contiguous())
    check(_lib.load().fx_pairfm_fwd(ptr(rec), _rows(rec), B, F, D, PAIRFM_MODES[mode], ptr(W), ptr(wlin), ptr(bias),
                                    ptr(addend), ptr(out), stream_ptr(rec.device)), "fx_pairfm_fwd")
    return out


@_timed("pairfm_bwd", "pairfm", lambda g, rec, F, D, mode, *a, **kw: 3.0 * _pairfm_flops(rec, F, D, mode))
def pairfm_bwd(g, rec, F, D, mode, W, wlin, has_bias, drec, grads, workspace):
    """From g = dout [B, 1]: drec [B, F * D] (own row stride) and grads [pairfm_grad_floats(..)] = [dW | dwlin |
    dbias] summed over the batch in a fixed order (per-slab rows in workspace, then the column sums).  workspace:
    pairfm_workspace_floats(mode, B, F, D) floats."""
    B = _pairfm_check(rec, F, D, mode, W, wlin)
    assert g.numel() == B and g.is_contiguous()
    assert tuple(drec.shape) == (B, F * D) and drec.stride(1) == 1
    assert grads.numel() == pairfm_grad_floats(mode, F, D, wlin is not None, has_bias) and grads.is_contiguous()
    assert workspace.numel() >= pairfm_workspace_floats(mode, B, F, D) and workspace.is_contiguous()
    check(_lib.load().fx_pairfm_bwd(ptr(g), ptr(rec), _rows(rec), B, F, D, PAIRFM_MODES[mode], ptr(W), ptr(wlin),
                                    1 if has_bias else 0, ptr(drec), _rows(drec), ptr(grads), ptr(workspace),
                                    stream_ptr(rec.device)), "fx_pairfm_bwd")
    return drec, grads


# ---- BST: one fused transformer block over the positions of a sample --------------------------------
BST_MAX = 64         # L1 = history + target positions, and dm of fx_bst_block_*
BST_MAX_PARTS = 3
BST_POOLS = {"none": 0, "concat": 0, "mean": 1, "sum": 2, "target": 3}
# the order of fx_bst_weights and of the parameter gradients' matrices / vectors
BST_WEIGHTS = ("in_w", "in_b", "out_w", "out_b", "w1", "b1", "w2", "b2", "ln1_w", "ln1_b", "ln2_w", "ln2_b")


def bst_check(L1, dm, H, D=None, who="bst"):
    """The limits of fx_bst_block_*, raised here before anything is launched."""
    if not 1 <= L1 <= BST_MAX:
        raise NotImplementedError("{}: L1={} (history + target), the kernel's limit is 1 <= L1 <= {}"
                                  .format(who, L1, BST_MAX))
    if not 1 <= dm <= BST_MAX:
        raise NotImplementedError("{}: dm={}, the kernel's limit is 1 <= dm <= {}".format(who, dm, BST_MAX))
    if H < 1 or dm % H:
        raise NotImplementedError("{}: H={} does not divide dm={}".format(who, H, dm))
    if D is not None and (D < 1 or dm % D or dm // D > BST_MAX_PARTS + 1):
        raise NotImplementedError("{}: D={} must divide dm={} at most {} times".format(who, D, dm,
                                                                                       BST_MAX_PARTS + 1))


def bst_limits():
    """(most L1, most dm, forward grid, backward grid) of fx_bst_block_*."""
    lim = (C.c_int32 * 4)()
    _lib.load().fx_bst_limits(lim)
    return tuple(int(v) for v in lim)


def bst_grad_floats(L1, dm, pos_D):
    """grads of bst_block_bwd: [d in_w (3 dm dm) | d out_w | d w1 | d w2 (dm dm each) | d in_b (3 dm) | d out_b |
    d b1 | d b2 | d ln1_w | d ln1_b | d ln2_w | d ln2_b (dm each) | d position_emb (L1 * pos_D)]."""
    return 6 * dm * dm + 10 * dm + L1 * pos_D


def bst_workspace_floats(B, L1, dm, pos_D):
    return int(_lib.load().fx_bst_workspace_floats(B, L1, dm, pos_D))


def bst_flops(B, L1, dm, backward=False):
    """fp32 flops of one block: forward 2 L1 dm (6 dm + 2 L1) per sample (three projections, scores, P V, the output
    projection, two FFN layers); the backward runs that again and adds 2 L1 dm (15 dm + 5 L1): Q, K, V and the
    scores a second time, dP, dV, dQ, dK, four dX products over the weights and six weight gradients."""
    fwd = 2.0 * L1 * dm * (6 * dm + 2 * L1)
    return B * (fwd + 2.0 * L1 * dm * (15 * dm + 5 * L1) if backward else fwd)


SEQ_MAX_PARTS = 3    # room in struct fx_seq_parts; the entry points keep their own limits (BST 3, DIEN 2)


def _seq_parts(seqs, tgts, who, D=None):
    """struct fx_seq_parts of the sequence parts seqs[i] [B, L, D] and / or the target parts tgts[i] [B, D].  A side
    that is None stays null, and so does a part that is None (a gradient nobody wants; D then comes from the
    caller).  Unit stride over D, every other stride the tensor's own; an axis of extent 1, whose stride torch
    leaves arbitrary, gets the dense one."""
    sides = [list(p) for p in (tgts, seqs) if p is not None]
    n = len(sides[0])
    assert 1 <= n <= SEQ_MAX_PARTS and all(len(p) == n for p in sides), who
    d = _lib.SeqParts()
    D = D or next((t.shape[-1] for p in sides for t in p if t is not None), 1)
    for i, t in enumerate(tgts or ()):
        if t is not None:
            assert t.dim() == 2 and t.shape[1] == D and t.stride(1) == 1 and t.dtype == torch.float32, who
            d.tgt[i], d.tgt_ld[i] = t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else D)
    for i, s in enumerate(seqs or ()):
        if s is not None and s.shape[1] > 0:
            assert s.dim() == 3 and s.shape[2] == D and s.stride(2) == 1 and s.dtype == torch.float32, who
            d.seq[i] = s.data_ptr()
            d.seq_row_ld[i] = s.stride(1) if s.shape[1] > 1 else D
            d.seq_ld[i] = s.stride(0) if s.shape[0] > 1 else s.shape[1] * d.seq_row_ld[i]
    d.n_parts, d.D = n, D
    return d


def _seq_ids(ids, B, L, nullable=False):
    """(pointer, row stride) of the int32 ids [B, L] of the first sequence field; None (nothing is padded) only
    where nullable."""
    if ids is None and nullable:
        return vp(0), 0
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, L) and (L <= 1 or ids.stride(1) == 1)
    return ptr(ids), (ids.stride(0) if B > 1 else L)


def _bst_weights(w, pos, D):
    s = _lib.BstWeights()
    for name, t in zip(BST_WEIGHTS, w):
        if t is not None:
            assert t.is_contiguous() and t.dtype == torch.float32, name
            setattr(s, name, t.data_ptr())
    if pos is not None:
        assert pos.is_contiguous() and pos.shape[1] == D and pos.dtype == torch.float32, "position_emb"
        s.pos = pos.data_ptr()
    return s


def _bst_shape(seqs, tgts, pos):
    B, D = tgts[0].shape
    L1 = (seqs[0].shape[1] if seqs[0] is not None else 0) + 1
    return B, L1, D * (len(tgts) + (1 if pos is not None else 0)), D


def _bst_bytes_fwd(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool, Y):
    B, L1, dm, D = _bst_shape(seqs, tgts, pos)
    return 4.0 * (B * L1 * len(tgts) * D + (B * (L1 - 1) if ids is not None else 0) + Y.numel()
                  + 6 * dm * dm + 10 * dm)


def _bst_bytes_bwd(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool, dY, *a, **kw):
    B, L1, dm, D = _bst_shape(seqs, tgts, pos)
    G = min(B, bst_limits()[3])
    n = bst_grad_floats(L1, dm, D if pos is not None else 0)
    return 4.0 * (2 * B * L1 * len(tgts) * D + (B * (L1 - 1) if ids is not None else 0) + dY.numel()
                  + 6 * dm * dm + 10 * dm + 2 * G * n)


@_timed("bst_block_fwd", "bst", _bst_bytes_fwd)
def bst_block_fwd(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool, Y):
    """One transformer block.  seqs[i] [B, L, D] / tgts[i] [B, D]: part i of the history positions and of the target
    (views with unit stride over D are read in place; a later block passes x[:, :L] and x[:, L] of its [B, L1, dm]
    input), pos: position_emb [L1, D] or None, ids: int32 [B, L] of the first sequence field (0 = padding) or None,
    w: the 12 tensors of BST_WEIGHTS (the LayerNorm ones None without layer_norm), pool: a key of BST_POOLS.
    Y: [B, L1, dm] ("none" / "concat") or [B, dm], contiguous."""
    _need_cuda(Y, "Y")
    B, L1, dm, D = _bst_shape(seqs, tgts, pos)
    bst_check(L1, dm, H, D)
    assert Y.is_contiguous() and Y.numel() == (B * L1 * dm if BST_POOLS[pool] == 0 else B * dm)
    ip, iw = _seq_ids(ids, B, L1 - 1, nullable=True)
    check(_lib.load().fx_bst_block_fwd(C.byref(_seq_parts(seqs, tgts, "bst_block_fwd")), ip, iw, B, L1, dm, H,
                                       C.byref(_bst_weights(w, pos, D)), 1 if layer_norm else 0, 1 if residual else 0,
                                       1 if causal else 0, BST_POOLS[pool], ptr(Y), stream_ptr(Y.device)),
          "fx_bst_block_fwd")
    return Y


@_timed("bst_block_bwd", "bst", _bst_bytes_bwd)
def bst_block_bwd(seqs, tgts, pos, ids, w, H, layer_norm, residual, causal, pool, dY, dseqs, dtgts, grads, workspace,
                  dx_accumulate=False):
    """From dY (the shape of Y): the parts' gradients into dseqs[i] / dtgts[i] (the shapes of seqs / tgts, own
    strides; None: not wanted; added to when dx_accumulate) and grads [bst_grad_floats(..)].  workspace:
    bst_workspace_floats(B, L1, dm, pos_D) floats."""
    _need_cuda(dY, "dY")
    B, L1, dm, D = _bst_shape(seqs, tgts, pos)
    bst_check(L1, dm, H, D)
    pos_D = D if pos is not None else 0
    assert dY.is_contiguous() and dY.numel() == (B * L1 * dm if BST_POOLS[pool] == 0 else B * dm)
    assert grads.is_contiguous() and grads.numel() == bst_grad_floats(L1, dm, pos_D)
    assert workspace.is_contiguous() and workspace.numel() >= bst_workspace_floats(B, L1, dm, pos_D)
    ip, iw = _seq_ids(ids, B, L1 - 1, nullable=True)
    din = _seq_parts(dseqs, dtgts, "bst_block_bwd", D)
    check(_lib.load().fx_bst_block_bwd(C.byref(_seq_parts(seqs, tgts, "bst_block_bwd")), ip, iw, B, L1, dm, H,
                                       C.byref(_bst_weights(w, pos, D)), 1 if layer_norm else 0, 1 if residual else 0,
                                       1 if causal else 0, BST_POOLS[pool], ptr(dY), C.byref(din),
                                       1 if dx_accumulate else 0, ptr(grads), ptr(workspace),
                                       stream_ptr(dY.device)), "fx_bst_block_bwd")
    return grads


# ---- DIEN: GRU / AGRU / AUGRU over a padded history in one launch, and the attention scores ---------
GRU_MAX_H = 64       # hidden (= input) width of fx_gru_seq_*, a multiple of 4
GRU_MAX_L = 256
GRU_MAX_PARTS = 2
GRU_MODES = {"GRU": 0, "AGRU": 1, "AUGRU": 2}


def gru_check(H, L=None, who="gru"):
    """The limits of fx_gru_seq_* / fx_seq_score_*, raised here before anything is launched."""
    if H % 4 or not 4 <= H <= GRU_MAX_H:
        raise NotImplementedError("{}: H={}, the kernel's limit is 4 <= H <= {} and H % 4 == 0"
                                  .format(who, H, GRU_MAX_H))
    if L is not None and not 1 <= L <= GRU_MAX_L:
        raise NotImplementedError("{}: L={}, the kernel's limit is 1 <= L <= {}".format(who, L, GRU_MAX_L))


def gru_limits():
    """(most H, most L, forward grid, backward grid) of fx_gru_seq_*."""
    lim = (C.c_int32 * 4)()
    _lib.load().fx_gru_limits(lim)
    return tuple(int(v) for v in lim)


def gru_tile_rows(H):
    """Samples one workgroup of fx_gru_seq_* keeps on chip."""
    return int(_lib.load().fx_gru_tile_rows(H))


def gru_grad_floats(H):
    """grads of gru_seq_bwd: [d w_ih (3 H H) | d w_hh (3 H H) | d b_ih (3 H) | d b_hh (3 H)]."""
    return 6 * H * H + 6 * H


def gru_workspace_floats(B, H):
    return int(_lib.load().fx_gru_workspace_floats(B, H))


def seq_score_workspace_floats(B, H):
    return int(_lib.load().fx_seq_score_workspace_floats(B, H))


def _gru_shape(parts):
    B, L, D = parts[0].shape
    return B, L, D * len(parts)


def _gru_bytes_fwd(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh, states, final):
    B, L, H = _gru_shape(parts)
    return 4.0 * (2 * B * L * H + B * L * (2 if scores is not None else 1) + B * H + 6 * H * H + 6 * H)


def _gru_bytes_bwd(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh, states, d_states, d_final, *a, **kw):
    B, L, H = _gru_shape(parts)
    G = min(-(-B // gru_tile_rows(H)), gru_limits()[3])
    return 4.0 * (B * L * H * (3 + (d_states is not None)) + 3 * B * L + B * H + 6 * H * H + 6 * H
                  + 2 * G * gru_grad_floats(H))


@_timed("gru_seq_fwd", "gru", _gru_bytes_fwd)
def gru_seq_fwd(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh, states, final):
    """One recurrent layer over the history.  parts[i] [B, L, D]: column part i of the input (views with unit stride
    over D are read in place), ids: int32 [B, L] of the first sequence field (len = its non-zero count; positions
    0 .. len-1 run), scores: [B, L] a_t or None ("GRU"), mode: a key of GRU_MODES, w_ih / w_hh [3H, H], b_ih / b_hh
    [3H].  states [B, L, H] (0 past len) and final [B, H], contiguous."""
    _need_cuda(states, "states")
    B, L, H = _gru_shape(parts)
    gru_check(H, L)
    assert states.is_contiguous() and tuple(states.shape) == (B, L, H) and final.is_contiguous() \
        and tuple(final.shape) == (B, H)
    for t in (w_ih, w_hh, b_ih, b_hh):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert tuple(w_ih.shape) == (3 * H, H) and tuple(w_hh.shape) == (3 * H, H)
    assert scores is None or (scores.is_contiguous() and tuple(scores.shape) == (B, L))
    ip, iw = _seq_ids(ids, B, L)
    check(_lib.load().fx_gru_seq_fwd(C.byref(_seq_parts(parts, None, "gru_seq_fwd")), ip, iw, ptr(scores), B, L, H,
                                     GRU_MODES[mode], ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(states),
                                     ptr(final), stream_ptr(states.device)), "fx_gru_seq_fwd")
    return states, final


@_timed("gru_seq_bwd", "gru", _gru_bytes_bwd)
def gru_seq_bwd(parts, ids, scores, mode, w_ih, w_hh, b_ih, b_hh, states, d_states, d_final, dparts, d_scores, grads,
                workspace):
    """Back-propagation through time from d_states [B, L, H] and / or d_final [B, H] (None: no such gradient):
    the parts' gradients into dparts[i] (own strides; None: not wanted), d_scores [B, L] (not "GRU") and grads
    [gru_grad_floats(H)].  workspace: gru_workspace_floats(B, H) floats."""
    _need_cuda(grads, "grads")
    B, L, H = _gru_shape(parts)
    gru_check(H, L)
    assert states.is_contiguous() and tuple(states.shape) == (B, L, H)
    assert d_states is None or (d_states.is_contiguous() and tuple(d_states.shape) == (B, L, H))
    assert d_final is None or (d_final.is_contiguous() and tuple(d_final.shape) == (B, H))
    assert scores is None or (scores.is_contiguous() and d_scores.is_contiguous()
                              and tuple(d_scores.shape) == (B, L))
    assert grads.is_contiguous() and grads.numel() == gru_grad_floats(H)
    assert workspace.is_contiguous() and workspace.numel() >= gru_workspace_floats(B, H)
    ip, iw = _seq_ids(ids, B, L)
    check(_lib.load().fx_gru_seq_bwd(C.byref(_seq_parts(parts, None, "gru_seq_bwd")), ip, iw, ptr(scores), B, L, H,
                                     GRU_MODES[mode], ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(states),
                                     ptr(d_states), ptr(d_final),
                                     C.byref(_seq_parts(dparts, None, "gru_seq_bwd", H // len(parts))), ptr(d_scores),
                                     ptr(grads), ptr(workspace), stream_ptr(grads.device)),
          "fx_gru_seq_bwd")
    return grads


def _score_bytes(interest, tgts, ids, W, softmax, *a, **kw):
    B, L, H = interest.shape
    return 4.0 * (B * L * H + 2 * B * L + B * H + (H * H if W is not None else 0))


@_timed("seq_score_fwd", "gru", _score_bytes)
def seq_score_fwd(interest, tgts, ids, W, softmax, scores):
    """scores[b, t] = (interest[b, t] W) . target[b] (W None: the plain dot), times (ids != 0); with softmax then
    + -1e9 where ids == 0 and a soft-max over the L positions (a row without an open position: zeros).
    interest [B, L, H] contiguous, tgts[i] [B, D] the target's column parts, ids int32 [B, L]."""
    _need_cuda(scores, "scores")
    B, L, H = interest.shape
    gru_check(H, L, who="seq_score")
    assert interest.is_contiguous() and interest.dtype == torch.float32
    assert scores.is_contiguous() and tuple(scores.shape) == (B, L)
    assert W is None or (W.is_contiguous() and tuple(W.shape) == (H, H) and W.dtype == torch.float32)
    ip, iw = _seq_ids(ids, B, L)
    check(_lib.load().fx_seq_score_fwd(ptr(interest), C.byref(_seq_parts(None, tgts, "seq_score_fwd")), ip, iw, B, L, H,
                                       ptr(W), 1 if softmax else 0, ptr(scores), stream_ptr(scores.device)),
          "fx_seq_score_fwd")
    return scores


@_timed("seq_score_bwd", "gru", _score_bytes)
def seq_score_bwd(interest, tgts, ids, W, softmax, scores, d_scores, d_interest, dtgts, dW, workspace):
    """From d_scores and the forward's scores: d_interest [B, L, H] (None: not wanted), the target parts' gradients
    into dtgts[i] (None: not wanted), dW [H, H] (with W).  workspace: seq_score_workspace_floats(B, H) floats."""
    _need_cuda(d_scores, "d_scores")
    B, L, H = interest.shape
    gru_check(H, L, who="seq_score")
    assert interest.is_contiguous() and scores.is_contiguous() and d_scores.is_contiguous()
    assert tuple(scores.shape) == (B, L) and tuple(d_scores.shape) == (B, L)
    assert d_interest is None or (d_interest.is_contiguous() and tuple(d_interest.shape) == (B, L, H))
    assert W is None or (dW.is_contiguous() and dW.numel() == H * H
                         and workspace.numel() >= seq_score_workspace_floats(B, H))
    ip, iw = _seq_ids(ids, B, L)
    check(_lib.load().fx_seq_score_bwd(ptr(interest), C.byref(_seq_parts(None, tgts, "seq_score_bwd")), ip, iw, B, L, H,
                                       ptr(W), 1 if softmax else 0, ptr(scores), ptr(d_scores), ptr(d_interest),
                                       C.byref(_seq_parts(None, dtgts, "seq_score_bwd", H // len(tgts))), ptr(dW),
                                       ptr(workspace), stream_ptr(d_scores.device)), "fx_seq_score_bwd")
    return dW


# ---- evaluation metrics ---------------------------------------------------------------------------
def binary_metrics(y_pred, y_true):
    """(logloss, AUC) of float32 device vectors, as sklearn's log_loss / roc_auc_score on float64.
    One host sync (reads three 8-byte words)."""
    lib = _lib.load()
    y_pred = y_pred.reshape(-1).contiguous().float()
    y_true = y_true.reshape(-1).contiguous().float()
    n = y_pred.numel()
    nbytes = int(lib.fx_binary_metrics_workspace_bytes(n))
    if nbytes == 0:
        check(1, "fx_binary_metrics_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=y_pred.device)
    ll = torch.empty(1, dtype=torch.float64, device=y_pred.device)
    cnt = torch.empty(2, dtype=torch.int64, device=y_pred.device)
    check(lib.fx_binary_metrics(ptr(y_pred), ptr(y_true), n, ptr(ws), nbytes, ptr(ll), ptr(cnt),
                                stream_ptr(y_pred.device)), "fx_binary_metrics")
    s2, n_pos = (int(v) for v in cnt.tolist())
    n_neg = n - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that "
                         "case.")
    auc = (s2 - n_pos * (n_pos + 1)) / (2 * n_pos * n_neg)     # exact integers, one rounding
    return float(ll.item()) / n, auc


GROUP_METRIC_MAX_KS = 8


def group_metrics(y_pred, y_true, group_key, key_bits, ndcg_ks=()):
    """{"gAUC", "avgAUC", "MRR", "NDCG(k=K)" for K in ndcg_ks} -> float64 of float32 device vectors and a
    uint32 group key per sample (an int32 tensor holding the bits; only the low key_bits bits are read), as
    rank_model.evaluate_metrics computes them on the host.  Among equal predictions of a group the sample that
    came later in the input ranks first.  A metric whose weights sum to 0 is nan.  One host sync (reads
    2 * (3 + len(ndcg_ks)) + 1 doubles)."""
    lib = _lib.load()
    _need_cuda(y_pred, "y_pred")
    y_pred = y_pred.reshape(-1).contiguous().float()
    y_true = y_true.reshape(-1).contiguous().float()
    group_key = group_key.reshape(-1).contiguous()
    if group_key.dtype != torch.int32 or group_key.device != y_pred.device:
        raise _lib.FxError("group_metrics: group_key must be an int32 tensor (uint32 bits) on %s, got %s on %s"
                           % (y_pred.device, group_key.dtype, group_key.device))
    n = y_pred.numel()
    if y_true.numel() != n or group_key.numel() != n:
        raise _lib.FxError("group_metrics: %d predictions, %d labels, %d group keys"
                           % (n, y_true.numel(), group_key.numel()))
    ks = [int(k) for k in ndcg_ks]
    nbytes = int(lib.fx_group_metrics_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=y_pred.device)
    out = torch.empty(2 * (3 + len(ks)) + 1, dtype=torch.float64, device=y_pred.device)
    ks_arr = (C.c_int32 * max(len(ks), 1))(*ks)
    check(lib.fx_group_metrics(ptr(y_pred), ptr(y_true), ptr(group_key), int(key_bits), n, ks_arr, len(ks),
                               ptr(ws), nbytes, ptr(out), stream_ptr(y_pred.device)), "fx_group_metrics")
    sums = out.tolist()
    names = ["gAUC", "avgAUC", "MRR"] + ["NDCG(k=%d)" % k for k in ks]
    return OrderedDict((name, sums[2 * s] / sums[2 * s + 1] if sums[2 * s + 1] != 0.0 else float("nan"))
                       for s, name in enumerate(names))


# ---- FiGNN: the gated graph propagation over the fields and the attentional head (csrc/fx_fignn.hip) -----
FIGNN_GRU, FIGNN_RES, FIGNN_REUSE = 1, 2, 4


def fignn_flags(use_gru=True, use_residual=True, reuse_graph_layer=False):
    return (FIGNN_GRU if use_gru else 0) | (FIGNN_RES if use_residual else 0) | (FIGNN_REUSE if reuse_graph_layer else 0)


def fignn_limits():
    """The native envelope of fignn_fwd / fignn_bwd, stated once in the library."""
    lim = (C.c_int32 * 5)()
    _lib.load().fx_fignn_limits(lim)
    return dict(zip(("F_min", "FD_max", "D_max", "layers_max", "F_max"), (int(v) for v in lim)))


def fignn_check(F, D, layers, who="fignn"):
    """The limits of fx_fignn_*, raised here before anything is launched."""
    lim = fignn_limits()
    if not lim["F_min"] <= F <= lim["F_max"]:
        raise NotImplementedError("{}: F={}, the kernel's limit is {} <= F <= {} (a single field has no neighbour: "
                                  "the reference's soft-max row is all -inf)".format(who, F, lim["F_min"], lim["F_max"]))
    if not 1 <= D <= lim["D_max"] or F * D > lim["FD_max"]:
        raise NotImplementedError("{}: D={}, F*D={}, the kernel's limits are 1 <= D <= {} and F*D <= {}"
                                  .format(who, D, F * D, lim["D_max"], lim["FD_max"]))
    if not 1 <= layers <= lim["layers_max"]:
        raise NotImplementedError("{}: gnn_layers={}, the kernel's limit is 1 <= gnn_layers <= {}"
                                  .format(who, layers, lim["layers_max"]))


def fignn_tile_rows(F, D, flags=FIGNN_GRU | FIGNN_RES, backward=False):
    """Samples one workgroup of fx_fignn_fwd (or _bwd) keeps in LDS for all layers."""
    return int(_lib.load().fx_fignn_tile_rows(F, D, flags, 1 if backward else 0))


def fignn_layer_floats(F, D):
    """One layer's block of the packed graph weights: [W_in F D D | W_out F D D | bias_p D]."""
    return 2 * F * D * D + D


def fignn_grad_floats(F, D, layers, flags):
    """grads of fignn_bwd: [LW x (d W_in | d W_out | d bias_p) | d w_ih | d w_hh | d b_ih | d b_hh (GRU) | d w_attn]."""
    return int(_lib.load().fx_fignn_grad_floats(F, D, layers, flags))


def fignn_workspace_floats(B, F, D, layers, flags):
    """Floats of a workspace that serves fignn_bwd and fignn_head_bwd."""
    return int(_lib.load().fx_fignn_workspace_floats(B, F, D, layers, flags))


def _fignn_check(rec, F, D, layers, flags, W, gru, w_attn):
    _need_cuda(rec, "rec")
    fignn_check(F, D, layers)
    assert rec.dim() == 2 and rec.shape[1] == F * D and rec.stride(1) == 1 and rec.dtype == torch.float32
    LW = 1 if flags & FIGNN_REUSE else layers
    assert W.numel() == LW * fignn_layer_floats(F, D) and W.is_contiguous() and W.dtype == torch.float32
    assert w_attn.numel() == 2 * D and w_attn.is_contiguous()
    if flags & FIGNN_GRU:
        w_ih, w_hh, b_ih, b_hh = gru
        assert tuple(w_ih.shape) == (3 * D, D) and tuple(w_hh.shape) == (3 * D, D)
        assert b_ih.numel() == 3 * D and b_hh.numel() == 3 * D and all(t.is_contiguous() for t in gru)
    else:
        gru = (None,) * 4
    return rec.shape[0], gru


def _fignn_flops(rec, F, D, layers, flags, *a, **kw):
    per = F * D * (2 * D + F + (6 * D if flags & FIGNN_GRU else 0))
    return 2.0 * rec.shape[0] * (layers * per + F * F)


@_timed("fignn_fwd", "fignn", _fignn_flops)
def fignn_fwd(rec, F, D, layers, flags, W, gru, w_attn, h_out, hs):
    """h_out [B, F * D] = the FiGNN layer of rec [B, F * D] (unit column stride, any row stride): the attentional
    graph, then `layers` rounds of W_out / aggregation / W_in and the GRU cell (or the plain sum) with the residual.
    W: the packed graph weights, gru: (w_ih, w_hh, b_ih, b_hh) or None, w_attn [2 D]; hs [layers - 1, B, F * D] or None:
    the layers' inputs, kept for fignn_bwd."""
    B, gru = _fignn_check(rec, F, D, layers, flags, W, gru, w_attn)
    assert tuple(h_out.shape) == (B, F * D) and h_out.is_contiguous()
    assert hs is None or (hs.numel() == (layers - 1) * B * F * D and hs.is_contiguous())
    check(_lib.load().fx_fignn_fwd(ptr(rec), _rows(rec), B, F, D, layers, flags, ptr(W), ptr(gru[0]), ptr(gru[1]),
                                   ptr(gru[2]), ptr(gru[3]), ptr(w_attn), ptr(h_out), ptr(hs),
                                   stream_ptr(rec.device)), "fx_fignn_fwd")
    return h_out


@_timed("fignn_bwd", "fignn", lambda dh, rec, F, D, layers, flags, *a, **kw: 3.0 * _fignn_flops(rec, F, D, layers, flags))
def fignn_bwd(d_h_out, rec, F, D, layers, flags, W, gru, w_attn, hs, drec, grads, workspace):
    """From d_h_out [B, F * D]: drec [B, F * D] (own row stride) and grads [fignn_grad_floats(..)], summed over the
    batch in a fixed order (per-workgroup rows in workspace, then the column sums)."""
    B, gru = _fignn_check(rec, F, D, layers, flags, W, gru, w_attn)
    assert tuple(d_h_out.shape) == (B, F * D) and d_h_out.is_contiguous()
    assert layers == 1 or (hs is not None and hs.numel() == (layers - 1) * B * F * D and hs.is_contiguous())
    assert tuple(drec.shape) == (B, F * D) and drec.stride(1) == 1
    assert grads.numel() == fignn_grad_floats(F, D, layers, flags) and grads.is_contiguous()
    assert workspace.numel() >= fignn_workspace_floats(B, F, D, layers, flags) and workspace.is_contiguous()
    check(_lib.load().fx_fignn_bwd(ptr(d_h_out), ptr(rec), _rows(rec), B, F, D, layers, flags, ptr(W), ptr(gru[0]),
                                   ptr(gru[1]), ptr(gru[2]), ptr(gru[3]), ptr(w_attn), ptr(hs), ptr(drec),
                                   _rows(drec), ptr(grads), ptr(workspace), stream_ptr(rec.device)), "fx_fignn_bwd")
    return drec, grads


def _fignn_head_check(H, Z, w1, F, D):
    _need_cuda(H, "H")
    B = H.shape[0]
    assert tuple(H.shape) == (B, F * D) and H.is_contiguous() and H.dtype == torch.float32
    assert tuple(Z.shape) == (B, F) and Z.is_contiguous() and w1.numel() == D and w1.is_contiguous()
    if not 1 <= D <= fignn_limits()["D_max"]:
        raise NotImplementedError("fignn_head: D={}, the kernel's limit is 1 <= D <= {}"
                                  .format(D, fignn_limits()["D_max"]))
    return B


@_timed("fignn_head_fwd", "fignn")
def fignn_head_fwd(H, Z, w1, F, D, logit):
    """logit [B, 1] = sum_f sigmoid(Z[:, f]) (w1 . H[:, f]): H [B, F * D], Z [B, F] (the mlp2 product), w1 [D]."""
    B = _fignn_head_check(H, Z, w1, F, D)
    assert logit.numel() == B and logit.is_contiguous()
    check(_lib.load().fx_fignn_head_fwd(ptr(H), ptr(Z), ptr(w1), B, F, D, ptr(logit), stream_ptr(H.device)),
          "fx_fignn_head_fwd")
    return logit


@_timed("fignn_head_bwd", "fignn")
def fignn_head_bwd(g, H, Z, w1, F, D, dH, dZ, dw1, workspace):
    """From g = dlogit [B, 1]: dH [B, F * D] (the score's share), dZ [B, F] and dw1 [D] (a fixed-order sum)."""
    B = _fignn_head_check(H, Z, w1, F, D)
    assert g.numel() == B and g.is_contiguous()
    assert tuple(dH.shape) == (B, F * D) and dH.is_contiguous() and tuple(dZ.shape) == (B, F) and dZ.is_contiguous()
    assert dw1.numel() == D and dw1.is_contiguous()
    assert workspace.numel() >= fignn_workspace_floats(B, 0, 0, 0, 0) and workspace.is_contiguous()
    check(_lib.load().fx_fignn_head_bwd(ptr(g), ptr(H), ptr(Z), ptr(w1), B, F, D, ptr(dH), ptr(dZ), ptr(dw1),
                                        ptr(workspace), stream_ptr(H.device)), "fx_fignn_head_bwd")
    return dH, dZ, dw1


# ---- fused sparse front end / back end (csrc/fx_fused.hip) ----------------------------------------
class RowState(object):
    """One packed table + its optimizer state (struct fx_row_state)."""
    __slots__ = ("table", "m", "v", "last_step", "G", "D")

    def __init__(self, table, m, v, last_step, D, G=None):
        self.table, self.m, self.v, self.last_step, self.D, self.G = table, m, v, last_step, D, G


def _row_states(states):
    arr = (_lib.RowState * max(len(states), 1))()
    for i, s in enumerate(states):
        arr[i].table = s.table.data_ptr()
        arr[i].m = s.m.data_ptr() if s.m is not None else None
        arr[i].v = s.v.data_ptr() if s.v is not None else None
        arr[i].last_step = s.last_step.data_ptr() if s.last_step is not None else None
        arr[i].G = s.G.data_ptr() if s.G is not None else None
        arr[i].D = int(s.D)
        arr[i].table_dtype = _lib.FX_BF16 if s.table.dtype == torch.bfloat16 else _lib.FX_F32
        # row strides: 0 (packed) unless the arrays are fields of a row record
        arr[i].table_ld = _row_ld(s.table)
        arr[i].m_ld = _row_ld(s.m)
        arr[i].v_ld = _row_ld(s.v)
        arr[i].last_ld = 0 if s.last_step is None else int(s.last_step.stride(0))
    return arr


@_timed("dedup_catchup", "sparse_path")
def dedup_catchup(ids, col_row_base, col_vocab, col_pad, workspace, states, scal, begin_scal=None,
                  upto_offset=-1, want_uid=False, result=None):
    """Column fast path of the de-dup + (optionally) the fused begin-step + the exact-mode catch-up
    of every table group in `states` (list of RowState); 2 launches.  -> DedupResult."""
    lib = _lib.load()
    B, C_ = ids.shape
    if result is None:
        result = DedupResult(B * C_, C_, ids.device, want_uid=want_uid)
    check(lib.fx_dedup_catchup(ptr(ids), ids.stride(0), B, C_, ptr(col_row_base), ptr(col_vocab),
                               ptr(col_pad), ptr(workspace), workspace.numel(),
                               ptr(result.sorted_key), ptr(result.sorted_pos), ptr(result.uniq_row),
                               ptr(result.seg_start), ptr(result.n_unique), ptr(result.sorted_uid),
                               ptr(begin_scal), _row_states(states), len(states), upto_offset,
                               ptr(scal), stream_ptr(ids.device)), "fx_dedup_catchup")
    return result


def _emb_fm_bytes(table, D, ids, col_row_base, col_vocab, col_out_off, dense, num_w, num_out_off,
                  out, scal, table1=None, **kw):
    B = out.shape[0]
    C_ = 0 if ids is None else ids.shape[1]
    Fd = 0 if dense is None else dense.shape[1]
    # rows + ids + dense in (+ the 4-byte first-order rows), the record out
    eb = 2 if (table is not None and table.dtype == torch.bfloat16) else 4
    return B * (C_ * (eb * D + 4) + Fd * 4 + (C_ * 4 if table1 is not None else 0)
                + (C_ + Fd) * 4 * D)


@_timed("k_emb_fm_fwd", "sparse_path", _emb_fm_bytes, alone=True)
def emb_fm_fwd(table, D, ids, col_row_base, col_vocab, col_out_off, dense, num_w, num_out_off, out,
               scal, table1=None, num_w1=None, bias1=None, lr_out=None, fm_out=None, fm_lr_out=None,
               S=None, zero_ranges=()):
    """Gather + numeric expansion (+ first-order term) (+ FM second-order term), one launch.
    zero_ranges: up to two (offset, floats) ranges of every record row that the launch clears (reserved
    slots a later kernel of the step fills).
    table / table1 may be column ranges of a wider block (their row stride is passed on): the rows a
    row-sharded exchange delivered are read in place."""
    lib = _lib.load()
    B = out.shape[0]
    C_ = 0 if ids is None else ids.shape[1]
    Fd = 0 if dense is None else dense.shape[1]
    tdt = _lib.FX_BF16 if (table is not None and table.dtype == torch.bfloat16) else _lib.FX_F32
    check(lib.fx_emb_fm_fwd(ptr(table), tdt, D, ptr(ids), 0 if ids is None else ids.stride(0),
                            ptr(col_row_base), ptr(col_vocab), ptr(col_out_off), C_, ptr(dense),
                            0 if dense is None else dense.stride(0), ptr(num_w), ptr(num_out_off),
                            Fd, ptr(out), out.stride(0), B, ptr(table1), ptr(num_w1), ptr(bias1),
                            ptr(lr_out), ptr(fm_out), ptr(fm_lr_out), ptr(S), ptr(scal),
                            0 if table is None else table.stride(0),
                            0 if table1 is None else table1.stride(0),
                            *[int(x) for r in (tuple(zero_ranges) + ((0, 0), (0, 0)))[:2] for x in r],
                            stream_ptr(out.device)), "fx_emb_fm_fwd")
    return out


def emb_fm_bwd_partials(n_lookups, D):
    return int(_lib.load().fx_emb_fm_bwd_partials(n_lookups, D))


def emb_fm_bwd_workspace_floats(n_lookups, D, Fd):
    return int(_lib.load().fx_emb_fm_bwd_workspace_floats(n_lookups, D, Fd))


@_timed("emb_fm_bwd", "sparse_path")
def emb_fm_bwd(drec, rec, S, g_fm, g_lr, col_out_off, C_, D, dd, G, sq_partials, G1, sq1_partials,
               dense, num_out_off, B, dnum_w, dnum_w1, dbias1, workspace):
    """Backward of emb_fm_fwd: unique-row gradients of the D-float table (and of the D=1 table),
    their squared-norm partials, numeric weight / LR bias gradients; 2 launches.  dd must carry
    sorted_uid (dedup_catchup(..., want_uid=True))."""
    Fd = 0 if dense is None else dense.shape[1]
    have = dd is not None and C_ > 0
    check(_lib.load().fx_emb_fm_bwd(
        ptr(drec), 0 if drec is None else drec.stride(0), ptr(rec),
        0 if rec is None else rec.stride(0), ptr(S), ptr(g_fm), ptr(g_lr), ptr(col_out_off), C_, D,
        ptr(dd.sorted_pos) if have else vp(0), ptr(dd.sorted_uid) if have else vp(0),
        ptr(dd.seg_start) if have else vp(0), ptr(dd.n_unique) if have else vp(0),
        dd.n_max if have else 0, ptr(G), ptr(sq_partials), ptr(G1), ptr(sq1_partials), ptr(dense),
        0 if dense is None else dense.stride(0), ptr(num_out_off), Fd, B, ptr(dnum_w), ptr(dnum_w1),
        ptr(dbias1), ptr(workspace), stream_ptr(workspace.device)), "fx_emb_fm_bwd")


def adam_catchup_all(state, total_rows, upto_offset, scal):
    """Exact-mode flush of one table (fp32 or bf16): every row up to step + upto_offset."""
    check(_lib.load().fx_adam_catchup_all(_row_states([state]), total_rows, upto_offset, ptr(scal),
                                          stream_ptr(scal.device)), "fx_adam_catchup_all")


@_timed("adam_catchup_rows", "sparse_path")
def adam_catchup_rows(states, dd, upto_offset, scal):
    """Exact-mode catch-up of the unique rows of `dd` in every table group of `states` (RowState; fp32
    or bf16 tables), FX_MAX_TABLES groups per launch."""
    lib = _lib.load()
    for i in range(0, len(states), _lib.FX_MAX_TABLES):
        part = states[i:i + _lib.FX_MAX_TABLES]
        check(lib.fx_adam_catchup_rows(_row_states(part), len(part), ptr(dd.uniq_row),
                                       ptr(dd.n_unique), dd.n_max, upto_offset, ptr(scal),
                                       stream_ptr(scal.device)), "fx_adam_catchup_rows")


@_timed("owner_fetch_rows", "sparse_path")
def owner_fetch_rows(states, offs, dd, send, catchup, scal, upto_offset=-1, zero_row=None):
    """Owner side of the row-sharded forward: (exact-mode catch-up +) gather of every table group in
    `states` (RowState list) into its columns `offs` of the send block [n, ld]; one launch.
    zero_row: a 1-D fp32 view cleared on the way (the pad row of the received-rows block)."""
    arr = (C.c_int32 * len(offs))(*[int(o) for o in offs])
    check(_lib.load().fx_owner_fetch_rows(_row_states(states), arr, len(states), ptr(dd.uniq_row),
                                          ptr(dd.seg_start), ptr(dd.sorted_pos), ptr(dd.n_unique),
                                          send.shape[0], ptr(send), send.stride(0),
                                          1 if catchup else 0, upto_offset, ptr(scal), ptr(zero_row),
                                          0 if zero_row is None else zero_row.numel(),
                                          stream_ptr(send.device)), "fx_owner_fetch_rows")


@_timed("sparse_update_multi", "sparse_path")
def sparse_update_multi(kind, states, dd, scal):
    """Row update (kind 'adam' | 'sgd') of every table group in `states` (RowState with .G)."""
    lib = _lib.load()
    fn = lib.fx_sparse_adam_multi if kind == "adam" else lib.fx_sparse_sgd_multi
    check(fn(_row_states(states), len(states), ptr(dd.uniq_row), ptr(dd.n_unique), dd.n_max,
             ptr(scal), stream_ptr(scal.device)), "fx_sparse_%s_multi" % kind)


# Round 1's one-table argument lists.  Their C entry points are gone; these names stay, in Python only, because a host
# test installs its CPU emulation by replacing the functions of this module by name, and the tests of any earlier commit
# must keep running against this module.  Nothing in the package or its tests calls them: they build a list of one
# RowState and add no checks and no path of their own (adam_catchup of listed rows is adam_catchup_rows, quad replay
# included).  New code takes the RowState functions above.
def sparse_adam(table, m, v, last_step, D, dd, G, scal):
    sparse_update_multi("adam", [RowState(table, m, v, last_step, D, G)], dd, scal)


def sparse_sgd(table, D, dd, G, scal, last_step=None):
    sparse_update_multi("sgd", [RowState(table, None, None, last_step, D, G)], dd, scal)


def adam_catchup(table, m, v, last_step, D, dd, total_rows, upto_offset, scal):
    """dd=None: every row of the table (flush); else only the unique rows of dd."""
    state = RowState(table, m, v, last_step, D)
    if dd is None:
        adam_catchup_all(state, total_rows, upto_offset, scal)
    else:
        adam_catchup_rows([state], dd, upto_offset, scal)


def pack_columns_multi_prepare(items):
    """Validate `items` (see pack_columns_multi) and build the ctypes argument blocks ONCE.
    -> a callable that launches the cast on torch's current stream; it keeps the source and
    destination tensors alive.  A replayed training step on a batch it has already seen costs
    the launches alone (BaseModel's captured step: rank_model._GraphStep.fill)."""
    lib = _lib.load()
    if not items:
        return lambda: None
    B = items[0][1].shape[0]
    device = items[0][1].device
    calls, keep = [], []
    i = 0
    while i < len(items):
        chunk = items[i:i + _lib.FX_PACKM_MAX_COLS]
        cols, dts, ws, outs, odts, olds = [], [], [], [], [], []
        for t, out, col0 in chunk:
            _need_cuda(t, "input column")
            if t.dtype not in _DT or out.dtype not in (torch.int32, torch.float32):
                raise _lib.FxError("unsupported dtype %s -> %s" % (t.dtype, out.dtype))
            if not t.is_contiguous():
                t = t.contiguous()
            if t.shape[0] != B or out.shape[0] != B:
                raise _lib.FxError("input column has %d rows, expected %d" % (t.shape[0], B))
            cols.append(t)
            dts.append(_DT[t.dtype])
            ws.append(1 if t.dim() == 1 else int(t.shape[1]))
            outs.append(out.data_ptr() + col0 * out.element_size())
            odts.append(_DT[out.dtype])
            olds.append(out.stride(0))
            keep.append((t, out))
        oarr = (vp * len(outs))()
        for k, a in enumerate(outs):
            oarr[k] = a
        calls.append((_lib.ptr_array(cols), _lib.i32_array(dts), _lib.i32_array(ws), oarr,
                      _lib.i32_array(odts), _lib.i64_array(olds), len(cols), B))
        i += len(chunk)
    fn = lib.fx_pack_columns_multi

    def launch(_keep=keep):
        stream = stream_ptr(device)
        for c in calls:
            check(fn(*c, stream), "fx_pack_columns_multi")
    return launch


@_timed("pack_columns_multi", "other")
def pack_columns_multi(items):
    """items: list of (column tensor [B] | [B,w], destination matrix, first destination column);
    every column is cast into its destination (int32 or float32) in ONE launch per 96 columns."""
    pack_columns_multi_prepare(items)()
