"""Cases and references of the unfused embedding kernels (csrc/fx_embed.hip: gather, pooled sequences, numeric-weight
gradient, FM, LR, dot interaction) and of fx_emb_grad_reduce[_scaled] (csrc/fx_sparse.hip), shared by
tests/test_gpu_embed_arms.py (the kernels on an MI355X) and tests/test_embed_cases_host.py (the references and the
case lists themselves, no GPU).  A plain module: no fixtures.

Every operand a kernel reads through a leading dimension is a `View`: a column (and row) range of a wider block
whose other elements carry one bit pattern, FILL, so a kernel that assumes a packed operand reads garbage and one
that writes outside its slots is seen.  A reference is stated once, in plain torch, and evaluated in fp64 (the truth)
and in fp32 with left-to-right sums (`seq_sum`: the yardstick of rowopt_cases.within_yardstick); copies and single
multiplies are compared bit for bit.  No reference calls `ops` or tests/_cpu_emul.py."""
import functools
import os
import re
import types

import numpy as np
import torch

import fuxictr_amd
from rowopt_cases import FILL, geometry, within_yardstick  # noqa: F401  (re-exported)

# every (vec, lanes) class of fx_row_geom; 130, 65, 255: rows wider than one wave
WIDTHS = {4: [4, 16, 64, 256], 2: [2, 10, 126, 130], 1: [1, 3, 13, 63, 65, 255]}
ALL_D = sorted(d for ds in WIDTHS.values() for d in ds)
WAVE_D = [D for D in ALL_D if geometry(D)[1] <= 64]
WIDE_D = [D for D in ALL_D if geometry(D)[1] > 64]
# FM: S = max(16, lanes) lanes per sample; no width of WIDTHS has 32 lanes, so 31 (vec 1) and 128 (vec 4) join them
FM_D = [1, 2, 3, 4, 10, 13, 16, 31, 63, 64, 126, 128, 256]
FM_F = [1, 2, 5, 39]
POOL_SUM, POOL_MEAN = 0, 1
BAD_ID = 1                                                     # FX_FLAG_BAD_ID
U32 = 2.0 ** -24                                               # unit roundoff of fp32
NO_POS = 0xFFFFFFFF


def rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (1 << 31)
    return torch.Generator().manual_seed(seed)


def filled(*shape, dtype=torch.float32):
    return torch.full(shape, FILL, dtype=torch.int32).view(dtype) if dtype == torch.float32 else \
        torch.full(shape, -7, dtype=dtype)


def bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x.contiguous()


def same_bits(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    bad = (bits(a) != bits(b)).nonzero()
    assert bad.numel() == 0, (what, "differs at", bad[:4].tolist(), "of", tuple(a.shape))


def seq_sum(x, dim):
    """Left-to-right sum along `dim` in x's own dtype, one rounding per term (the fp32 yardstick's order)."""
    acc = torch.zeros_like(x.select(dim, 0)) if x.shape[dim] else x.sum(dim)
    for i in range(x.shape[dim]):
        acc = acc + x.select(dim, i)
    return acc


class View(object):
    """values [r, c] inside a block of FILL: `margin` columns either side (a multiple of the row's vec keeps the
    vector accesses aligned) and one guard row above and below."""

    def __init__(self, values, margin=0, rows=True):
        values = torch.as_tensor(values)
        r, c = values.shape
        g = 1 if rows else 0
        self.block = filled(r + 2 * g, c + 2 * margin, dtype=values.dtype)
        self.rows, self.cols = slice(g, g + r), slice(margin, margin + c)
        self.block[self.rows, self.cols] = values
        self.init = self.block.clone()

    def host(self):
        return self.block[self.rows, self.cols]

    def on(self, device):
        """-> the view of a fresh device copy of the block (kept as self.dev_block)."""
        self.dev_block = self.init.clone().to(device)
        return self.dev_block[self.rows, self.cols]

    def untouched(self, what, written=None):
        """Every element of the device block outside the view (and outside `written`, a bool mask over the view)
        carries its first bits."""
        now = self.dev_block.cpu()
        free = torch.zeros(now.shape, dtype=torch.bool)
        free[self.rows, self.cols] = True if written is None else written
        bad = ((bits(now) != bits(self.init)) & ~free).nonzero()
        assert bad.numel() == 0, ("written outside its slots: %s at %s" % (what, bad[:4].tolist()))


# ---- launch limits, read once from the sources ---------------------------------------------------------------------
def _src(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(fuxictr_amd.__file__)), "csrc", name)) as f:
        return f.read()


def _body(src, name):
    m = re.search(r'^(?:extern "C" |static )int %s\(' % name, src, re.M)
    assert m, name
    return src[m.start():src.index("\n}\n", m.start())]


def _prod(text):
    out = 1
    for t in text.split("*"):
        out *= int(t)
    return out


def _cap(body):
    m = re.search(r"if \((\w+) > ([0-9 *]+)\) \1 = \2;", body)
    assert m, body[:80]
    return _prod(m.group(2))


def _define(src, name):
    return int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))


@functools.lru_cache(maxsize=None)
def limits():
    """The grid caps and thresholds of the kernels under test (workgroups; items per workgroup are the kernels')."""
    e, s = _src("fx_embed.hip"), _src("fx_sparse.hip")
    dot = _body(e, "fx_dot_interact_fwd")
    return types.SimpleNamespace(
        gather_blocks=_cap(_body(e, "fx_emb_gather_fwd")),
        pool_blocks=_cap(_body(e, "fx_emb_seq_pool_fwd")), pool_items=4,
        fm_blocks=_cap(_body(e, "fx_fm_launch")),
        lr_blocks=_cap(_body(e, "fx_lr_fwd")), lr_items=16,
        dot_mfma_blocks=_cap(dot), dot_mfma_items=4,
        dot_plain_blocks=int(re.search(r"blocks = B < (\d+) \? B : \1;", dot).group(1)),
        dot_max_fd=_define(e, "FX_DOT_MAX_FD"), numgrad_chunks=_define(e, "FX_NUMGRAD_CHUNKS"),
        long_run=_define(s, "FX_LONG_RUN"),
        long_blocks=int(re.search(r"grid_long\((\d+)\)", s).group(1)))


def fm_lanes(D):
    return max(16, geometry(D)[1])


def dot_mfma(F, D):
    """fx_dot_mfma_ok with FX_DOT_MFMA unset."""
    return F <= 32 and D <= 32 and D % 2 == 0


# ---- gather --------------------------------------------------------------------------------------------------------
GATHER_STRIDE = dict(D=255, B=1030, C=5, Fd=3)                 # one item per workgroup, 8240 items


def gather_case(D, B=37, C=4, Fd=3, strided=True, edge_ids=True, n_cols=None, seed=0):
    """C id columns over C tables and Fd numeric columns into interleaved slots of a record whose rows are wider than
    the slots (one slot and a margin are nobody's).  strided: the table is a column range of a wider block, ids and
    dense column ranges of wider matrices.  n_cols: only the first n_cols id columns are gathered.  edge_ids: column
    0 holds the ids -1, vocab and vocab - 1 in samples 0, 1, 2."""
    g = rng(1, D, B, C, Fd, seed)
    vec, _ = geometry(D)
    vocabs = [5 + 6 * c for c in range(C)]
    bases = [int(x) for x in np.concatenate([[0], np.cumsum(vocabs)[:-1]])] if C else []
    R = max(1, sum(vocabs))
    k = types.SimpleNamespace(D=D, B=B, C=C, Fd=Fd, vocabs=vocabs, bases=bases, R=R, vec=vec)
    k.n_cols = C if n_cols is None else n_cols
    m = vec if strided else 0
    k.table = View(torch.randn(R, D, generator=g), margin=2 * m)
    ids = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocabs], 1).int() if C else \
        torch.zeros(B, 0, dtype=torch.int32)
    if edge_ids and C:
        ids[0, 0], ids[1, 0], ids[2, 0] = -1, vocabs[0], vocabs[0] - 1
    k.ids = View(ids, margin=3 if strided else 0, rows=False)
    k.dense = View(torch.rand(B, Fd, generator=g) + 0.5, margin=2 if strided else 0, rows=False)
    k.num_w = torch.randn(Fd, D, generator=g)
    n_slots = k.n_cols + Fd + 1
    order = torch.randperm(n_slots, generator=g).tolist()      # slot of: id columns, numeric columns, nobody
    k.col_off = [order[c] * D for c in range(k.n_cols)]
    k.num_off = [order[k.n_cols + j] * D for j in range(Fd)]
    k.out = View(filled(B, n_slots * D), margin=m, rows=True)   # the record itself starts as FILL too
    return k


def gather_ref(k):
    """-> (record [B, n_slots * D] bit for bit, mask of the floats the launch writes, error flag)."""
    ids, table, dense = k.ids.host().long(), k.table.host(), k.dense.host()
    out = k.out.init[k.out.rows, k.out.cols].clone()
    written = torch.zeros(out.shape, dtype=torch.bool)
    flag = 0
    for c in range(k.n_cols):
        ok = (ids[:, c] >= 0) & (ids[:, c] < k.vocabs[c])
        rows = table[ids[:, c].clamp(0, k.vocabs[c] - 1) + k.bases[c]].clone()
        rows[~ok] = 0.0
        out[:, k.col_off[c]:k.col_off[c] + k.D] = rows
        written[:, k.col_off[c]:k.col_off[c] + k.D] = True
        flag |= BAD_ID if bool((~ok).any()) else 0
    for j in range(k.Fd):
        out[:, k.num_off[j]:k.num_off[j] + k.D] = dense[:, j:j + 1] * k.num_w[j]       # one fp32 multiply
        written[:, k.num_off[j]:k.num_off[j] + k.D] = True
    return out, written, flag


# ---- pooled sequences ----------------------------------------------------------------------------------------------
POOL_D = [1, 16, 64, 256, 126]                                 # P = 64, 16, 4, 1 and 1 positions per wave
POOL_STRIDE = dict(D=4, B=8200, lens=[2, 2, 2, 2])


def pool_positions(D):
    return 64 // geometry(D)[1]


def pool_lens(D):
    P = pool_positions(D)
    return sorted({L for L in (1, P - 1, P, P + 1, 2 * P + 3) if L >= 1})


def pool_case(D, B=21, lens=None, strided=True, bad=False, seed=0):
    """One sequence feature per entry of lens (its own table of 23 rows, row 0 the zero padding row, row 1 a row of
    [1, -1, 0 ...] that sums to exactly 0 without being padding), modes MEAN / SUM alternating, behind one plain
    column.  Sample 0: empty histories; 1: full; 2: padding in the middle; 3: the bad id when `bad`; 4: the
    zero-sum row first (L >= 2); the rest: every position padding with probability 0.4."""
    g = rng(2, D, B, seed)
    lens = pool_lens(D) if lens is None else list(lens)
    vec, _ = geometry(D)
    V = 23
    n_seq = len(lens)
    k = types.SimpleNamespace(D=D, B=B, lens=lens, n_seq=n_seq, vec=vec, V=V)
    table = torch.randn((n_seq + 1) * V, D, generator=g)
    for s in range(n_seq):
        table[s * V] = 0.0
        if D >= 2:
            table[s * V + 1] = 0.0
            table[s * V + 1, 0], table[s * V + 1, 1] = 1.0, -1.0
    k.table = View(table, margin=2 * vec if strided else 0)
    cols = [torch.randint(0, V, (B, 1), generator=g)]
    k.col_base, k.col_vocab, k.seq_col0 = [n_seq * V], [V], []
    for s, L in enumerate(lens):
        x = torch.randint(2, V, (B, L), generator=g)
        x[torch.rand(B, L, generator=g) < 0.4] = 0
        x[0] = 0
        if B > 4:
            x[1] = torch.randint(2, V, (L,), generator=g)
            x[2] = torch.randint(2, V, (L,), generator=g)
            x[2, L // 2] = 0
            x[3] = torch.randint(2, V, (L,), generator=g)
            if bad and s % 2 == 0:
                x[3, L - 1] = V if s % 4 == 0 else -1
            if L >= 2:                                          # (alone it would be a mean of 1 / 1e-12)
                x[4, 0], x[4, 1] = 1, 2 + s
        k.seq_col0.append(sum(c.shape[1] for c in cols))
        cols.append(x)
        k.col_base += [s * V] * L
        k.col_vocab += [V] * L
    k.ids = View(torch.cat(cols, 1).int(), margin=2 if strided else 0, rows=False)
    k.modes = [POOL_MEAN if s % 2 == 0 else POOL_SUM for s in range(n_seq)]
    k.out_off = [(n_seq - 1 - s) * D for s in range(n_seq)]     # slots in reverse order, one spare slot behind
    k.out = View(filled(B, (n_seq + 1) * D), margin=vec, rows=True)
    return k


def pool_ref(k, dtype):
    """-> (pooled [B, n_seq, D] in dtype, denom [B, n_seq] fp32, flag): feature s sums its valid rows left to right;
    a position counts towards the mean when its row does not sum to exactly 0; denom = count + 1e-12 in fp32."""
    ids, table = k.ids.host().long(), k.table.host().to(dtype)
    pooled = torch.zeros(k.B, k.n_seq, k.D, dtype=dtype)
    denom = torch.zeros(k.B, k.n_seq)
    flag = 0
    for s, L in enumerate(k.lens):
        x = ids[:, k.seq_col0[s]:k.seq_col0[s] + L]
        ok = (x >= 0) & (x < k.V)
        e = table[x.clamp(0, k.V - 1) + s * k.V] * ok.unsqueeze(-1).to(dtype)
        flag |= BAD_ID if bool((~ok).any()) else 0
        denom[:, s] = (e.double().sum(-1) != 0).float().sum(-1) + 1e-12
        total = seq_sum(e, 1)
        pooled[:, s] = total / denom[:, s:s + 1].to(dtype) if k.modes[s] == POOL_MEAN else total
    return pooled, denom, flag


# ---- numeric-weight gradient ---------------------------------------------------------------------------------------
NUMGRAD_D = [1, 3, 16, 17, 255, 256]
NUMGRAD_B = [1, 15, 16, 17, 1000]


def numgrad_case(D, B, Fd=3, seed=0):
    """dW[j, :] = sum_b dense[b, j] * dout[b, slot j]: the numeric slots are every second slot of a record whose rows
    are wider than the slots; dense is a column range of a wider matrix."""
    g = rng(3, D, B, Fd, seed)
    k = types.SimpleNamespace(D=D, B=B, Fd=Fd)
    n_slots = 2 * Fd + 1
    k.num_off = [(2 * j + 1) * D for j in range(Fd)]
    k.dout = View(torch.randn(B, n_slots * D, generator=g), margin=3, rows=True)
    k.dense = View(torch.rand(B, Fd, generator=g) - 0.3, margin=2, rows=False)
    return k


def numgrad_ref(k, dtype):
    dout, dense = k.dout.host().to(dtype), k.dense.host().to(dtype)
    return torch.stack([seq_sum(dense[:, j:j + 1] * dout[:, o:o + k.D], 0) for j, o in enumerate(k.num_off)])


# ---- FM ------------------------------------------------------------------------------------------------------------
FM_STRIDE = dict(F=2, D=4, B=65541)


def fm_case(F, D, B=37, seed=0):
    g = rng(4, F, D, B, seed)
    vec, _ = geometry(D)
    k = types.SimpleNamespace(F=F, D=D, B=B, vec=vec)
    k.emb = View(torch.randn(B, F * D, generator=g) * 0.5, margin=vec, rows=True)
    k.addend = torch.randn(B, generator=g)
    k.g = torch.randn(B, generator=g)
    k.demb0 = torch.randn(B, F * D, generator=g)               # what accumulate adds to
    return k


def fm_ref(emb, addend, dtype):
    """emb [B, F, D] -> 0.5 * sum_d((sum_f e)^2 - sum_f e^2) (+ addend), [B]."""
    e = emb.to(dtype)
    out = seq_sum((seq_sum(e, 1) ** 2 - seq_sum(e * e, 1)) * 0.5, 1)
    return out if addend is None else out + addend.to(dtype)


def fm_grad_ref(emb, g, base, dtype):
    """d/d emb of sum_b g[b] * fm[b]: g * (sum_f e - e), [B, F, D] (+ base, what the launch accumulates onto)."""
    e = emb.to(dtype)
    d = g.to(dtype).view(-1, 1, 1) * (seq_sum(e, 1).unsqueeze(1) - e)
    return d if base is None else base.to(dtype).view_as(d) + d


# ---- LR ------------------------------------------------------------------------------------------------------------
LR_C = [0, 1, 15, 16, 17, 40]
LR_FD = [0, 1, 17]
LR_STRIDE = dict(C=3, Fd=1, B=65541)


def lr_case(C, Fd, B=37, bad=False, seed=0):
    """The D = 1 table is column 1 of a 3-column block (table1_ld = 3); ids and dense column ranges."""
    g = rng(5, C, Fd, B, seed)
    vocabs = [3 + (5 * c) % 11 for c in range(C)]
    k = types.SimpleNamespace(C=C, Fd=Fd, B=B, vocabs=vocabs)
    k.bases = [int(x) for x in np.concatenate([[0], np.cumsum(vocabs)[:-1]])] if C else []
    k.table1 = View(torch.randn(max(1, sum(vocabs)), 1, generator=g), margin=1)
    ids = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocabs], 1).int() if C else \
        torch.zeros(B, 0, dtype=torch.int32)
    if bad:
        ids[1, 0], ids[B - 1, C - 1] = -1, vocabs[C - 1]
    k.ids = View(ids, margin=2, rows=False)
    k.dense = View(torch.rand(B, Fd, generator=g) - 0.4, margin=1, rows=False)
    k.w1 = torch.randn(Fd, generator=g)
    k.bias = torch.randn(1, generator=g)
    return k


def lr_ref(k, bias, dtype):
    ids, t = k.ids.host().long(), k.table1.host()[:, 0].to(dtype)
    terms, flag = [], 0
    for c in range(k.C):
        ok = (ids[:, c] >= 0) & (ids[:, c] < k.vocabs[c])
        terms.append(t[ids[:, c].clamp(0, k.vocabs[c] - 1) + k.bases[c]] * ok.to(dtype))
        flag |= BAD_ID if bool((~ok).any()) else 0
    terms += [k.dense.host()[:, j].to(dtype) * k.w1[j].to(dtype) for j in range(k.Fd)]
    out = seq_sum(torch.stack(terms, 1), 1) if terms else torch.zeros(k.B, dtype=dtype)
    return (out + k.bias.to(dtype) if bias else out), flag


# ---- dot interaction -----------------------------------------------------------------------------------------------
DOT_MFMA = [(2, 2), (3, 16), (31, 30), (32, 32), (5, 2), (27, 16)]
DOT_PLAIN = [(2, 3), (3, 13), (5, 34), (33, 4), (16, 256)]      # odd D, D = 34, F = 33, F * D = FX_DOT_MAX_FD
DOT_MFMA_STRIDE = dict(F=3, D=2, B=8197)
DOT_PLAIN_STRIDE = dict(F=3, D=3, B=8195)


def pairs(F):
    i, j = np.triu_indices(F, 1)                               # row-major upper triangle: the kernels' pair order
    return torch.from_numpy(i), torch.from_numpy(j)


def dot_case(F, D, B=13, tail=0, seed=0):
    g = rng(6, F, D, B, tail, seed)
    P = F * (F - 1) // 2
    k = types.SimpleNamespace(F=F, D=D, B=B, tail=tail, P=P)
    k.emb = View(torch.randn(B, F * D, generator=g), margin=1, rows=True)
    k.g = View(torch.randn(B, P + tail, generator=g), margin=2, rows=True)
    k.out = View(filled(B, P + tail), margin=1, rows=True)
    k.demb = View(filled(B, F * D), margin=3, rows=True)
    return k


def dot_ref(emb, tail, dtype):
    """emb [B, F, D] -> [dots of the pairs i < j | last field | zeros], [B, P + tail]."""
    e = emb.to(dtype)
    B, F, D = e.shape
    i, j = pairs(F)
    out = seq_sum(e[:, i] * e[:, j], 2)
    if tail:
        out = torch.cat([out, e[:, F - 1], torch.zeros(B, tail - D, dtype=dtype)], 1)
    return out


def dot_grad_ref(emb, g, tail, dtype):
    """de[b, i] = sum_{j != i} g[b, p(i, j)] e[b, j], j ascending (+ the gradient of the appended copy)."""
    e, g = emb.to(dtype), g.to(dtype)
    B, F, D = e.shape
    i, j = pairs(F)
    G = torch.zeros(B, F, F, dtype=dtype)
    G[:, i, j] = g[:, :len(i)]
    G[:, j, i] = g[:, :len(i)]
    de = seq_sum(G.unsqueeze(-1) * e.unsqueeze(1), 2)
    if tail:
        de[:, F - 1] += g[:, len(i):len(i) + D]
    return de


# ---- gradient reduce -----------------------------------------------------------------------------------------------
RUNS = [1, 31, 32, 33, 64]
REDUCE_MANY_LONG = dict(D=2, n_rows=520, run=33)


def reduce_case(D, runs, hot=0, pads=(), C=3, scaled=False, seed=0):
    """Unique row u has runs[u] lookups (+ `hot` more for the last row); lookup positions p = b * C + c are dealt out
    to the runs at random and listed ascending inside a run, as the stable de-dup leaves them.  pads: (row, index
    inside its run) of lookups that are padding: sorted_pos = 0xFFFFFFFF, no contribution.  scaled: columns 0 and 2
    divide by their sample's pooling denominator (col_denom -> a [B, 2] denom matrix inside a wider one)."""
    g = rng(7, D, len(runs), hot, C, seed)
    runs = list(runs)
    runs[-1] += hot
    n = sum(runs)
    B = (n + C - 1) // C
    vec, _ = geometry(D)
    k = types.SimpleNamespace(D=D, C=C, B=B, runs=runs, n=n, n_max=B * C, nu=len(runs), scaled=scaled, vec=vec)
    perm = torch.randperm(B * C, generator=g)[:n]
    seg = np.concatenate([[0], np.cumsum(runs)])
    pos = torch.cat([perm[seg[u]:seg[u + 1]].sort().values for u in range(k.nu)]).long()
    k.row_of = torch.repeat_interleave(torch.arange(k.nu), torch.as_tensor(runs))
    k.live = torch.ones(n, dtype=torch.bool)
    for u, i in pads:
        k.live[seg[u] + i] = False
    k.pos = pos
    sp = torch.full((k.n_max,), NO_POS, dtype=torch.int64)      # the tail behind seg_start[nu]: never read
    sp[:n] = torch.where(k.live, pos, torch.full_like(pos, NO_POS))
    k.sorted_pos = torch.where(sp == NO_POS, torch.full_like(sp, -1), sp).to(torch.int32)      # the uint32's bits
    ss = torch.zeros(k.n_max + 1, dtype=torch.int32)
    ss[:k.nu + 1] = torch.as_tensor(seg, dtype=torch.int32)
    k.seg_start = ss
    n_slots = C + 1
    k.col_off = [(C - c) * D for c in range(C)]                 # slots in reverse order, slot 0 nobody's
    k.dout = View(torch.randn(B, n_slots * D, generator=g), margin=vec, rows=True)
    k.col_denom = [0, -1, 1][:C] if scaled else None
    k.denom = View(torch.randint(1, 9, (B, 2), generator=g).float() + 1e-12, margin=1, rows=False)
    return k


def reduce_standard(D, scaled=False, seed=0):
    """Runs of every length of RUNS (twice) and a hot last row with four fifths of the lookups, long enough for chunks
    of 8 lookups per lane group of the workgroup-per-row kernel; a padding lookup inside the first chunk of 4 of a short run, inside the remainder
    of another, and inside a chunk of 8 of lane group 0 of the hot row."""
    rpb = 256 // geometry(D)[1]
    runs = RUNS + RUNS[::-1] + [1]
    return reduce_case(D, runs, hot=max(8 * rpb + 40, 4 * sum(runs)), pads=((1, 1), (4, 63), (8, 29), (len(runs) - 1, 3 * rpb)),
                       scaled=scaled, seed=seed)


def reduce_ref(k, dtype):
    """G [nu, D]: the live lookups of a row, in ascending position, each divided by its denominator first."""
    dout = k.dout.host().to(dtype)
    pos = k.pos[k.live]
    b, c = pos // k.C, pos % k.C
    off = torch.as_tensor(k.col_off)[c]
    vals = dout[b.unsqueeze(1), off.unsqueeze(1) + torch.arange(k.D).unsqueeze(0)]
    if k.scaled:
        j = torch.as_tensor(k.col_denom)[c]
        den = k.denom.host()[b, j.clamp(min=0)].to(dtype)
        vals = torch.where((j >= 0).unsqueeze(1), vals / den.unsqueeze(1), vals)
    return torch.zeros(k.nu, k.D, dtype=dtype).index_add_(0, k.row_of[k.live], vals)


def sqnorm_bound(ref64, elem_bound, terms):
    """|sum(sq_partials) - ||G||^2| for a G within elem_bound of ref64 elementwise, the partials fp32 sums of `terms`
    non-negative products each and the total taken in fp64: (terms + 1) u ||G||^2 (Higham's gamma_n for a sum of
    non-negative terms in any order) + 2 ||G|| E + E^2 with E = sqrt(numel) * elem_bound."""
    n2 = float((ref64 ** 2).sum())
    E = (ref64.numel() ** 0.5) * elem_bound
    return (terms + 1) * U32 * n2 + 2 * (n2 ** 0.5) * E + E * E


def floor_of(ref64, scale=None):
    """The floor of within_yardstick: one fp32 rounding (2u) of the largest result, or of `scale` where the result is
    a difference of larger sums (a reference whose fp32 restatement happens to be exact, such as the FM term of one
    field, 0.5 * (e^2 - e^2), still admits one rounding of what an evaluation in another order holds in between)."""
    top = float(ref64.abs().max()) if ref64.numel() else 0.0
    return 2 * U32 * max(top, scale or 0.0, 2.0 ** -126)


def fm_scale(emb):
    """The largest 0.5 * (sum_d (sum_f e)^2 + sum_fd e^2) of a sample: the two sums whose difference the FM term is."""
    e = emb.double()
    return float((0.5 * ((e.sum(1) ** 2).sum(1) + (e * e).sum((1, 2)))).max())
