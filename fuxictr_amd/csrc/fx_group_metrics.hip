// fx_group_metrics.hip — on-device group metrics: gAUC, avgAUC, MRR and NDCG@k of fuxictr/metrics.py:57-189
// (pandas.groupby + a process pool + one roc_auc_score call per group in the reference).
//
// Per group of n samples with n+ positives (positive: y > 0.5), metric = sum value / sum weight over the groups:
//   gAUC     value AUC * n, weight n       for 0 < n+ < n, else (0, 0)          metrics.py:115-130
//   avgAUC   value AUC,     weight 1       for 0 < n+ < n, else (0, 0)          metrics.py:99-113
//   MRR      value sum y / rank / (n+ + 1e-12), weight 1, every group           metrics.py:132-146
//   NDCG@K   value DCG@K / (IDCG@K + 1e-12),    weight 1, every group           metrics.py:149-189
// rank = 1-based position in descending prediction order.  The reference's argsort()[::-1] defines nothing for
// tied predictions; the rule here: AMONG EQUAL PREDICTIONS THE SAMPLE THAT CAME LATER IN THE INPUT RANKS FIRST
// (the reverse of the stable ascending order, which is what the stable radix sort leaves).
//
// Passes (no allocation, no synchronisation, no atomics of its own; fx_sort.hip's are integer):
//   k_gm_keys      order-preserving prediction key, value (index << 1 | label)
//   sort 1         stable, by prediction (32 bits)
//   k_gm_gkeys     group key gathered through the permutation, value (position after sort 1 << 1 | label)
//   sort 2         stable, by group key over key_bits only: groups contiguous, predictions ascending inside a
//                  group, input order kept inside ties
//   k_gm_gather    the prediction key of every element in the final order
//   k_gm_idcg      idcg[m] = sum_{r <= m} 1 / log2(r + 1), m <= min(max K, n)
//   k_gm_tile_heads / k_gm_tile_scan   per 1024-element tile: its last tie-run head, first tie-run tail, first
//                  group tail; then, over the tiles, what each tile inherits from the tiles before / after it
//   k_gm_segments  one element a lane.  From wave ballots of the head / tail flags (+ the per-wave words in LDS
//                  + the tile's inherited words) every element knows its tie run [R0, R1) and its group's end E,
//                  hence rank = E - i and — for a positive — twice its average rank inside the group,
//                  R0 + R1 + 1 - 2 S (S: group start, subtracted once per group).  A segmented wave scan sums
//                  (sum of R0 + R1 + 1 | n+ | sum 1 / rank | DCG@K...) per group piece: a group inside one
//                  64-element chunk is finished on the spot; a piece that crosses a chunk edge is written out
//   k_gm_fixup     one wave per chunk that holds the head of a crossing group: sums the group's pieces (lanes
//                  strided over the chunks, fixed shuffle tree) and finishes it
//   k_gm_finish    fixed-order fp64 sum of the per-tile results
// No thread walks a group: a group of 10^4 rows is 157 chunk pieces and one 157-term wave sum.  The AUC part is
// exact integer arithmetic (n <= 2^26: n+ (2 n + 1) < 2^54) with one fp64 division per group; all fp64 sums have
// a fixed order, so two runs give the same bits.
#include "fx_common.h"

#define FX_GM_TILE 1024            // elements (= threads) per workgroup of the segmented passes
#define FX_GM_WAVES (FX_GM_TILE / 64)
#define FX_GM_MAX_K 8              // NDCG cut-offs per call
#define FX_GM_NV (6 + FX_GM_MAX_K) // per-group result: gAUC v, w | avgAUC v, w | MRR v | 1 | NDCG v ...

namespace {

struct GmKs {
    int32_t k[FX_GM_MAX_K];
    int32_t nk;
};

// sums of one piece of a group
struct GmPart {
    unsigned long long a;          // sum over its positives of R0 + R1 + 1 (global positions)
    unsigned long long np;         // positives
    double mrr;                    // sum over its positives of 1 / rank
    double dcg[FX_GM_MAX_K];       // sum over its positives with rank <= K of 1 / log2(rank + 1)
};

__global__ __launch_bounds__(256) void k_gm_keys(const float* pred, const float* label, int64_t n,
                                                 uint32_t* key, uint32_t* val) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        uint32_t u = __float_as_uint(pred[i] + 0.0f);          // (-0.0 sorts with +0.0)
        u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;            // order-preserving float -> uint
        key[i] = u;
        val[i] = ((uint32_t)i << 1) | (label[i] > 0.5f ? 1u : 0u);
    }
}

__global__ __launch_bounds__(256) void k_gm_gkeys(const uint32_t* group_key, const uint32_t* val1, int64_t n,
                                                  uint32_t mask, uint32_t* gk, uint32_t* gv) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t v = val1[i];
        gk[i] = group_key[v >> 1] & mask;
        gv[i] = ((uint32_t)i << 1) | (v & 1u);
    }
}

__global__ __launch_bounds__(256) void k_gm_gather(const uint32_t* key1, const uint32_t* vs, int64_t n,
                                                   uint32_t* pk) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        pk[i] = key1[vs[i] >> 1];
}

// idcg[m], m = 0 .. L: every thread sums a contiguous stretch, the stretches are chained in thread order
__global__ __launch_bounds__(1024) void k_gm_idcg(double* idcg, int L) {
    __shared__ double part[1024];
    const int per = (L + 1023) / 1024;
    const int lo = threadIdx.x * per + 1;                      // r = lo .. hi - 1
    const int hi = min(lo + per, L + 1);
    double acc = 0.0;
    for (int r = lo; r < hi; ++r) acc += 1.0 / log2((double)r + 1.0);
    part[threadIdx.x] = acc;
    __syncthreads();
    double run = 0.0;
    for (int t = 0; t < (int)threadIdx.x; ++t) run += part[t];
    if (threadIdx.x == 0) idcg[0] = 0.0;
    for (int r = lo; r < hi; ++r) {
        run += 1.0 / log2((double)r + 1.0);
        idcg[r] = run;
    }
}

// Head / tail flags of element i = tile base + thread and the per-wave words of the tile.
struct GmFlags {
    bool valid, ghead, gtail, rhead, rtail;
    uint32_t label;
};
struct GmWaveWords {
    int last_rh[FX_GM_WAVES];      // last tie-run head of the wave (global position), -1: none
    int first_rt[FX_GM_WAVES];     // first tie-run tail, -1: none
    int first_gt[FX_GM_WAVES];     // first group tail, -1: none
};

__device__ __forceinline__ GmFlags gm_flags(const uint32_t* gs, const uint32_t* vs, const uint32_t* pk, int n,
                                            int i, GmWaveWords& ww, unsigned long long& m_gh,
                                            unsigned long long& m_gt, unsigned long long& m_rh,
                                            unsigned long long& m_rt) {
    GmFlags f;
    f.valid = i < n;
    f.ghead = f.gtail = f.rhead = f.rtail = false;
    f.label = 0u;
    if (f.valid) {
        const uint32_t g = gs[i], p = pk[i];
        f.label = vs[i] & 1u;
        f.ghead = (i == 0) || gs[i - 1] != g;
        f.rhead = f.ghead || pk[i - 1] != p;
        f.gtail = (i == n - 1) || gs[i + 1] != g;
        f.rtail = f.gtail || pk[i + 1] != p;
    }
    m_gh = __ballot(f.ghead);
    m_gt = __ballot(f.gtail);
    m_rh = __ballot(f.rhead);
    m_rt = __ballot(f.rtail);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wbase = i - lane;
    if (lane == 0) {
        ww.last_rh[wave] = m_rh ? wbase + 63 - __clzll((long long)m_rh) : -1;
        ww.first_rt[wave] = m_rt ? wbase + __ffsll((long long)m_rt) - 1 : -1;
        ww.first_gt[wave] = m_gt ? wbase + __ffsll((long long)m_gt) - 1 : -1;
    }
    __syncthreads();
    return f;
}

__global__ __launch_bounds__(FX_GM_TILE) void k_gm_tile_heads(const uint32_t* gs, const uint32_t* vs,
                                                              const uint32_t* pk, int n, int* t_last_rh,
                                                              int* t_first_rt, int* t_first_gt) {
    __shared__ GmWaveWords ww;
    unsigned long long m_gh, m_gt, m_rh, m_rt;
    gm_flags(gs, vs, pk, n, (int)blockIdx.x * FX_GM_TILE + (int)threadIdx.x, ww, m_gh, m_gt, m_rh, m_rt);
    if (threadIdx.x == 0) {
        int lrh = -1, frt = -1, fgt = -1;
        for (int w = 0; w < FX_GM_WAVES; ++w) {
            if (ww.last_rh[w] >= 0) lrh = ww.last_rh[w];
            if (frt < 0) frt = ww.first_rt[w];
            if (fgt < 0) fgt = ww.first_gt[w];
        }
        t_last_rh[blockIdx.x] = lrh;
        t_first_rt[blockIdx.x] = frt;
        t_first_gt[blockIdx.x] = fgt;
    }
}

// in place: t_last_rh[t] <- the last run head of the tiles before t; t_first_rt / t_first_gt[t] <- the first
// run / group tail of the tiles after t.  One workgroup; a thread owns a contiguous stretch of tiles.
__global__ __launch_bounds__(1024) void k_gm_tile_scan(int* t_last_rh, int* t_first_rt, int* t_first_gt,
                                                       int nt) {
    __shared__ int s_rh[1024], s_rt[1024], s_gt[1024];
    const int per = (nt + 1023) / 1024;
    const int lo = min((int)threadIdx.x * per, nt), hi = min(lo + per, nt);
    int lrh = -1, frt = -1, fgt = -1;
    for (int t = lo; t < hi; ++t) {
        if (t_last_rh[t] >= 0) lrh = t_last_rh[t];
        if (frt < 0) frt = t_first_rt[t];
        if (fgt < 0) fgt = t_first_gt[t];
    }
    s_rh[threadIdx.x] = lrh;
    s_rt[threadIdx.x] = frt;
    s_gt[threadIdx.x] = fgt;
    __syncthreads();
    int before = -1, after_rt = -1, after_gt = -1;
    for (int t = 0; t < (int)threadIdx.x; ++t)
        if (s_rh[t] >= 0) before = s_rh[t];
    for (int t = 1023; t > (int)threadIdx.x; --t) {
        if (s_rt[t] >= 0) after_rt = s_rt[t];
        if (s_gt[t] >= 0) after_gt = s_gt[t];
    }
    for (int t = lo; t < hi; ++t) {                            // exclusive prefix: forwards
        const int own = t_last_rh[t];
        t_last_rh[t] = before;
        if (own >= 0) before = own;
    }
    for (int t = hi - 1; t >= lo; --t) {                       // exclusive suffix: backwards
        const int own_rt = t_first_rt[t], own_gt = t_first_gt[t];
        t_first_rt[t] = after_rt;
        t_first_gt[t] = after_gt;
        if (own_rt >= 0) after_rt = own_rt;
        if (own_gt >= 0) after_gt = own_gt;
    }
}

// the (value, weight) vector of one finished group [S, E)
__device__ __forceinline__ void gm_finalize(const GmPart& p, int S, int E, const GmKs& ks, const double* idcg,
                                            double (&v)[FX_GM_NV]) {
    const unsigned long long n = (unsigned long long)(E - S), np = p.np;
    v[0] = v[1] = v[2] = v[3] = 0.0;
    if (np > 0ull && np < n) {
        const unsigned long long s2 = p.a - 2ull * (unsigned long long)S * np;    // twice the rank sum
        const double auc = (double)(s2 - np * (np + 1ull)) / (double)(2ull * np * (n - np));
        v[0] = auc * (double)n;
        v[1] = (double)n;
        v[2] = auc;
        v[3] = 1.0;
    }
    v[4] = p.mrr / ((double)np + 1e-12);
    v[5] = 1.0;
#pragma unroll
    for (int k = 0; k < FX_GM_MAX_K; ++k) {
        v[6 + k] = 0.0;
        if (k < ks.nk) {
            const unsigned long long m = np < (unsigned long long)ks.k[k] ? np : (unsigned long long)ks.k[k];
            v[6 + k] = p.dcg[k] / (idcg[m] + 1e-12);
        }
    }
}

// v summed over the workgroup's lanes in a fixed order -> out[FX_GM_NV] (thread 0 writes)
__device__ __forceinline__ void gm_block_sum(double (&v)[FX_GM_NV], double (*red)[FX_GM_NV], double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < FX_GM_NV; ++c) {
        const double s = fx_wave_sum(v[c]);
        if (lane == 0) red[wave][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < FX_GM_NV) {
        double s = 0.0;
        for (int w = 0; w < FX_GM_WAVES; ++w) s += red[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(FX_GM_TILE) void k_gm_segments(
    const uint32_t* gs, const uint32_t* vs, const uint32_t* pk, int n, GmKs ks, int kmax, const double* idcg,
    const int* t_prev_rh, const int* t_next_rt, const int* t_next_gt, GmPart* c_first, GmPart* c_own,
    int* c_own_s, int* c_own_e, double* tile_out) {
    __shared__ GmWaveWords ww;
    __shared__ double red[FX_GM_WAVES][FX_GM_NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (int)blockIdx.x * FX_GM_TILE + (int)threadIdx.x;
    const int chunk = (int)blockIdx.x * FX_GM_WAVES + wave;
    unsigned long long m_gh, m_gt, m_rh, m_rt;
    const GmFlags f = gm_flags(gs, vs, pk, n, i, ww, m_gh, m_gt, m_rh, m_rt);

    // ---- tie run [R0, R1) and group end E of this element --------------------------------------
    const unsigned long long upto = (2ull << lane) - 1ull;     // lanes <= this one
    int R0 = -1, R1 = -1, E = -1;
    if (m_rh & upto) R0 = i - lane + 63 - __clzll((long long)(m_rh & upto));
    if (m_rt >> lane) R1 = i + __ffsll((long long)(m_rt >> lane));
    if (m_gt >> lane) E = i + __ffsll((long long)(m_gt >> lane));
    if (f.valid) {
        for (int w = wave - 1; R0 < 0 && w >= 0; --w) R0 = ww.last_rh[w];
        if (R0 < 0) R0 = t_prev_rh[blockIdx.x];
        for (int w = wave + 1; R1 < 0 && w < FX_GM_WAVES; ++w)
            if (ww.first_rt[w] >= 0) R1 = ww.first_rt[w] + 1;
        if (R1 < 0) R1 = t_next_rt[blockIdx.x] + 1;
        for (int w = wave + 1; E < 0 && w < FX_GM_WAVES; ++w)
            if (ww.first_gt[w] >= 0) E = ww.first_gt[w] + 1;
        if (E < 0) E = t_next_gt[blockIdx.x] + 1;
    }

    // ---- this element's terms ---------------------------------------------------------------------
    GmPart p;
    p.a = 0ull;
    p.np = 0ull;
    p.mrr = 0.0;
#pragma unroll
    for (int k = 0; k < FX_GM_MAX_K; ++k) p.dcg[k] = 0.0;
    if (f.valid && f.label) {
        const int rank = E - i;
        p.a = (unsigned long long)R0 + (unsigned long long)R1 + 1ull;
        p.np = 1ull;
        p.mrr = 1.0 / (double)rank;
        if (rank <= kmax) {
            const double d = 1.0 / log2((double)rank + 1.0);
#pragma unroll
            for (int k = 0; k < FX_GM_MAX_K; ++k)
                if (k < ks.nk && rank <= ks.k[k]) p.dcg[k] = d;
        }
    }

    // ---- segmented inclusive scan over the wave: a segment starts at a group head (or at lane 0) ----------
    const bool has_head = (m_gh & upto) != 0ull;
    const int seg = has_head ? 63 - __clzll((long long)(m_gh & upto)) : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const bool take = lane - o >= seg;
        const unsigned long long a = __shfl_up(p.a, o, 64), c = __shfl_up(p.np, o, 64);
        const double r = __shfl_up(p.mrr, o, 64);
        if (take) {
            p.a += a;
            p.np += c;
            p.mrr += r;
        }
#pragma unroll
        for (int k = 0; k < FX_GM_MAX_K; ++k) {
            if (k < ks.nk) {
                const double d = __shfl_up(p.dcg[k], o, 64);
                if (take) p.dcg[k] += d;
            }
        }
    }

    // ---- the last lane of every segment holds its sums -----------------------------------------
    double v[FX_GM_NV];
#pragma unroll
    for (int c = 0; c < FX_GM_NV; ++c) v[c] = 0.0;
    bool own = false;
    if (f.valid && (f.gtail || lane == 63)) {
        if (!has_head) {
            c_first[chunk] = p;                    // a piece of a group that began in an earlier chunk
        } else if (f.gtail) {
            gm_finalize(p, i - lane + seg, E, ks, idcg, v);
        } else {                                   // head here, tail in a later chunk
            own = true;
            c_own[chunk] = p;
            c_own_s[chunk] = i - lane + seg;
            c_own_e[chunk] = E;
        }
    }
    if (lane == 63 && !own) c_own_s[chunk] = -1;
    gm_block_sum(v, red, tile_out + (int64_t)blockIdx.x * FX_GM_NV);
}

// one wave per chunk: the group whose head is in the chunk and whose tail is not
__global__ __launch_bounds__(FX_GM_TILE) void k_gm_fixup(GmKs ks, const double* idcg, const GmPart* c_first,
                                                         const GmPart* c_own, const int* c_own_s,
                                                         const int* c_own_e, double* tile_out) {
    __shared__ double red[FX_GM_WAVES][FX_GM_NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = (int)blockIdx.x * FX_GM_WAVES + wave;
    double v[FX_GM_NV];
#pragma unroll
    for (int c = 0; c < FX_GM_NV; ++c) v[c] = 0.0;
    const int S = c_own_s[chunk];
    if (S >= 0) {                                              // (wave-uniform)
        const int E = c_own_e[chunk];
        const int last = (E - 1) >> 6;                         // the chunk of the group's tail, > chunk
        GmPart p;
        p.a = 0ull;
        p.np = 0ull;
        p.mrr = 0.0;
#pragma unroll
        for (int k = 0; k < FX_GM_MAX_K; ++k) p.dcg[k] = 0.0;
        for (int c = chunk + 1 + lane; c <= last; c += 64) {
            const GmPart q = c_first[c];
            p.a += q.a;
            p.np += q.np;
            p.mrr += q.mrr;
#pragma unroll
            for (int k = 0; k < FX_GM_MAX_K; ++k)
                if (k < ks.nk) p.dcg[k] += q.dcg[k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            p.a += __shfl_xor(p.a, off, 64);
            p.np += __shfl_xor(p.np, off, 64);
        }
        p.mrr = fx_wave_sum(p.mrr);
#pragma unroll
        for (int k = 0; k < FX_GM_MAX_K; ++k)
            if (k < ks.nk) p.dcg[k] = fx_wave_sum(p.dcg[k]);
        if (lane == 0) {
            const GmPart q = c_own[chunk];
            p.a += q.a;
            p.np += q.np;
            p.mrr += q.mrr;
#pragma unroll
            for (int k = 0; k < FX_GM_MAX_K; ++k)
                if (k < ks.nk) p.dcg[k] += q.dcg[k];
            gm_finalize(p, S, E, ks, idcg, v);
        }
    }
    gm_block_sum(v, red, tile_out + (int64_t)blockIdx.x * FX_GM_NV);
}

// out: (sum value, sum weight) of gAUC | avgAUC | MRR | NDCG@K..., then the number of groups
__global__ __launch_bounds__(256) void k_gm_finish(const double* tile_out, int rows, int nk, double* out) {
    __shared__ double red[256];
    __shared__ double tot[FX_GM_NV];
    for (int c = 0; c < FX_GM_NV; ++c) {
        double acc = 0.0;
        for (int r = threadIdx.x; r < rows; r += 256) acc += tile_out[(int64_t)r * FX_GM_NV + c];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) tot[c] = red[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = tot[0];
        out[1] = tot[1];
        out[2] = tot[2];
        out[3] = tot[3];
        out[4] = tot[4];
        out[5] = tot[5];
        for (int k = 0; k < nk; ++k) {
            out[6 + 2 * k] = tot[6 + k];
            out[7 + 2 * k] = tot[5];
        }
        out[6 + 2 * nk] = tot[5];
    }
}

inline size_t gm_up(size_t x) { return (x + 255) / 256 * 256; }

// workspace layout: 7 n-word arrays | pk | idcg [n + 1] | 3 per-tile words | per-chunk pieces and spans |
// per-tile results (segments, fixup) | the sort's temp
struct GmLayout {
    int nt, nc;
    size_t arr, idcg, tile_words, parts, spans, tile_out, sort, total;
};

inline GmLayout gm_layout(int64_t n) {
    GmLayout L;
    L.nt = (int)fx_ceil_div(n, FX_GM_TILE);
    L.nc = L.nt * FX_GM_WAVES;
    L.arr = gm_up((size_t)n * 4);
    L.idcg = gm_up(((size_t)n + 1) * sizeof(double));
    L.tile_words = gm_up((size_t)L.nt * sizeof(int));
    L.parts = gm_up((size_t)L.nc * sizeof(GmPart));
    L.spans = gm_up((size_t)L.nc * sizeof(int));
    L.tile_out = gm_up((size_t)2 * L.nt * FX_GM_NV * sizeof(double));
    L.sort = gm_up(fx_sort_temp_bytes(n));
    L.total = 8 * L.arr + L.idcg + 3 * L.tile_words + 2 * L.parts + 2 * L.spans + L.tile_out + L.sort;
    return L;
}

}  // namespace

extern "C" size_t fx_group_metrics_workspace_bytes(int64_t n) {
    if (n <= 0) return 256;
    return gm_layout(n).total + 256;
}

extern "C" int fx_group_metrics(const float* y_pred, const float* y_true, const uint32_t* group_key,
                                int32_t key_bits, int64_t n, const int32_t* ndcg_ks, int32_t n_ks,
                                void* workspace, size_t workspace_bytes, double* out, fx_stream_t stream) {
    FX_CHECK_ARG(n >= 1 && n <= ((int64_t)1 << 26), "fx_group_metrics: n=%lld not in [1, 2^26]", (long long)n);
    FX_CHECK_ARG(key_bits >= 1 && key_bits <= 32, "fx_group_metrics: key_bits=%d not in [1, 32]", key_bits);
    FX_CHECK_ARG(n_ks >= 0 && n_ks <= FX_GM_MAX_K, "fx_group_metrics: %d NDCG cut-offs (at most %d)", n_ks,
                 FX_GM_MAX_K);
    FX_CHECK_ARG(n_ks == 0 || ndcg_ks, "fx_group_metrics: null ndcg_ks");
    FX_CHECK_ARG(y_pred && y_true && group_key && workspace && out, "fx_group_metrics: null pointer");
    GmKs ks;
    ks.nk = n_ks;
    int kmax = 0;
    for (int k = 0; k < FX_GM_MAX_K; ++k) {
        ks.k[k] = k < n_ks ? ndcg_ks[k] : 0;
        FX_CHECK_ARG(k >= n_ks || ks.k[k] >= 1, "fx_group_metrics: NDCG cut-off %d < 1", ks.k[k]);
        if (ks.k[k] > kmax) kmax = ks.k[k];
    }
    const GmLayout L = gm_layout(n);
    FX_CHECK_ARG(workspace_bytes >= L.total, "fx_group_metrics: workspace too small");
    char* w = reinterpret_cast<char*>(workspace);
    uint32_t* a[8];
    for (int j = 0; j < 8; ++j) a[j] = reinterpret_cast<uint32_t*>(w + (size_t)j * L.arr);
    w += 8 * L.arr;
    double* idcg = reinterpret_cast<double*>(w);
    w += L.idcg;
    int* t_rh = reinterpret_cast<int*>(w);
    int* t_rt = reinterpret_cast<int*>(w + L.tile_words);
    int* t_gt = reinterpret_cast<int*>(w + 2 * L.tile_words);
    w += 3 * L.tile_words;
    GmPart* c_first = reinterpret_cast<GmPart*>(w);
    GmPart* c_own = reinterpret_cast<GmPart*>(w + L.parts);
    w += 2 * L.parts;
    int* c_own_s = reinterpret_cast<int*>(w);
    int* c_own_e = reinterpret_cast<int*>(w + L.spans);
    w += 2 * L.spans;
    double* tile_out = reinterpret_cast<double*>(w);
    w += L.tile_out;
    void* temp = w;
    hipStream_t s = fx_hip_stream(stream);

    int64_t blocks = fx_ceil_div(n, 256);
    if (blocks > 8192) blocks = 8192;
    const dim3 flat((unsigned)blocks), tiles((unsigned)L.nt);
    // sort 1: (a0, a1) -> (a2, a3), scratch (a4, a5)
    hipLaunchKernelGGL(k_gm_keys, flat, dim3(256), 0, s, y_pred, y_true, n, a[0], a[1]);
    FX_CHECK_LAUNCH();
    int rc = fx_sort_pairs_u32(a[0], a[1], a[2], a[3], a[4], a[5], n, 32u, temp, false, s);
    if (rc != FX_OK) return rc;
    // sort 2: (a0, a1) -> (a4, a5), scratch (a6, a7); a2 (the sorted prediction keys) stays
    const uint32_t mask = key_bits >= 32 ? 0xFFFFFFFFu : ((1u << key_bits) - 1u);
    hipLaunchKernelGGL(k_gm_gkeys, flat, dim3(256), 0, s, group_key, a[3], n, mask, a[0], a[1]);
    FX_CHECK_LAUNCH();
    rc = fx_sort_pairs_u32(a[0], a[1], a[4], a[5], a[6], a[7], n, (unsigned)key_bits, temp, false, s);
    if (rc != FX_OK) return rc;
    const uint32_t *gs = a[4], *vs = a[5];
    uint32_t* pk = a[0];
    hipLaunchKernelGGL(k_gm_gather, flat, dim3(256), 0, s, a[2], vs, n, pk);
    const int idcg_len = (int)((int64_t)kmax < n ? (int64_t)kmax : n);
    hipLaunchKernelGGL(k_gm_idcg, dim3(1), dim3(1024), 0, s, idcg, idcg_len);
    hipLaunchKernelGGL(k_gm_tile_heads, tiles, dim3(FX_GM_TILE), 0, s, gs, vs, pk, (int)n, t_rh, t_rt, t_gt);
    hipLaunchKernelGGL(k_gm_tile_scan, dim3(1), dim3(1024), 0, s, t_rh, t_rt, t_gt, L.nt);
    FX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gm_segments, tiles, dim3(FX_GM_TILE), 0, s, gs, vs, pk, (int)n, ks, kmax, idcg, t_rh,
                       t_rt, t_gt, c_first, c_own, c_own_s, c_own_e, tile_out);
    hipLaunchKernelGGL(k_gm_fixup, tiles, dim3(FX_GM_TILE), 0, s, ks, idcg, c_first, c_own, c_own_s, c_own_e,
                       tile_out + (int64_t)L.nt * FX_GM_NV);
    hipLaunchKernelGGL(k_gm_finish, dim3(1), dim3(256), 0, s, tile_out, 2 * L.nt, (int)n_ks, out);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
