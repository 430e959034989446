// fx_gru.hip — DIEN's recurrent layers and its attention scores (model_zoo/DIEN/src/DIEN.py:241-294, 342-370,
// 373-448; torch.nn.GRU's packed weight_ih_l0 / weight_hh_l0):
//     one layer over X [B, L, H] (up to two column parts, read in place), positions 0 .. len-1 of each sample,
//     len[b] = the number of non-zero ids of the first sequence field (what pack_padded_sequence keeps):
//         gx = W_ih x_t + b_ih,  gh = W_hh h + b_hh,  three chunks of H each
//         r = sigmoid(gx_r + gh_r),  n = tanh(gx_n + r * gh_n),  h' = h + g * (n - h)
//         GRU   chunks (r, z, n):  g = 1 - sigmoid(gx_z + gh_z)          (torch.nn.GRU)
//         AGRU  chunks (u, r, n):  g = a_t                               (DIEN.py:399-408; the u chunk is unused)
//         AUGRU chunks (u, r, n):  g = sigmoid(gx_u + gh_u) * a_t        (DIEN.py:437-448)
//     states [B, L, H] (zero past len) and the final state [B, H] (zero for len = 0).
//     scores: s[b, t] = (interest[b, t] W) . target[b]  (W [H, H], or none: the plain dot), times mask[b, t],
//     then optionally + -1e9 (1 - mask) and a soft-max over all L positions (DIEN.py:353-370).
// The recurrence: a workgroup of 256 threads owns a tile of TB = 2 * (256 / H) samples for the whole sequence.
// W_ih and W_hh sit transposed in LDS (row stride 3H + 1: lanes that walk the units and lanes that walk the inputs
// both hit distinct banks), x_t and h in LDS (double buffered: one barrier per step), thread (sample pair, unit j)
// forms the six dot products of its unit for its two samples in fp32 FMAs.  The steps stop at the tile's longest
// history.  No atomics: two launches give the same bits.
// The backward is back-propagation through time in one launch: it re-reads the saved states (h_{t-1} = states[t-1]),
// recomputes the gates, carries dh in LDS, writes dX through the parts' own strides and d(scores), and keeps the
// two weight-gradient matrices in registers over the workgroup's tiles and steps (entry e belongs to thread
// e % 256); one row of partial sums per workgroup, added in fixed order by fx_rowsum.
#include "fx_rowsum.h"
#include "fx_seq_parts.h"

#define GR_T 256
#define GR_S 2               // samples per thread
#define GR_MAX_H 64
#define GR_MAX_L 256
#define GR_FWD_GRID 1024
#define GR_BWD_GRID 256      // = rows of the weight-gradient partials
#define GR_LDS_MAX (160 * 1024)
#define SC_WAVES 4           // samples per workgroup pass of the score kernels
#define SC_GRID 256
#define SC_PER_LANE (GR_MAX_L / 64)

enum { GR_GRU = 0, GR_AGRU = 1, GR_AUGRU = 2 };

struct GruArgs {
    fx_seq_parts x;          // the layer's input: the sequence side
    fx_seq_parts dx;         // where its gradient goes (backward; a null part is skipped)
    const int32_t* ids;      // [B, L] ids of the first sequence field, row stride ids_ld
    int64_t ids_ld;
    const float* scores;     // [B, L] a_t (AGRU, AUGRU)
    int64_t B;
    int L, H, mode, np, D, NG, TB;
    const float* w_ih;       // [3H, H]
    const float* w_hh;
    const float* b_ih;       // [3H]
    const float* b_hh;
    float* states;           // forward out [B, L, H]
    float* fin;              // forward out [B, H]
    const float* hs;         // backward: the saved states
    const float* d_states;   // nullable
    const float* d_final;    // nullable
    float* d_scores;         // [B, L]
    float* partial;          // [grid, n_grad]
    int64_t n_grad;
};

__device__ __forceinline__ float gr_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

struct GruLds {
    float* sWi;      // [H][3H + 1]: W_ih transposed
    float* sWh;
    float* sBias;    // b_ih | b_hh
    float* sX;       // 2 x [TB][H | 1]
    float* sH;       // 2 x [TB][H | 1]
    int* sLen;       // [TB]
    float* rest;
};

__device__ __forceinline__ GruLds gr_lds(const GruArgs& p, float* smem) {
    const int H = p.H, WS = 3 * H + 1, HS = H | 1;
    GruLds l;
    l.sWi = smem;
    l.sWh = l.sWi + H * WS;
    l.sBias = l.sWh + H * WS;
    l.sX = l.sBias + 6 * H;
    l.sH = l.sX + 2 * p.TB * HS;
    l.sLen = reinterpret_cast<int*>(l.sH + 2 * p.TB * HS);
    l.rest = reinterpret_cast<float*>(l.sLen + p.TB);
    return l;
}

__device__ __forceinline__ void gr_stage_weights(const GruArgs& p, const GruLds& l) {
    const int H = p.H, H3 = 3 * H, WS = H3 + 1;
    for (int e = threadIdx.x; e < H3 * H; e += GR_T) {
        const int cj = e / H, k = e - cj * H;
        l.sWi[k * WS + cj] = p.w_ih[e];
        l.sWh[k * WS + cj] = p.w_hh[e];
    }
    for (int e = threadIdx.x; e < H3; e += GR_T) {
        l.sBias[e] = p.b_ih[e];
        l.sBias[H3 + e] = p.b_hh[e];
    }
}

// the lengths of the tile's samples (0 past the batch) -> sLen; returns the longest.  Two barriers inside.
__device__ __forceinline__ int gr_lengths(const GruArgs& p, int64_t b0, int* sLen) {
    __syncthreads();
    if ((int)threadIdx.x < p.TB) {
        const int64_t b = b0 + threadIdx.x;
        int n = 0;
        if (b < p.B)
            for (int t = 0; t < p.L; ++t) n += p.ids[b * p.ids_ld + t] != 0 ? 1 : 0;
        sLen[threadIdx.x] = n;
    }
    __syncthreads();
    int mx = 0;
    for (int s = 0; s < p.TB; ++s) mx = sLen[s] > mx ? sLen[s] : mx;
    return mx;
}

// the six pre-activation sums of unit j for this thread's samples: a[i][0..2] = gx chunks, a[i][3..5] = gh chunks
__device__ __forceinline__ void gr_gates(const GruLds& l, int H, int j, int s0, const float* sX, const float* sH,
                                         float (&a)[GR_S][6]) {
    const int H3 = 3 * H, WS = H3 + 1, HS = H | 1;
#pragma unroll
    for (int i = 0; i < GR_S; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[i][c] = l.sBias[c * H + j];
            a[i][3 + c] = l.sBias[H3 + c * H + j];
        }
    for (int k = 0; k < H; ++k) {
        float wi[3], wh[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            wi[c] = l.sWi[k * WS + c * H + j];
            wh[c] = l.sWh[k * WS + c * H + j];
        }
#pragma unroll
        for (int i = 0; i < GR_S; ++i) {
            const float xv = sX[(s0 + i) * HS + k], hv = sH[(s0 + i) * HS + k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a[i][c] = fmaf(wi[c], xv, a[i][c]);
                a[i][3 + c] = fmaf(wh[c], hv, a[i][3 + c]);
            }
        }
    }
}

__global__ __launch_bounds__(GR_T) void k_gru_fwd(GruArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, HS = H | 1, TB = p.TB, L = p.L;
    const GruLds l = gr_lds(p, smem);
    gr_stage_weights(p, l);
    const int sg = threadIdx.x / H, j = threadIdx.x - sg * H, s0 = sg * GR_S;
    const bool live = sg < p.NG;
    const int cr = p.mode == GR_GRU ? 0 : 1, cg = p.mode == GR_GRU ? 1 : 0;
    const int64_t tiles = (p.B + TB - 1) / TB;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TB;
        const int maxlen = gr_lengths(p, b0, l.sLen);
        int len[GR_S];
        float h[GR_S];
#pragma unroll
        for (int i = 0; i < GR_S; ++i) {
            len[i] = live ? l.sLen[s0 + i] : 0;
            h[i] = 0.f;
            if (live) {
                int part;
                const int64_t off = fx_parts_seq_off(p.x, p.D, b0 + s0 + i, 0, j, part);
                l.sX[(s0 + i) * HS + j] = len[i] > 0 ? p.x.seq[part][off] : 0.f;
                l.sH[(s0 + i) * HS + j] = 0.f;
            }
        }
        __syncthreads();
        for (int t = 0; t < maxlen; ++t) {
            const float* sX = l.sX + (t & 1) * TB * HS;
            const float* sH = l.sH + (t & 1) * TB * HS;
            float* sXn = l.sX + ((t + 1) & 1) * TB * HS;
            float* sHn = l.sH + ((t + 1) & 1) * TB * HS;
            if (live) {
                float xn[GR_S], at[GR_S];
#pragma unroll
                for (int i = 0; i < GR_S; ++i) {         // the next step's input, under this step's arithmetic
                    const int64_t b = b0 + s0 + i;
                    xn[i] = 0.f;
                    at[i] = 0.f;
                    if (t + 1 < len[i]) {
                        int part;
                        const int64_t off = fx_parts_seq_off(p.x, p.D, b, t + 1, j, part);
                        xn[i] = p.x.seq[part][off];
                    }
                    if (t < len[i] && p.mode != GR_GRU) at[i] = p.scores[b * L + t];
                }
                float a[GR_S][6];
                gr_gates(l, H, j, s0, sX, sH, a);
#pragma unroll
                for (int i = 0; i < GR_S; ++i) {
                    const int64_t b = b0 + s0 + i;
                    if (t < len[i]) {
                        const float r = gr_sigmoid(a[i][cr] + a[i][3 + cr]);
                        const float n = tanhf(fmaf(r, a[i][5], a[i][2]));
                        float g;
                        if (p.mode == GR_GRU) g = 1.f - gr_sigmoid(a[i][cg] + a[i][3 + cg]);
                        else if (p.mode == GR_AGRU) g = at[i];
                        else g = gr_sigmoid(a[i][cg] + a[i][3 + cg]) * at[i];
                        h[i] = fmaf(g, n - h[i], h[i]);
                        p.states[(b * L + t) * H + j] = h[i];
                    } else if (b < p.B) {
                        p.states[(b * L + t) * H + j] = 0.f;
                    }
                    sHn[(s0 + i) * HS + j] = h[i];
                    sXn[(s0 + i) * HS + j] = xn[i];
                }
            }
            __syncthreads();
        }
        if (live) {
#pragma unroll
            for (int i = 0; i < GR_S; ++i) {
                const int64_t b = b0 + s0 + i;
                if (b < p.B) {
                    p.fin[b * H + j] = h[i];
                    for (int t = maxlen; t < L; ++t) p.states[(b * L + t) * H + j] = 0.f;
                }
            }
        }
    }
}

// R: entries per thread of one weight-gradient matrix (3 H H <= 256 R)
template <int R>
__global__ __launch_bounds__(GR_T) void k_gru_bwd(GruArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, H3 = 3 * H, WS = H3 + 1, HS = H | 1, GS = H3 | 1, TB = p.TB, L = p.L;
    const GruLds l = gr_lds(p, smem);
    float* sDh = l.rest;                 // [TB][HS]   dh carried to the step before
    float* sGX = sDh + TB * HS;          // [TB][GS]   d gx of this step
    float* sGH = sGX + TB * GS;          // [TB][GS]   d gh
    float* sDa = sGH + TB * GS;          // [TB][HS]   unit j's share of d a_t
    gr_stage_weights(p, l);
    const int sg = threadIdx.x / H, j = threadIdx.x - sg * H, s0 = sg * GR_S;
    const bool live = sg < p.NG;
    const int cr = p.mode == GR_GRU ? 0 : 1, cg = p.mode == GR_GRU ? 1 : 0;
    const int q = GR_T / H, rem = GR_T - q * H;       // entry e + 256 is (cj + q, k + rem), carried
    float accI[R], accH[R];
#pragma unroll
    for (int r = 0; r < R; ++r) accI[r] = accH[r] = 0.f;
    float dbi = 0.f, dbh = 0.f;
    const int64_t tiles = (p.B + TB - 1) / TB;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TB;
        const int maxlen = gr_lengths(p, b0, l.sLen);
        int len[GR_S];
#pragma unroll
        for (int i = 0; i < GR_S; ++i) {
            len[i] = live ? l.sLen[s0 + i] : 0;
            if (live) {
                const int64_t b = b0 + s0 + i;
                const int t = maxlen - 1;
                float xv = 0.f, hv = 0.f;
                if (t >= 0 && t < len[i]) {
                    int part;
                    const int64_t off = fx_parts_seq_off(p.x, p.D, b, t, j, part);
                    xv = p.x.seq[part][off];
                    if (t > 0) hv = p.hs[(b * L + t - 1) * H + j];
                }
                const int buf = (t & 1) * TB * HS;
                l.sX[buf + (s0 + i) * HS + j] = xv;
                l.sH[buf + (s0 + i) * HS + j] = hv;
                sDh[(s0 + i) * HS + j] = 0.f;
            }
        }
        __syncthreads();
        for (int t = maxlen - 1; t >= 0; --t) {
            const float* sX = l.sX + (t & 1) * TB * HS;
            const float* sH = l.sH + (t & 1) * TB * HS;
            float* sXn = l.sX + ((t + 1) & 1) * TB * HS;
            float* sHn = l.sH + ((t + 1) & 1) * TB * HS;
            float xn[GR_S], hn[GR_S], dhd[GR_S];
            if (live) {
                float at[GR_S], dh[GR_S];
#pragma unroll
                for (int i = 0; i < GR_S; ++i) {         // step t - 1's input and the loads of this step
                    const int64_t b = b0 + s0 + i;
                    xn[i] = hn[i] = at[i] = 0.f;
                    dh[i] = sDh[(s0 + i) * HS + j];
                    if (t - 1 >= 0 && t - 1 < len[i]) {
                        int part;
                        const int64_t off = fx_parts_seq_off(p.x, p.D, b, t - 1, j, part);
                        xn[i] = p.x.seq[part][off];
                        if (t - 1 > 0) hn[i] = p.hs[(b * L + t - 2) * H + j];
                    }
                    if (t < len[i]) {
                        if (p.mode != GR_GRU) at[i] = p.scores[b * L + t];
                        if (p.d_states != nullptr) dh[i] += p.d_states[(b * L + t) * H + j];
                        if (p.d_final != nullptr && t == len[i] - 1) dh[i] += p.d_final[b * H + j];
                    }
                }
                float a[GR_S][6];
                gr_gates(l, H, j, s0, sX, sH, a);
#pragma unroll
                for (int i = 0; i < GR_S; ++i) {
                    float dg_pre = 0.f, dr_pre = 0.f, dn_pre = 0.f, dhn = 0.f, da = 0.f;
                    dhd[i] = 0.f;
                    if (t < len[i]) {
                        const float hp = sH[(s0 + i) * HS + j];
                        const float r = gr_sigmoid(a[i][cr] + a[i][3 + cr]);
                        const float n = tanhf(fmaf(r, a[i][5], a[i][2]));
                        float g, u = 0.f;
                        if (p.mode == GR_AGRU) {
                            g = at[i];
                        } else {
                            u = gr_sigmoid(a[i][cg] + a[i][3 + cg]);
                            g = p.mode == GR_GRU ? 1.f - u : u * at[i];
                        }
                        const float dgate = dh[i] * (n - hp);
                        dn_pre = dh[i] * g * (1.f - n * n);
                        dhn = dn_pre * r;
                        dr_pre = dn_pre * a[i][5] * r * (1.f - r);
                        dhd[i] = dh[i] * (1.f - g);
                        if (p.mode == GR_GRU) {
                            dg_pre = -dgate * u * (1.f - u);
                        } else if (p.mode == GR_AGRU) {
                            da = dgate;
                        } else {
                            da = dgate * u;
                            dg_pre = dgate * at[i] * u * (1.f - u);
                        }
                    }
                    float* gx = sGX + (s0 + i) * GS;
                    float* gh = sGH + (s0 + i) * GS;
                    gx[cg * H + j] = dg_pre;
                    gh[cg * H + j] = dg_pre;
                    gx[cr * H + j] = dr_pre;
                    gh[cr * H + j] = dr_pre;
                    gx[2 * H + j] = dn_pre;
                    gh[2 * H + j] = dhn;
                    sDa[(s0 + i) * HS + j] = da;
                }
            }
            __syncthreads();
            if (live) {                                  // thread (sample, input k = j): dX and the dh of step t - 1
#pragma unroll
                for (int i = 0; i < GR_S; ++i) {
                    const float* gx = sGX + (s0 + i) * GS;
                    const float* gh = sGH + (s0 + i) * GS;
                    float dxv = 0.f, dhv = dhd[i];
                    for (int c = 0; c < H3; ++c) {
                        dxv = fmaf(gx[c], l.sWi[j * WS + c], dxv);
                        dhv = fmaf(gh[c], l.sWh[j * WS + c], dhv);
                    }
                    const int64_t b = b0 + s0 + i;
                    if (b < p.B) {
                        int part;
                        const int64_t off = fx_parts_seq_off(p.dx, p.D, b, t, j, part);
                        fx_parts_put(p.dx.seq[part], off, dxv, false);
                    }
                    sDh[(s0 + i) * HS + j] = dhv;
                    sXn[(s0 + i) * HS + j] = xn[i];
                    sHn[(s0 + i) * HS + j] = hn[i];
                }
            }
            {                                            // dW_ih += d gx^T x_t,  dW_hh += d gh^T h_{t-1}
                int cj = threadIdx.x / H, k = threadIdx.x - cj * H;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (cj < H3) {
                        float si = 0.f, sh = 0.f;
                        for (int s = 0; s < TB; ++s) {
                            si = fmaf(sGX[s * GS + cj], sX[s * HS + k], si);
                            sh = fmaf(sGH[s * GS + cj], sH[s * HS + k], sh);
                        }
                        accI[r] += si;
                        accH[r] += sh;
                    }
                    cj += q;
                    k += rem;
                    if (k >= H) {
                        k -= H;
                        ++cj;
                    }
                }
            }
            if ((int)threadIdx.x < H3) {
                float si = 0.f, sh = 0.f;
                for (int s = 0; s < TB; ++s) {
                    si += sGX[s * GS + threadIdx.x];
                    sh += sGH[s * GS + threadIdx.x];
                }
                dbi += si;
                dbh += sh;
            }
            if (p.d_scores != nullptr && (int)threadIdx.x < TB && b0 + threadIdx.x < p.B) {
                float s = 0.f;
                for (int c = 0; c < H; ++c) s += sDa[threadIdx.x * HS + c];
                p.d_scores[(b0 + threadIdx.x) * L + t] = s;
            }
            __syncthreads();
        }
        // past the tile's longest history nothing has a gradient
        if (live) {
#pragma unroll
            for (int i = 0; i < GR_S; ++i) {
                const int64_t b = b0 + s0 + i;
                if (b >= p.B) continue;
                for (int t = maxlen; t < L; ++t) {
                    int part;
                    const int64_t off = fx_parts_seq_off(p.dx, p.D, b, t, j, part);
                    fx_parts_put(p.dx.seq[part], off, 0.f, false);
                    if (j == 0 && p.d_scores != nullptr) p.d_scores[b * L + t] = 0.f;
                }
            }
        }
    }
    float* row = p.partial + (int64_t)blockIdx.x * p.n_grad;
    {
        int e = threadIdx.x;
#pragma unroll
        for (int r = 0; r < R; ++r, e += GR_T) {
            if (e < H3 * H) {
                row[e] = accI[r];
                row[H3 * H + e] = accH[r];
            }
        }
    }
    if ((int)threadIdx.x < H3) {
        row[2 * H3 * H + threadIdx.x] = dbi;
        row[2 * H3 * H + H3 + threadIdx.x] = dbh;
    }
}

static inline int64_t gr_n_grad(int H) { return 6 * (int64_t)H * H + 6 * (int64_t)H; }
static inline int gr_tile(int H) { return GR_S * (GR_T / H); }
static inline int64_t gr_tiles(int64_t B, int H) { return (B + gr_tile(H) - 1) / gr_tile(H); }

static inline size_t gr_lds_floats(int H, bool backward) {
    const size_t TB = gr_tile(H), HS = H | 1, GS = (3 * H) | 1;
    size_t n = 2 * (size_t)H * (3 * H + 1) + 6 * H + 4 * TB * HS + TB;
    if (backward) n += 2 * TB * HS + 2 * TB * GS;
    return n;
}

static int gr_check(const char* who, const fx_seq_parts* x, const int32_t* ids, int64_t ids_ld, const float* scores,
                    int64_t B, int32_t L, int32_t H, int32_t mode, const float* w_ih, const float* w_hh,
                    const float* b_ih, const float* b_hh) {
    FX_CHECK_ARG(x, "%s: null input description", who);
    FX_CHECK_ARG(H >= 4 && H <= GR_MAX_H && H % 4 == 0, "%s: H=%d, limit 4 <= H <= 64 and H %% 4 == 0", who, H);
    FX_CHECK_ARG(L >= 1 && L <= GR_MAX_L, "%s: L=%d, limit 1 <= L <= 256", who, L);
    FX_CHECK_ARG(mode >= GR_GRU && mode <= GR_AUGRU, "%s: mode=%d", who, mode);
    FX_CHECK_ARG(x->n_parts >= 1 && x->n_parts <= 2 && x->D >= 1 && x->D * x->n_parts == H,
                 "%s: H=%d is not n_parts=%d (1 or 2) * D=%d", who, H, x->n_parts, x->D);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    if (B == 0) return FX_OK;
    for (int i = 0; i < x->n_parts; ++i)
        if (int st = fx_parts_check_seq(who, "part", x, i, x->D, L, false)) return st;
    FX_CHECK_ARG(ids && ids_ld >= L, "%s: null ids or ids stride %lld < L", who, (long long)ids_ld);
    FX_CHECK_ARG(mode == GR_GRU || scores, "%s: null scores", who);
    FX_CHECK_ARG(w_ih && w_hh && b_ih && b_hh, "%s: null weight or bias", who);
    return FX_OK;
}

static GruArgs gr_args(const fx_seq_parts* x, const int32_t* ids, int64_t ids_ld, const float* scores, int64_t B,
                       int32_t L, int32_t H, int32_t mode, const float* w_ih, const float* w_hh, const float* b_ih,
                       const float* b_hh) {
    GruArgs p;
    memset(&p, 0, sizeof(p));
    p.x = *x;
    p.ids = ids; p.ids_ld = ids_ld; p.scores = scores; p.B = B;
    p.L = L; p.H = H; p.mode = mode; p.np = x->n_parts; p.D = x->D;
    p.NG = GR_T / H; p.TB = gr_tile(H);
    p.w_ih = w_ih; p.w_hh = w_hh; p.b_ih = b_ih; p.b_hh = b_hh;
    return p;
}

template <auto Kernel, typename Args>
static int gr_launch(const Args& p, unsigned grid, size_t lds, hipStream_t s) {
    static const hipError_t lds_ok = fx_allow_lds(Kernel, GR_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(GR_T), lds, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" void fx_gru_limits(int32_t* limits) {
    limits[0] = GR_MAX_H;
    limits[1] = GR_MAX_L;
    limits[2] = GR_FWD_GRID;
    limits[3] = GR_BWD_GRID;
}

extern "C" int32_t fx_gru_tile_rows(int32_t H) { return H >= 4 && H <= GR_MAX_H ? gr_tile(H) : 0; }

extern "C" int64_t fx_gru_grad_floats(int32_t H) { return gr_n_grad(H); }

extern "C" int64_t fx_gru_workspace_floats(int64_t B, int32_t H) {
    if (H < 4 || H > GR_MAX_H) return 0;
    const int64_t tiles = gr_tiles(B > 0 ? B : 1, H);
    return (tiles < GR_BWD_GRID ? tiles : GR_BWD_GRID) * fx_al4(gr_n_grad(H));
}

extern "C" int fx_gru_seq_fwd(const fx_seq_parts* x, const int32_t* ids, int64_t ids_ld, const float* scores,
                              int64_t B, int32_t L, int32_t H, int32_t mode, const float* w_ih, const float* w_hh,
                              const float* b_ih, const float* b_hh, float* states, float* final_state,
                              fx_stream_t stream) {
    if (int st = gr_check("fx_gru_seq_fwd", x, ids, ids_ld, scores, B, L, H, mode, w_ih, w_hh, b_ih, b_hh)) return st;
    FX_CHECK_ARG(B == 0 || (states && final_state), "fx_gru_seq_fwd: null states / final state");
    if (B == 0) return FX_OK;
    GruArgs p = gr_args(x, ids, ids_ld, scores, B, L, H, mode, w_ih, w_hh, b_ih, b_hh);
    p.states = states;
    p.fin = final_state;
    const int64_t tiles = gr_tiles(B, H);
    const unsigned grid = (unsigned)(tiles < GR_FWD_GRID ? tiles : GR_FWD_GRID);
    return gr_launch<k_gru_fwd>(p, grid, 4 * gr_lds_floats(H, false), fx_hip_stream(stream));
}

static int gr_launch_bwd(const GruArgs& p, unsigned grid, size_t lds, hipStream_t s) {
    const int need = (3 * p.H * p.H + GR_T - 1) / GR_T;
    if (need <= 1) return gr_launch<k_gru_bwd<1>>(p, grid, lds, s);
    if (need <= 3) return gr_launch<k_gru_bwd<3>>(p, grid, lds, s);
    if (need <= 7) return gr_launch<k_gru_bwd<7>>(p, grid, lds, s);
    if (need <= 12) return gr_launch<k_gru_bwd<12>>(p, grid, lds, s);
    if (need <= 27) return gr_launch<k_gru_bwd<27>>(p, grid, lds, s);
    return gr_launch<k_gru_bwd<48>>(p, grid, lds, s);
}

extern "C" int fx_gru_seq_bwd(const fx_seq_parts* x, const int32_t* ids, int64_t ids_ld, const float* scores,
                              int64_t B, int32_t L, int32_t H, int32_t mode, const float* w_ih, const float* w_hh,
                              const float* b_ih, const float* b_hh, const float* states, const float* d_states,
                              const float* d_final, const fx_seq_parts* dx, float* d_scores, float* grads,
                              float* workspace, fx_stream_t stream) {
    if (int st = gr_check("fx_gru_seq_bwd", x, ids, ids_ld, scores, B, L, H, mode, w_ih, w_hh, b_ih, b_hh)) return st;
    FX_CHECK_ARG(B > 0, "fx_gru_seq_bwd: B=%lld", (long long)B);
    FX_CHECK_ARG(states && dx && grads && workspace, "fx_gru_seq_bwd: null states / gradient description / grads / "
                 "workspace");
    FX_CHECK_ARG(d_states || d_final, "fx_gru_seq_bwd: neither d_states nor d_final");
    FX_CHECK_ARG(fx_al16(workspace), "fx_gru_seq_bwd: the workspace is not 16-byte aligned");
    FX_CHECK_ARG(dx->n_parts == x->n_parts && dx->D == x->D, "fx_gru_seq_bwd: the gradient's parts differ from the "
                 "input's");
    for (int i = 0; i < x->n_parts; ++i)
        if (int st = fx_parts_check_seq("fx_gru_seq_bwd", "gradient of part", dx, i, x->D, L, true)) return st;
    GruArgs p = gr_args(x, ids, ids_ld, scores, B, L, H, mode, w_ih, w_hh, b_ih, b_hh);
    p.dx = *dx;
    p.hs = states;
    p.d_states = d_states;
    p.d_final = d_final;
    p.d_scores = mode == GR_GRU ? nullptr : d_scores;
    const int64_t n = gr_n_grad(H), n4 = fx_al4(n);
    p.partial = workspace;
    p.n_grad = n4;
    const int64_t tiles = gr_tiles(B, H);
    const unsigned grid = (unsigned)(tiles < GR_BWD_GRID ? tiles : GR_BWD_GRID);
    const size_t lds = 4 * gr_lds_floats(H, true);
    FX_CHECK_ARG(lds <= GR_LDS_MAX, "fx_gru_seq_bwd: %zu bytes of LDS", lds);
    hipStream_t s = fx_hip_stream(stream);
    if (int st = gr_launch_bwd(p, grid, lds, s)) return st;
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)grid, n4, fx_rowsum_out(grads, n));
}

// ---- the attention scores ---------------------------------------------------------------------------------
struct ScoreArgs {
    const float* I;          // interest [B, L, H], contiguous
    fx_seq_parts tgt;
    fx_seq_parts dtgt;      // backward; a null part is skipped
    const int32_t* ids;
    int64_t ids_ld;
    int64_t B;
    int L, H, D, softmax;
    const float* W;          // [H, H] or null (dot)
    float* S;                // forward out [B, L]
    const float* P;          // backward: the forward's output
    const float* dS;
    float* dI;               // [B, L, H] or null
    float* partial;          // [grid, n_grad]
    int64_t n_grad;          // H H, 4-aligned
};

struct ScoreLds {
    float* sW;       // [H][H | 1]
    float* sT;       // [waves][H]   target
    float* sV;       // [waves][H]   W target, later d(W target)
    float* sD;       // [waves][GR_MAX_L]  d(dot) per position
};

__device__ __forceinline__ ScoreLds sc_lds(const ScoreArgs& p, float* smem) {
    ScoreLds l;
    l.sW = smem;
    l.sT = l.sW + p.H * (p.H | 1);
    l.sV = l.sT + SC_WAVES * GR_MAX_H;
    l.sD = l.sV + SC_WAVES * GR_MAX_H;
    return l;
}

// the target of sample b -> sT, v = W target (or the target itself) -> sV.  Two barriers inside.
__device__ __forceinline__ void sc_target(const ScoreArgs& p, const ScoreLds& l, int64_t b, bool valid) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, H = p.H, HS = H | 1;
    if (lane < H) {
        const int part = lane / p.D;
        l.sT[w * GR_MAX_H + lane] = valid ? p.tgt.tgt[part][fx_parts_tgt_off(p.tgt, part, b, lane - part * p.D)] : 0.f;
    }
    __syncthreads();
    if (lane < H) {
        float v = l.sT[w * GR_MAX_H + lane];
        if (p.W != nullptr) {
            v = 0.f;
            for (int c = 0; c < H; ++c) v = fmaf(l.sW[lane * HS + c], l.sT[w * GR_MAX_H + c], v);
        }
        l.sV[w * GR_MAX_H + lane] = v;
    }
    __syncthreads();
}

__device__ __forceinline__ void sc_stage_w(const ScoreArgs& p, const ScoreLds& l) {
    if (p.W == nullptr) return;
    const int H = p.H, HS = H | 1;
    for (int e = threadIdx.x; e < H * H; e += GR_T) l.sW[(e / H) * HS + e % H] = p.W[e];
}

__global__ __launch_bounds__(GR_T) void k_seq_score_fwd(ScoreArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ScoreLds l = sc_lds(p, smem);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, H = p.H, L = p.L;
    sc_stage_w(p, l);
    __syncthreads();
    const int64_t groups = (p.B + SC_WAVES - 1) / SC_WAVES;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t b = g * SC_WAVES + w;
        const bool valid = b < p.B;
        sc_target(p, l, b, valid);
        if (valid) {
            const float* v = l.sV + w * GR_MAX_H;
            float sc[SC_PER_LANE];
            int mk[SC_PER_LANE];
            float open = 0.f, mx = -__builtin_huge_valf();
#pragma unroll
            for (int i = 0; i < SC_PER_LANE; ++i) {
                const int t = lane + 64 * i;
                sc[i] = 0.f;
                mk[i] = 0;
                if (t < L) {
                    mk[i] = p.ids[b * p.ids_ld + t] != 0 ? 1 : 0;
                    const float4* row = reinterpret_cast<const float4*>(p.I + (b * L + t) * H);
                    float s = 0.f;
                    for (int c = 0; c < H / 4; ++c) {
                        const float4 x = row[c];
                        s = fmaf(x.x, v[4 * c], s);
                        s = fmaf(x.y, v[4 * c + 1], s);
                        s = fmaf(x.z, v[4 * c + 2], s);
                        s = fmaf(x.w, v[4 * c + 3], s);
                    }
                    sc[i] = mk[i] ? s : 0.f;
                    open += (float)mk[i];
                    if (p.softmax) {
                        sc[i] = mk[i] ? s : -1e9f;
                        mx = fmaxf(mx, sc[i]);
                    }
                }
            }
            if (p.softmax) {
                open = fx_wave_sum(open);
                mx = fx_wave_max(mx);
                float sum = 0.f;
#pragma unroll
                for (int i = 0; i < SC_PER_LANE; ++i) {
                    sc[i] = lane + 64 * i < L ? expf(sc[i] - mx) : 0.f;
                    sum += sc[i];
                }
                sum = fx_wave_sum(sum);
#pragma unroll
                for (int i = 0; i < SC_PER_LANE; ++i) sc[i] = open > 0.f ? sc[i] / sum : 0.f;   // len 0: no NaN, 0
            }
#pragma unroll
            for (int i = 0; i < SC_PER_LANE; ++i)
                if (lane + 64 * i < L) p.S[b * L + lane + 64 * i] = sc[i];
        }
    }
}

// R: entries per thread of dW (H H <= 256 R)
template <int R>
__global__ __launch_bounds__(GR_T) void k_seq_score_bwd(ScoreArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ScoreLds l = sc_lds(p, smem);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, H = p.H, HS = H | 1, L = p.L;
    sc_stage_w(p, l);
    __syncthreads();
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    const int64_t groups = (p.B + SC_WAVES - 1) / SC_WAVES;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t b = g * SC_WAVES + w;
        const bool valid = b < p.B;
        sc_target(p, l, b, valid);
        float* sD = l.sD + w * GR_MAX_L;
        if (valid) {
            float pr[SC_PER_LANE], ds[SC_PER_LANE];
            int mk[SC_PER_LANE];
            float delta = 0.f, open = 0.f;
#pragma unroll
            for (int i = 0; i < SC_PER_LANE; ++i) {
                const int t = lane + 64 * i;
                pr[i] = ds[i] = 0.f;
                mk[i] = 0;
                if (t < L) {
                    mk[i] = p.ids[b * p.ids_ld + t] != 0 ? 1 : 0;
                    pr[i] = p.P[b * L + t];
                    ds[i] = p.dS[b * L + t];
                    delta = fmaf(pr[i], ds[i], delta);
                    open += (float)mk[i];
                }
            }
            if (p.softmax) {
                delta = fx_wave_sum(delta);
                open = fx_wave_sum(open);
            }
#pragma unroll
            for (int i = 0; i < SC_PER_LANE; ++i) {
                const int t = lane + 64 * i;
                if (t < L) {
                    float d = ds[i];
                    if (p.softmax) d = open > 0.f ? pr[i] * (ds[i] - delta) : 0.f;
                    sD[t] = mk[i] ? d : 0.f;
                }
            }
        }
        __syncthreads();
        float dv = 0.f;
        if (valid) {
            const float* v = l.sV + w * GR_MAX_H;
            if (p.dI != nullptr)
                for (int e = lane; e < L * (H / 4); e += 64) {       // d interest[t] = d(dot)[t] * v
                    const int t = e / (H / 4), c = e - t * (H / 4);
                    const float d = sD[t];
                    reinterpret_cast<float4*>(p.dI + (b * L + t) * H)[c] =
                        make_float4(d * v[4 * c], d * v[4 * c + 1], d * v[4 * c + 2], d * v[4 * c + 3]);
                }
            if (lane < H)
                for (int t = 0; t < L; ++t) dv = fmaf(sD[t], p.I[(b * L + t) * H + lane], dv);
        }
        __syncthreads();                                             // every lane is done with v
        if (lane < H) l.sV[w * GR_MAX_H + lane] = dv;                // d(W target); 0 for a wave without a sample
        __syncthreads();
        if (valid && lane < H) {
            float dt = l.sV[w * GR_MAX_H + lane];
            if (p.W != nullptr) {
                dt = 0.f;
                for (int c = 0; c < H; ++c) dt = fmaf(l.sW[c * HS + lane], l.sV[w * GR_MAX_H + c], dt);
            }
            const int part = lane / p.D;
            fx_parts_put(p.dtgt.tgt[part], fx_parts_tgt_off(p.dtgt, part, b, lane - part * p.D), dt, false);
        }
        if (p.W != nullptr) {                                        // dW[k][c] += d(W target)[k] * target[c]
            int e = threadIdx.x;
#pragma unroll
            for (int r = 0; r < R; ++r, e += GR_T) {
                if (e < H * H) {
                    const int k = e / H, c = e - k * H;
                    float s = 0.f;
#pragma unroll
                    for (int ww = 0; ww < SC_WAVES; ++ww)
                        s = fmaf(l.sV[ww * GR_MAX_H + k], l.sT[ww * GR_MAX_H + c], s);
                    acc[r] += s;
                }
            }
        }
        __syncthreads();
    }
    if (p.W != nullptr) {
        float* part = p.partial + (int64_t)blockIdx.x * p.n_grad;
        int e = threadIdx.x;
#pragma unroll
        for (int r = 0; r < R; ++r, e += GR_T)
            if (e < H * H) part[e] = acc[r];
    }
}

static int sc_check(const char* who, const float* interest, const fx_seq_parts* tgt, const int32_t* ids,
                    int64_t ids_ld, int64_t B, int32_t L, int32_t H) {
    FX_CHECK_ARG(tgt, "%s: null target description", who);
    FX_CHECK_ARG(H >= 4 && H <= GR_MAX_H && H % 4 == 0, "%s: H=%d, limit 4 <= H <= 64 and H %% 4 == 0", who, H);
    FX_CHECK_ARG(L >= 1 && L <= GR_MAX_L, "%s: L=%d, limit 1 <= L <= 256", who, L);
    FX_CHECK_ARG(tgt->n_parts >= 1 && tgt->n_parts <= 2 && tgt->D >= 1 && tgt->D * tgt->n_parts == H,
                 "%s: H=%d is not n_parts=%d (1 or 2) * D=%d", who, H, tgt->n_parts, tgt->D);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(interest && fx_al16(interest), "%s: interest is null or not 16-byte aligned", who);
    for (int i = 0; i < tgt->n_parts; ++i)
        if (int st = fx_parts_check_tgt(who, "part", tgt, i, tgt->D, false)) return st;
    FX_CHECK_ARG(ids && ids_ld >= L, "%s: null ids or ids stride %lld < L", who, (long long)ids_ld);
    return FX_OK;
}

static ScoreArgs sc_args(const float* interest, const fx_seq_parts* tgt, const int32_t* ids, int64_t ids_ld,
                         int64_t B, int32_t L, int32_t H, const float* W, int32_t softmax) {
    ScoreArgs p;
    memset(&p, 0, sizeof(p));
    p.I = interest; p.tgt = *tgt; p.ids = ids; p.ids_ld = ids_ld; p.B = B;
    p.L = L; p.H = H; p.D = tgt->D; p.softmax = softmax ? 1 : 0; p.W = W;
    return p;
}

static inline size_t sc_lds_bytes(int H) {
    return 4 * ((size_t)H * (H | 1) + 2 * SC_WAVES * GR_MAX_H + SC_WAVES * GR_MAX_L);
}
static inline unsigned sc_grid(int64_t B) {
    const int64_t groups = (B + SC_WAVES - 1) / SC_WAVES;
    return (unsigned)(groups < SC_GRID ? groups : SC_GRID);
}

extern "C" int64_t fx_seq_score_workspace_floats(int64_t B, int32_t H) {
    return (int64_t)sc_grid(B > 0 ? B : 1) * fx_al4((int64_t)H * H);
}

extern "C" int fx_seq_score_fwd(const float* interest, const fx_seq_parts* tgt, const int32_t* ids, int64_t ids_ld,
                                int64_t B, int32_t L, int32_t H, const float* W, int32_t softmax, float* scores,
                                fx_stream_t stream) {
    if (int st = sc_check("fx_seq_score_fwd", interest, tgt, ids, ids_ld, B, L, H)) return st;
    FX_CHECK_ARG(B == 0 || scores, "fx_seq_score_fwd: null scores");
    if (B == 0) return FX_OK;
    ScoreArgs p = sc_args(interest, tgt, ids, ids_ld, B, L, H, W, softmax);
    p.S = scores;
    hipLaunchKernelGGL(k_seq_score_fwd, dim3(sc_grid(B)), dim3(GR_T), sc_lds_bytes(H), fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_seq_score_bwd(const float* interest, const fx_seq_parts* tgt, const int32_t* ids, int64_t ids_ld,
                                int64_t B, int32_t L, int32_t H, const float* W, int32_t softmax, const float* scores,
                                const float* d_scores, float* d_interest, const fx_seq_parts* d_tgt, float* dW,
                                float* workspace, fx_stream_t stream) {
    if (int st = sc_check("fx_seq_score_bwd", interest, tgt, ids, ids_ld, B, L, H)) return st;
    FX_CHECK_ARG(B > 0, "fx_seq_score_bwd: B=%lld", (long long)B);
    FX_CHECK_ARG(scores && d_scores && d_tgt, "fx_seq_score_bwd: null scores / d_scores / gradient description");
    FX_CHECK_ARG(!d_interest || fx_al16(d_interest), "fx_seq_score_bwd: d_interest is not 16-byte aligned");
    FX_CHECK_ARG(!W || (dW && workspace && fx_al16(workspace)), "fx_seq_score_bwd: null dW / workspace, or the "
                 "workspace is not 16-byte aligned");
    for (int i = 0; i < tgt->n_parts; ++i)
        if (int st = fx_parts_check_tgt("fx_seq_score_bwd", "gradient of part", d_tgt, i, tgt->D, true)) return st;
    ScoreArgs p = sc_args(interest, tgt, ids, ids_ld, B, L, H, W, softmax);
    p.dtgt = *d_tgt;
    p.P = scores;
    p.dS = d_scores;
    p.dI = d_interest;
    p.partial = workspace;
    p.n_grad = fx_al4((int64_t)H * H);
    const unsigned grid = sc_grid(B);
    hipStream_t s = fx_hip_stream(stream);
    const size_t lds = sc_lds_bytes(H);
    const int HH = H * H;
    if (HH <= GR_T) hipLaunchKernelGGL(k_seq_score_bwd<1>, dim3(grid), dim3(GR_T), lds, s, p);
    else if (HH <= 4 * GR_T) hipLaunchKernelGGL(k_seq_score_bwd<4>, dim3(grid), dim3(GR_T), lds, s, p);
    else if (HH <= 9 * GR_T) hipLaunchKernelGGL(k_seq_score_bwd<9>, dim3(grid), dim3(GR_T), lds, s, p);
    else hipLaunchKernelGGL(k_seq_score_bwd<16>, dim3(grid), dim3(GR_T), lds, s, p);
    FX_CHECK_LAUNCH();
    if (!W) return FX_OK;
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)grid, fx_al4(HH), fx_rowsum_out(dW, HH));
}
