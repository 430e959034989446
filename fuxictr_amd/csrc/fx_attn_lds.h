// fx_attn_lds.h — the in-LDS multi-head attention core of fx_mhsa.hip (AutoInt) and fx_bst.hip (BST), written once.
// One workgroup of FX_ATTN_T threads holds one sample: X [n, d], Q, K, V [n, a] and the scores [hg, n, n] of a
// group of heads, every row with an odd stride (x | 1), so that the row-wise and the column-wise walks of a phase
// are both free of bank conflicts.  fp32 FMAs out of LDS in a fixed order: the backward calls the forward's own
// functions and gets the forward's bits.  None of the functions synchronises: the callers place the barriers.
// What is NOT here: loading X and the Q / K / V projection (each file keeps its own: as a shared helper it cost the
// R = 16 backward kernels 4 to 5 %) and, because the two kernels differ in them, the soft-max (a thread per row with
// serial sums in fx_mhsa.hip, a wave per row with butterfly sums in fx_bst.hip: two summation orders, two sets of
// bits) and everything after O = P V.
#pragma once
#include "fx_common.h"

#define FX_ATTN_T 256                 // threads per workgroup
#define FX_ATTN_MAX 64                // n, d, a
#define FX_ATTN_SBUF (64 * 65)        // floats of one score buffer: the heads of a group share it
#define FX_ATTN_LDS_MAX (160 * 1024)
#define FX_ATTN_NEG_INF (-__builtin_huge_valf())

struct FxAttnDims {
    int n, d, a;      // rows (fields, positions), width of X, width of Q / K / V
    int hd, HG;       // head width, heads per pass
    float scale;
};

// ---- host: what a launch needs ----------------------------------------------------------------------------
static inline int fx_attn_odd(int n) { return n | 1; }
static inline int fx_attn_heads_per_pass(int n, int H) {
    const int hg = FX_ATTN_SBUF / (n * fx_attn_odd(n));
    return hg < H ? hg : H;
}
static inline size_t fx_attn_score_floats(int n, int HG) { return (size_t)HG * n * fx_attn_odd(n); }
// floats of LDS: X + n_rows [n, a] arrays + n_score score buffers of score_floats + extra, without the weights
static inline size_t fx_attn_lds_floats(int n, int d, int a, int n_rows, int n_score, size_t score_floats,
                                        size_t extra) {
    return (size_t)n * fx_attn_odd(d) + (size_t)n_rows * n * fx_attn_odd(a) + n_score * score_floats + extra;
}
// the nW [a, d] weight matrices join the rest in LDS when all of it fits
struct FxAttnLds {
    bool wlds;
    size_t bytes;
};
static inline FxAttnLds fx_attn_lds(size_t floats, int nW, int a, int d) {
    const size_t with_w = 4 * (floats + (size_t)nW * a * fx_attn_odd(d));
    FxAttnLds l;
    l.wlds = with_w <= FX_ATTN_LDS_MAX;
    l.bytes = l.wlds ? with_w : 4 * floats;
    return l;
}

// One launch of Kernel(p).  (once per kernel and process: it may use the whole 160 KiB)
template <auto Kernel, typename Args>
static int fx_attn_launch(const Args& p, unsigned grid, size_t lds, hipStream_t s) {
    static const hipError_t lds_ok = fx_allow_lds(Kernel, FX_ATTN_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(FX_ATTN_T), lds, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ---- device ---------------------------------------------------------------------------------------------
// NW matrices of [rows, cols], in LDS (WLDS) or where they are: element (a, d) of matrix m
template <int NW, bool WLDS>
struct FxAttnW {
    const float* w[NW];
    int ld;
    __device__ __forceinline__ float operator()(int m, int a, int d) const { return w[m][a * ld + d]; }
};

// stages the first n_stage matrices (WLDS); the caller synchronises before the first use
template <int NW, bool WLDS>
__device__ __forceinline__ FxAttnW<NW, WLDS> fx_attn_weights(const float* const (&W)[NW], int n_stage, int rows,
                                                             int cols, float* sW) {
    FxAttnW<NW, WLDS> w;
    if constexpr (WLDS) {
        const int WS = cols | 1, RC = rows * cols;
        for (int idx = threadIdx.x; idx < n_stage * RC; idx += FX_ATTN_T) {
            const int m = idx / RC, r = idx - m * RC, a = r / cols, d = r - a * cols;
            sW[(m * rows + a) * WS + d] = W[m][r];
        }
        for (int m = 0; m < NW; ++m) w.w[m] = sW + m * rows * WS;
        w.ld = WS;
    } else {
        for (int m = 0; m < NW; ++m) w.w[m] = W[m];
        w.ld = cols;
    }
    return w;
}

// scores of the heads h0 .. h0+hg-1: sS[hh][i][j] = scale * Q_i . K_j (BST's masked ones are its own: fx_bst.hip)
__device__ __forceinline__ void fx_attn_scores(const FxAttnDims& g, int h0, int hg, const float* sQ, const float* sK,
                                               float* sS) {
    const int n = g.n, AS = g.a | 1, NS = n | 1, hd = g.hd, NN = n * n;
    for (int idx = threadIdx.x; idx < hg * NN; idx += FX_ATTN_T) {
        const int hh = idx / NN, r = idx - hh * NN, i = r / n, j = r - i * n;
        const float* q = sQ + i * AS + (h0 + hh) * hd;
        const float* k = sK + j * AS + (h0 + hh) * hd;
        float s = 0.f;
        for (int c = 0; c < hd; ++c) s = fmaf(q[c], k[c], s);
        sS[(hh * n + i) * NS + j] = s * g.scale;
    }
}

// O = P V of the group: put(i, a, O[i][a]) for this group's columns a of every row i
template <typename Put>
__device__ __forceinline__ void fx_attn_pv(const FxAttnDims& g, int h0, int hg, const float* sP, const float* sV,
                                           Put put) {
    const int n = g.n, AS = g.a | 1, NS = n | 1, hd = g.hd;
    const int GW = hg * hd, a0 = h0 * hd;
    for (int idx = threadIdx.x; idx < n * GW; idx += FX_ATTN_T) {
        const int i = idx / GW, r = idx - i * GW, hh = r / hd, a = a0 + r;
        const float* prow = sP + (hh * n + i) * NS;
        float o = 0.f;
        for (int j = 0; j < n; ++j) o = fmaf(prow[j], sV[j * AS + a], o);
        put(i, a, o);
    }
}

// dP[i][j] = dO_i . V_j of the group
__device__ __forceinline__ void fx_attn_dp(const FxAttnDims& g, int h0, int hg, const float* sdO, const float* sV,
                                           float* sD) {
    const int n = g.n, AS = g.a | 1, NS = n | 1, hd = g.hd, NN = n * n;
    for (int idx = threadIdx.x; idx < hg * NN; idx += FX_ATTN_T) {
        const int hh = idx / NN, r = idx - hh * NN, i = r / n, j = r - i * n;
        const float* go = sdO + i * AS + (h0 + hh) * hd;
        const float* v = sV + j * AS + (h0 + hh) * hd;
        float s = 0.f;
        for (int c = 0; c < hd; ++c) s = fmaf(go[c], v[c], s);
        sD[(hh * n + i) * NS + j] = s;
    }
}

// The group's columns, from P and dS:  dV[j][a] = sum_i P[i][j] dO[i][a], over V in place (dP is done with it);
// dQ[i][a] = sum_j dS[i][j] K[j][a];  dK[i][a] = sum_j dS[j][i] Q[j][a]
__device__ __forceinline__ void fx_attn_dqkv(const FxAttnDims& g, int h0, int hg, const float* sP, const float* sdS,
                                             const float* sdO, const float* sQ, const float* sK, float* sV,
                                             float* sdQ, float* sdK) {
    const int n = g.n, AS = g.a | 1, NS = n | 1, hd = g.hd;
    const int GW = hg * hd, a0 = h0 * hd;
    for (int idx = threadIdx.x; idx < n * GW; idx += FX_ATTN_T) {
        const int j = idx / GW, r = idx - j * GW, hh = r / hd, a = a0 + r;
        const float* pc = sP + hh * n * NS + j;
        float s = 0.f;
        for (int i = 0; i < n; ++i) s = fmaf(pc[i * NS], sdO[i * AS + a], s);
        sV[j * AS + a] = s;
    }
    for (int idx = threadIdx.x; idx < n * GW; idx += FX_ATTN_T) {
        const int i = idx / GW, r = idx - i * GW, hh = r / hd, a = a0 + r;
        const float* ds = sdS + hh * n * NS;
        float dq = 0.f, dk = 0.f;
        for (int j = 0; j < n; ++j) {
            dq = fmaf(ds[i * NS + j], sK[j * AS + a], dq);
            dk = fmaf(ds[j * NS + i], sQ[j * AS + a], dk);
        }
        sdQ[i * AS + a] = dq;
        sdK[i * AS + a] = dk;
    }
}

// dX = dQ W_0 + dK W_1 + dV W_2: put(f, d, dX[f][d])
template <typename W, typename Put>
__device__ __forceinline__ void fx_attn_dx(const FxAttnDims& g, const W& w, const float* sdQ, const float* sdK,
                                           const float* sdV, Put put) {
    const int n = g.n, D = g.d, A = g.a, AS = A | 1;
    for (int idx = threadIdx.x; idx < n * D; idx += FX_ATTN_T) {
        const int f = idx / D, d = idx - f * D;
        float s = 0.f;
        for (int a = 0; a < A; ++a) {
            s = fmaf(sdQ[f * AS + a], w(0, a, d), s);
            s = fmaf(sdK[f * AS + a], w(1, a, d), s);
            s = fmaf(sdV[f * AS + a], w(2, a, d), s);
        }
        put(f, d, s);
    }
}

// acc[a][d] += sum_f dz[f][a] in[f][d] for dz [n, A], in [n, D]: this sample's sum first, then onto the running
// one.  Entry e = a * D + d belongs to thread e % FX_ATTN_T, R entries per thread (A * D <= R * FX_ATTN_T).
template <int R>
__device__ __forceinline__ void fx_attn_acc_dw(float (&acc)[R], const float* dz, const float* in, int n, int A,
                                               int D) {
    const int AS = A | 1, XS = D | 1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = threadIdx.x + r * FX_ATTN_T;
        if (e < A * D) {
            const int a = e / D, d = e - a * D;
            float t = 0.f;
            for (int f = 0; f < n; ++f) t = fmaf(dz[f * AS + a], in[f * XS + d], t);
            acc[r] += t;
        }
    }
}
