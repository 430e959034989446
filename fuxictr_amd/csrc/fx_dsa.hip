// fx_dsa.hip — DESTINE's disentangled self-attention over the fields of one sample, one fused layer per launch
// (model_zoo/DESTINE/src/DESTINE.py:143-227):
//     q = X Wq^T + bq, k = X Wk^T + bk, v = X Wv^T + bv [F, A];  u = X Wu^T + bu [F, H];  (q, k, v = relu(.))
//     us = softmax over the fields of u, per column
//     heads by a FLAT view, no transpose: the sample's F H tokens of hd = A / H numbers — token t is field t / H,
//     columns (t % H) hd .. + hd — fall into H groups of F consecutive tokens; per group g
//         Q~ = Q_g - mean_rows(Q_g), K~ = K_g - mean_rows(K_g);  P = softmax_rows(Q~ K~^T [/ sqrt(hd)])
//         O_g[i] = sum_j (P[i][j] + us_token(g F + j)) V_g[j]
//     Y = O through the same token map back to [F, A]  (+ X Wres^T + bres)
// The work split is fx_mhsa.hip's: one workgroup of 256 threads holds one sample at a time, the grid strides over
// the batch, the weights are staged into LDS once per workgroup, only Y goes to HBM.  What is this file's own is the
// REGROUPED image: the projection writes element (field f, column a) of Q, K, V to row i = t % F, column
// g hd + a % hd (t = f H + a / hd, g = t / F), so that a group is a column slice of width hd over F rows — the layout
// the in-LDS core of fx_attn_lds.h works on, which is used unchanged; the token map is applied once on the way in
// (ds_project, the load of dY) and once on the way out (the put of P V; the walks of dX and of the weight gradients
// over the regrouped dQ, dK, dV).  The unary weights need no permutation at all: u [F, H] row-major IS [H][F] in
// token order.  The whitening, the unary soft-max, the ReLU masks (one bit per element, by wave ballot: after the
// whitening Q and K no longer show which of their elements the ReLU cut) and their backward are column walks here.
// The backward recomputes the forward from X with the forward's own functions; nothing else is kept.  Weight and
// bias gradients: entry e of a matrix belongs to thread e % 256 over its workgroup's samples, in registers; one
// partial row per workgroup, summed in a fixed order by fx_rowsum (fx_rowsum.h).  No atomics.
#include "fx_attn_lds.h"
#include "fx_rowsum.h"

#define DS_T FX_ATTN_T
#define DS_MAX FX_ATTN_MAX   // F, D_in, A
#define DS_H_MAX 16          // heads: Wu [H, D_in] next to the four [A, D_in] matrices in the forward's LDS image
#define DS_RU 4              // unary weight-gradient entries per thread (H * D_in <= DS_RU * DS_T)
#define DS_FWD_GRID 2048
#define DS_BWD_GRID 512      // workgroups of the backward = rows of the weight-gradient partials

static_assert(DS_H_MAX * DS_MAX <= DS_RU * DS_T && 4 * DS_MAX <= DS_T && 3 * DS_MAX + DS_H_MAX <= DS_T,
              "fx_dsa: the thread roles of the column phases and of the bias gradients");

struct DsaArgs {
    const float* X;
    int64_t x_ld;
    int64_t B;
    int F, D, A, H, hd, HG, nW;
    const float* W[4];      // Wq, Wk, Wv, Wres (or null), each [A, D]
    const float* Wu;        // [H, D]
    const float* b[4];      // bq, bk, bv, bres (or null), each [A]
    const float* bu;        // [H]
    float scale;            // 1 or 1 / sqrt(head_dim)
    int relu;               // relu_before_att
    float* Y;
    const float* dY;
    float* dX;
    int64_t dx_ld;
    int dx_acc;
    float* partial;         // [grid, n_part]: dWq | dWk | dWv (| dWres) | dWu | dbq | dbk | dbv (| dbres) | dbu
    int n_part;
};

__device__ __forceinline__ FxAttnDims ds_dims(const DsaArgs& p) { return {p.F, p.D, p.A, p.hd, p.HG, p.scale}; }

// the small operands: Wu in LDS next to the big matrices (WLDS) or where it is; the biases always in LDS
struct DsaSmall {
    const float* wu;
    int wu_ld;
    const float* b;         // [4][A]
    const float* bu;        // [H]
};

// floats of the small operands in LDS
__host__ __device__ static inline size_t ds_small_floats(int A, int H) { return 4 * (size_t)A + H; }
static inline size_t ds_wu_floats(int D, int H) { return (size_t)H * fx_attn_odd(D); }
// 32-bit words of one ReLU mask: one bit per element (f, a), a wave's 64 lanes fill two words at a time
static inline size_t ds_mask_words(int F, int A) { return 2 * (((size_t)F * A + 63) / 64); }

template <bool WLDS>
__device__ __forceinline__ DsaSmall ds_stage_small(const DsaArgs& p, float* sWu, float* sB) {
    const int A = p.A, D = p.D, H = p.H, XS = D | 1;
    DsaSmall s;
    if constexpr (WLDS) {
        for (int idx = threadIdx.x; idx < H * D; idx += DS_T) {
            const int c = idx / D, d = idx - c * D;
            sWu[c * XS + d] = p.Wu[idx];
        }
        s.wu = sWu;
        s.wu_ld = XS;
    } else {
        s.wu = p.Wu;
        s.wu_ld = D;
    }
    for (int idx = threadIdx.x; idx < 4 * A; idx += DS_T) {
        const int m = idx / A;
        sB[idx] = p.b[m] != nullptr ? p.b[m][idx - m * A] : 0.f;
    }
    for (int idx = threadIdx.x; idx < H; idx += DS_T) sB[4 * A + idx] = p.bu[idx];
    s.b = sB;
    s.bu = sB + 4 * A;
    return s;
}

// where element (field f, column a) lies in a regrouped [F, A | 1] array
__device__ __forceinline__ int ds_pos(const DsaArgs& p, int f, int a) {
    const int c = a / p.hd, r = a - c * p.hd, t = f * p.H + c, g = t / p.F, i = t - g * p.F;
    return i * (p.A | 1) + g * p.hd + r;
}

// X of sample b -> sX; then q, k, v with their biases (and the ReLU), regrouped, and u [F, H] as it lies.
// MASKS: which elements the ReLU let through, bit f A + a of sM[0 | 1 | 2] (q | k | v).
template <bool WLDS, bool MASKS>
__device__ __forceinline__ void ds_project(const DsaArgs& p, const FxAttnW<4, WLDS>& w, const DsaSmall& sm, int64_t b,
                                           float* sX, float* sQ, float* sK, float* sV, float* sU, unsigned* sM,
                                           int MW) {
    const int F = p.F, D = p.D, A = p.A, H = p.H, XS = D | 1;
    const float* x = p.X + b * p.x_ld;
    for (int idx = threadIdx.x; idx < F * D; idx += DS_T) {
        const int f = idx / D, d = idx - f * D;
        sX[f * XS + d] = x[idx];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < F * A; idx += DS_T) {
        const int f = idx / A, a = idx - f * A;
        float q = 0.f, k = 0.f, v = 0.f;
        for (int d = 0; d < D; ++d) {
            const float xv = sX[f * XS + d];
            q = fmaf(xv, w(0, a, d), q);
            k = fmaf(xv, w(1, a, d), k);
            v = fmaf(xv, w(2, a, d), v);
        }
        q += sm.b[a];
        k += sm.b[A + a];
        v += sm.b[2 * A + a];
        if (p.relu) {
            if constexpr (MASKS) {
                // the wave's 64 consecutive elements start at a multiple of 64: its first lane is always live
                const unsigned long long mq = __ballot(q > 0.f), mk = __ballot(k > 0.f), mv = __ballot(v > 0.f);
                if ((threadIdx.x & 63) == 0) {
                    const int wd = idx >> 5;
                    sM[wd] = (unsigned)mq;           sM[wd + 1] = (unsigned)(mq >> 32);
                    sM[MW + wd] = (unsigned)mk;      sM[MW + wd + 1] = (unsigned)(mk >> 32);
                    sM[2 * MW + wd] = (unsigned)mv;  sM[2 * MW + wd + 1] = (unsigned)(mv >> 32);
                }
            }
            q = fmaxf(q, 0.f);
            k = fmaxf(k, 0.f);
            v = fmaxf(v, 0.f);
        }
        const int pp = ds_pos(p, f, a);
        sQ[pp] = q;
        sK[pp] = k;
        sV[pp] = v;
    }
    for (int idx = threadIdx.x; idx < F * H; idx += DS_T) {
        const int f = idx / H, c = idx - f * H;
        float u = 0.f;
        for (int d = 0; d < D; ++d) u = fmaf(sX[f * XS + d], sm.wu[c * sm.wu_ld + d], u);
        sU[idx] = u + sm.bu[c];
    }
}

// column `col` of a regrouped array minus its mean over the F rows (a group's tokens), in place
__device__ __forceinline__ void ds_center_col(float* s, int col, int F, int AS) {
    float sum = 0.f;
    for (int i = 0; i < F; ++i) sum += s[i * AS + col];
    const float mean = sum / (float)F;
    for (int i = 0; i < F; ++i) s[i * AS + col] -= mean;
}

// The column phase after the projection: threads 0 .. 2A-1 whiten a column of Q or K, the next H soft-max a column
// of u over the fields (stable: the maximum subtracted), in place.
__device__ __forceinline__ void ds_whiten_and_unary(const DsaArgs& p, float* sQ, float* sK, float* sU) {
    const int F = p.F, A = p.A, H = p.H, AS = A | 1, tid = threadIdx.x;
    if (tid < 2 * A) {
        ds_center_col(tid < A ? sQ : sK, tid < A ? tid : tid - A, F, AS);
    } else if (tid < 2 * A + H) {
        float* u = sU + (tid - 2 * A);
        float m = u[0];
        for (int f = 1; f < F; ++f) m = fmaxf(m, u[f * H]);
        float sum = 0.f;
        for (int f = 0; f < F; ++f) {
            const float e = expf(u[f * H] - m);
            u[f * H] = e;
            sum += e;
        }
        for (int f = 0; f < F; ++f) u[f * H] = u[f * H] / sum;
    }
}

// fx_mhsa.hip's serial soft-max of one score row (a copy: that one is private to its file)
__device__ __forceinline__ void ds_softmax_row(float* row, int F) {
    float m = row[0];
    for (int j = 1; j < F; ++j) m = fmaxf(m, row[j]);
    float sum = 0.f;
    for (int j = 0; j < F; ++j) {
        const float e = expf(row[j] - m);
        row[j] = e;
        sum += e;
    }
    for (int j = 0; j < F; ++j) row[j] = row[j] / sum;
}

// (the weights always fit into LDS next to the forward's image: at most 159 104 bytes, at F = D = A = 64, H = 16 with
// a W_res — so the forward has no instantiation that reads them from HBM)
__global__ __launch_bounds__(DS_T) void k_dsa_fwd(DsaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FxAttnDims g = ds_dims(p);
    const int F = p.F, D = p.D, A = p.A, H = p.H, hd = p.hd, XS = D | 1, AS = A | 1, FS = F | 1;
    float* sX = smem;
    float* sQ = sX + F * XS;
    float* sK = sQ + F * AS;
    float* sV = sK + F * AS;
    float* sS = sV + F * AS;
    float* sU = sS + p.HG * F * FS;      // the unary weights, [F, H] = [H][F] in token order
    float* sB = sU + F * H;
    float* sW = sB + ds_small_floats(A, H);
    float* sWu = sW + p.nW * A * XS;
    const FxAttnW<4, true> w = fx_attn_weights<4, true>(p.W, p.nW, A, D, sW);
    const DsaSmall sm = ds_stage_small<true>(p, sWu, sB);
    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        __syncthreads();
        ds_project<true, false>(p, w, sm, b, sX, sQ, sK, sV, sU, nullptr, 0);
        __syncthreads();
        ds_whiten_and_unary(p, sQ, sK, sU);
        for (int h0 = 0; h0 < H; h0 += p.HG) {
            const int hg = H - h0 < p.HG ? H - h0 : p.HG;
            __syncthreads();
            fx_attn_scores(g, h0, hg, sQ, sK, sS);
            __syncthreads();
            // the pairwise soft-max of a row, then the group's unary weights onto every row
            for (int idx = threadIdx.x; idx < hg * F; idx += DS_T) {
                float* row = sS + idx * FS;
                const float* un = sU + (h0 + idx / F) * F;
                ds_softmax_row(row, F);
                for (int j = 0; j < F; ++j) row[j] += un[j];
            }
            __syncthreads();
            // the way out: token (group, row i) back to its field and column chunk; the biased residual out of sX
            fx_attn_pv(g, h0, hg, sS, sV, [&](int i, int a, float o) {
                const int gg = a / hd, r = a - gg * hd, t = gg * F + i, f = t / H, col = (t - f * H) * hd + r;
                if (p.W[3] != nullptr) {
                    float r2 = 0.f;
                    for (int d = 0; d < D; ++d) r2 = fmaf(sX[f * XS + d], w(3, col, d), r2);
                    o += r2 + sm.b[3 * A + col];
                }
                p.Y[(b * F + f) * A + col] = o;
            });
        }
    }
}

// R: weight-gradient entries per thread and [A, D] matrix (A * D <= 256 R)
template <bool WLDS, int R>
__global__ __launch_bounds__(DS_T) void k_dsa_bwd(DsaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FxAttnDims g = ds_dims(p);
    const int F = p.F, D = p.D, A = p.A, H = p.H, hd = p.hd, XS = D | 1, AS = A | 1, FS = F | 1;
    const int MW = (int)(2 * ((F * A + 63) / 64)), tid = threadIdx.x;
    float* sX = smem;
    float* sQ = sX + F * XS;
    float* sK = sQ + F * AS;
    float* sV = sK + F * AS;          // V, then dV (head by head)
    float* sG = sV + F * AS;          // dY, regrouped
    float* sdQ = sG + F * AS;
    float* sdK = sdQ + F * AS;
    float* sP = sdK + F * AS;
    float* sD = sP + p.HG * F * FS;   // dP, then dS
    float* sU = sD + p.HG * F * FS;   // us
    float* sdU = sU + F * H;          // d us, then du
    float* sGs = sdU + F * H;         // the column sums of G: a group's sum_i G_i
    unsigned* sM = reinterpret_cast<unsigned*>(sGs + A);
    float* sB = reinterpret_cast<float*>(sM + 3 * MW);
    float* sW = sB + ds_small_floats(A, H);
    float* sWu = sW + p.nW * A * XS;
    const FxAttnW<4, WLDS> w = fx_attn_weights<4, WLDS>(p.W, p.nW, A, D, sW);
    const DsaSmall sm = ds_stage_small<WLDS>(p, sWu, sB);
    const bool wres = p.W[3] != nullptr;
    float acc[4][R], accu[DS_RU], accb = 0.f, accbu = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
#pragma unroll
    for (int r = 0; r < DS_RU; ++r) accu[r] = 0.f;

    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        __syncthreads();
        for (int idx = tid; idx < F * A; idx += DS_T) {
            const int f = idx / A, a = idx - f * A;
            sG[ds_pos(p, f, a)] = p.dY[b * F * A + idx];
        }
        ds_project<WLDS, true>(p, w, sm, b, sX, sQ, sK, sV, sU, sM, MW);
        __syncthreads();
        ds_whiten_and_unary(p, sQ, sK, sU);
        if (tid >= DS_T - A) {              // (the threads the column phase leaves idle)
            const int col = DS_T - 1 - tid;
            float s = 0.f;
            for (int i = 0; i < F; ++i) s += sG[i * AS + col];
            sGs[col] = s;
        }
        __syncthreads();
        // d us of token j of group gg = V_j . sum_i G_i, before dV takes V's place
        for (int t = tid; t < F * H; t += DS_T) {
            const int gg = t / F, j = t - gg * F;
            const float* v = sV + j * AS + gg * hd;
            const float* gs = sGs + gg * hd;
            float s = 0.f;
            for (int c = 0; c < hd; ++c) s = fmaf(v[c], gs[c], s);
            sdU[t] = s;
        }
        for (int h0 = 0; h0 < H; h0 += p.HG) {
            const int hg = H - h0 < p.HG ? H - h0 : p.HG;
            __syncthreads();
            fx_attn_scores(g, h0, hg, sQ, sK, sP);
            fx_attn_dp(g, h0, hg, sG, sV, sD);
            __syncthreads();
            // row by row: P = softmax(S), then dS = P (dP - sum_j P dP) * scale — the pairwise P alone
            for (int idx = tid; idx < hg * F; idx += DS_T) {
                float* pr = sP + idx * FS;
                float* dr = sD + idx * FS;
                ds_softmax_row(pr, F);
                float delta = 0.f;
                for (int j = 0; j < F; ++j) delta = fmaf(pr[j], dr[j], delta);
                for (int j = 0; j < F; ++j) dr[j] = pr[j] * (dr[j] - delta) * p.scale;
            }
            __syncthreads();
            fx_attn_dqkv(g, h0, hg, sP, sD, sG, sQ, sK, sV, sdQ, sdK);
        }
        __syncthreads();
        // the column phase of the backward: dQ, dK through the whitening; d us through the unary soft-max;
        // dV_j += us_j sum_i G_i
        if (tid < 2 * A) {
            ds_center_col(tid < A ? sdQ : sdK, tid < A ? tid : tid - A, F, AS);
        } else if (tid < 2 * A + H) {
            // in fp64: du sums to zero over the fields in exact arithmetic (the soft-max ignores bu), so dbu is
            // all rounding residue, and the fp32 roundings of the dot product and the differences would be most of it
            const int c = tid - 2 * A;
            double dot = 0.0, sum = 0.0;
            for (int f = 0; f < F; ++f) dot += (double)sU[f * H + c] * (double)sdU[f * H + c];
            for (int f = 0; f < F; ++f) {
                const double du = (double)sU[f * H + c] * ((double)sdU[f * H + c] - dot);
                sdU[f * H + c] = (float)du;
                sum += du;
            }
            accbu += (float)sum;
        } else if (tid >= DS_T - A) {
            const int col = DS_T - 1 - tid;
            const float* un = sU + (col / hd) * F;
            const float gs = sGs[col];
            for (int i = 0; i < F; ++i) sV[i * AS + col] = fmaf(un[i], gs, sV[i * AS + col]);
        }
        __syncthreads();
        if (p.relu) {
            for (int idx = tid; idx < F * A; idx += DS_T) {
                const int f = idx / A, a = idx - f * A, pp = ds_pos(p, f, a), wd = idx >> 5;
                const unsigned bit = 1u << (idx & 31);
                if (!(sM[wd] & bit)) sdQ[pp] = 0.f;
                if (!(sM[MW + wd] & bit)) sdK[pp] = 0.f;
                if (!(sM[2 * MW + wd] & bit)) sV[pp] = 0.f;
            }
            __syncthreads();
        }
        // dX[f] = dq_f Wq + dk_f Wk + dv_f Wv (+ dY_f Wres) + du_f Wu: field f's H tokens lie one row apart
        for (int idx = tid; idx < F * D; idx += DS_T) {
            const int f = idx / D, d = idx - f * D;
            int gg = (f * H) / F, i = f * H - gg * F;
            float s = 0.f;
            for (int c = 0; c < H; ++c) {
                const int pp = i * AS + gg * hd;
                for (int r = 0; r < hd; ++r) {
                    const int a = c * hd + r;
                    s = fmaf(sdQ[pp + r], w(0, a, d), s);
                    s = fmaf(sdK[pp + r], w(1, a, d), s);
                    s = fmaf(sV[pp + r], w(2, a, d), s);
                    if (wres) s = fmaf(sG[pp + r], w(3, a, d), s);
                }
                s = fmaf(sdU[f * H + c], sm.wu[c * sm.wu_ld + d], s);
                if (++i == F) { i = 0; ++gg; }
            }
            float* dx = p.dX + b * p.dx_ld + (f * D + d);
            *dx = p.dx_acc ? *dx + s : s;
        }
        // dW*[a][d] += sum_f d*[f][a] X[f][d]: column a of field f is hd-chunk c = a / hd of token f H + c.  The fourth
        // sum (dY^T X, for W_res) runs without a W_res too and is then never stored: a test of `wres` inside the loop
        // timed the R = 4 backward 6 % slower with a W_res (1086 us against 1022 us at B 4096, F 24, D = A 40), and two
        // copies of the walk chosen outside it through a generic lambda 73 % slower (1768 us: the accumulators left
        // the registers); each_layer, the reference's default, always has a W_res
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = tid + r * DS_T;
            if (e < A * D) {
                const int a = e / D, d = e - a * D, c = a / hd;
                int gg = c / F, i = c - gg * F;
                const int off = a - c * hd;
                float tq = 0.f, tk = 0.f, tv = 0.f, tr = 0.f;
                for (int f = 0; f < F; ++f) {
                    const float xv = sX[f * XS + d];
                    const int pp = i * AS + gg * hd + off;
                    tq = fmaf(sdQ[pp], xv, tq);
                    tk = fmaf(sdK[pp], xv, tk);
                    tv = fmaf(sV[pp], xv, tv);
                    tr = fmaf(sG[pp], xv, tr);
                    i += H;
                    while (i >= F) { i -= F; ++gg; }
                }
                acc[0][r] += tq;
                acc[1][r] += tk;
                acc[2][r] += tv;
                acc[3][r] += tr;
            }
        }
        // the bias gradients: thread m A + a sums column a of matrix m's gradient over the fields
        if (tid < p.nW * A) {
            const int m = tid / A, a = tid - m * A, c = a / hd;
            const float* dz = m == 0 ? sdQ : m == 1 ? sdK : m == 2 ? sV : sG;
            int gg = c / F, i = c - gg * F;
            const int off = a - c * hd;
            float t = 0.f;
            for (int f = 0; f < F; ++f) {
                t += dz[i * AS + gg * hd + off];
                i += H;
                while (i >= F) { i -= F; ++gg; }
            }
            accb += t;
        }
        // dWu[c][d] += sum_f du[f][c] X[f][d] (dbu: thread 2A + c of the column phase above)
#pragma unroll
        for (int r = 0; r < DS_RU; ++r) {
            const int e = tid + r * DS_T;
            if (e < H * D) {
                const int c = e / D, d = e - c * D;
                float t = 0.f;
                for (int f = 0; f < F; ++f) t = fmaf(sdU[f * H + c], sX[f * XS + d], t);
                accu[r] += t;
            }
        }
    }
    float* part = p.partial + (int64_t)blockIdx.x * p.n_part;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = tid + r * DS_T;
        if (e < A * D) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < p.nW) part[m * A * D + e] = acc[m][r];
        }
    }
    part += p.nW * A * D;
#pragma unroll
    for (int r = 0; r < DS_RU; ++r) {
        const int e = tid + r * DS_T;
        if (e < H * D) part[e] = accu[r];
    }
    part += H * D;
    if (tid < p.nW * A) part[tid] = accb;
    if (tid >= 2 * A && tid < 2 * A + H) part[p.nW * A + tid - 2 * A] = accbu;
}

static int ds_check(const char* who, const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D,
                    const float* const* W, const float* const* bias, int32_t A, int32_t H) {
    FX_CHECK_ARG(F >= 1 && F <= DS_MAX, "%s: F=%d, limit 1 <= F <= %d", who, F, DS_MAX);
    FX_CHECK_ARG(D >= 1 && D <= DS_MAX, "%s: D_in=%d, limit 1 <= D_in <= %d", who, D, DS_MAX);
    FX_CHECK_ARG(A >= 1 && A <= DS_MAX, "%s: A=%d, limit 1 <= A <= %d", who, A, DS_MAX);
    FX_CHECK_ARG(H >= 1 && H <= DS_H_MAX, "%s: H=%d, limit 1 <= H <= %d", who, H, DS_H_MAX);
    FX_CHECK_ARG(A % H == 0, "%s: H=%d does not divide A=%d", who, H, A);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(W && bias, "%s: null W / bias pointer tables", who);
    FX_CHECK_ARG(B == 0 || X, "%s: null X", who);
    for (int m = 0; m < 5; ++m) {
        if (m == 3) continue;
        FX_CHECK_ARG(B == 0 || (W[m] && bias[m]), "%s: null weight or bias %d (Wq, Wk, Wv, Wres, Wunary)", who, m);
    }
    FX_CHECK_ARG((W[3] == nullptr) == (bias[3] == nullptr), "%s: Wres and its bias come together", who);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: sample stride %lld < F*D_in", who, (long long)x_ld);
    return FX_OK;
}

static DsaArgs ds_args(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* const* W,
                       const float* const* bias, int32_t A, int32_t H, int32_t use_scale, int32_t relu) {
    DsaArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B;
    p.F = F; p.D = D; p.A = A; p.H = H; p.hd = A / H;
    p.HG = fx_attn_heads_per_pass(F, H);
    for (int m = 0; m < 4; ++m) { p.W[m] = W[m]; p.b[m] = bias[m]; }
    p.Wu = W[4]; p.bu = bias[4];
    p.nW = p.W[3] ? 4 : 3;
    p.n_part = (p.nW * A + H) * (D + 1);
    p.scale = use_scale ? (float)(1.0 / sqrt((double)p.hd)) : 1.f;
    p.relu = relu ? 1 : 0;
    return p;
}

// LDS: X, n_rows [F, A] arrays, n_score score buffers and `extra` floats; the four matrices and Wu join them when
// all of it fits (Wu counts as rows of a fifth matrix: ds_wu_floats over A (D | 1), rounded up, is never the edge —
// the sum is recomputed exactly here)
static inline FxAttnLds ds_lds(const DsaArgs& p, int n_rows, int n_score, size_t extra) {
    const size_t n = fx_attn_lds_floats(p.F, p.D, p.A, n_rows, n_score, fx_attn_score_floats(p.F, p.HG),
                                        extra + ds_small_floats(p.A, p.H));
    const size_t with_w = 4 * (n + (size_t)p.nW * p.A * fx_attn_odd(p.D) + ds_wu_floats(p.D, p.H));
    FxAttnLds l;
    l.wlds = with_w <= FX_ATTN_LDS_MAX;
    l.bytes = l.wlds ? with_w : 4 * n;
    return l;
}

extern "C" void fx_dsa_limits(int32_t* limits) {
    limits[0] = DS_MAX;         // F
    limits[1] = DS_MAX;         // D_in
    limits[2] = DS_MAX;         // A
    limits[3] = DS_H_MAX;       // H
    limits[4] = DS_FWD_GRID;
    limits[5] = DS_BWD_GRID;
}

extern "C" int64_t fx_dsa_workspace_floats(int64_t B, int32_t D_in, int32_t A, int32_t H, int32_t has_wres) {
    const int64_t G = B < DS_BWD_GRID ? (B > 0 ? B : 1) : DS_BWD_GRID;
    return G * ((has_wres ? 4 : 3) * (int64_t)A + H) * (D_in + 1);
}

extern "C" int fx_dsa_fwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D_in, const float* const* W,
                          const float* const* bias, int32_t A, int32_t H, int32_t use_scale, int32_t relu_before_att,
                          float* Y, fx_stream_t stream) {
    if (int st = ds_check("fx_dsa_fwd", X, x_ld, B, F, D_in, W, bias, A, H)) return st;
    FX_CHECK_ARG(B == 0 || Y, "fx_dsa_fwd: null Y");
    if (B == 0) return FX_OK;
    DsaArgs p = ds_args(X, x_ld, B, F, D_in, W, bias, A, H, use_scale, relu_before_att);
    p.Y = Y;
    // Q, K, V, one score buffer, us and the weights: see k_dsa_fwd (the check only guards a later change of the limits)
    const FxAttnLds l = ds_lds(p, 3, 1, (size_t)F * H);
    FX_CHECK_ARG(l.wlds, "fx_dsa_fwd: %zu bytes of LDS without the weights", l.bytes);
    const unsigned grid = (unsigned)(B < DS_FWD_GRID ? B : DS_FWD_GRID);
    return fx_attn_launch<k_dsa_fwd>(p, grid, l.bytes, fx_hip_stream(stream));
}

template <bool WLDS>
static int ds_launch_bwd(const DsaArgs& p, unsigned grid, size_t lds, hipStream_t s) {
    const int AD = p.A * p.D;
    if (AD <= DS_T) return fx_attn_launch<k_dsa_bwd<WLDS, 1>>(p, grid, lds, s);
    if (AD <= 4 * DS_T) return fx_attn_launch<k_dsa_bwd<WLDS, 4>>(p, grid, lds, s);
    return fx_attn_launch<k_dsa_bwd<WLDS, 16>>(p, grid, lds, s);
}

extern "C" int fx_dsa_bwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D_in, const float* const* W,
                          const float* const* bias, int32_t A, int32_t H, int32_t use_scale, int32_t relu_before_att,
                          const float* dY, float* dX, int64_t dx_ld, int32_t dx_accumulate, float* dW,
                          float* workspace, fx_stream_t stream) {
    if (int st = ds_check("fx_dsa_bwd", X, x_ld, B, F, D_in, W, bias, A, H)) return st;
    FX_CHECK_ARG(B > 0, "fx_dsa_bwd: B=%lld", (long long)B);
    FX_CHECK_ARG(dY && dX && dW && workspace, "fx_dsa_bwd: null dY / dX / dW / workspace");
    FX_CHECK_ARG(dx_ld >= (int64_t)F * D_in, "fx_dsa_bwd: dX sample stride %lld < F*D_in", (long long)dx_ld);
    DsaArgs p = ds_args(X, x_ld, B, F, D_in, W, bias, A, H, use_scale, relu_before_att);
    p.dY = dY;
    p.dX = dX;
    p.dx_ld = dx_ld;
    p.dx_acc = dx_accumulate ? 1 : 0;
    p.partial = workspace;
    // six [F, A] arrays, two score buffers (P, dP | dS), us, d us, the column sums of dY and the three ReLU masks;
    // the weights join them in LDS when all of it fits
    const FxAttnLds l = ds_lds(p, 6, 2, 2 * (size_t)F * H + A + 3 * ds_mask_words(F, A));
    FX_CHECK_ARG(l.bytes <= FX_ATTN_LDS_MAX, "fx_dsa_bwd: %zu bytes of LDS without the weights", l.bytes);
    const unsigned grid = (unsigned)(B < DS_BWD_GRID ? B : DS_BWD_GRID);
    hipStream_t s = fx_hip_stream(stream);
    const int st = l.wlds ? ds_launch_bwd<true>(p, grid, l.bytes, s) : ds_launch_bwd<false>(p, grid, l.bytes, s);
    if (st) return st;
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)grid, p.n_part, fx_rowsum_out(dW, p.n_part));
}
