// fx_bst.hip — one transformer block of the Behavior Sequence Transformer over the positions of one sample, fused:
// masked multi-head attention, output projection, residual, LayerNorm, FFN, residual, LayerNorm and the pooling over
// positions (model_zoo/BST/src/BST.py:183-229, 317-366; torch.nn.MultiheadAttention's packed in_proj):
//     X    = [part 0 | part 1 | .. | position_emb]  per position, positions 0..L-1 of the history, then the target
//     QKV  = X in_w^T + in_b;   per head: P = softmax_rows(Q_h K_h^T / sqrt(hd), -inf where masked);  O_h = P V_h
//     s    = concat_h(O_h) out_w^T + out_b (+ X);  s = LN1(s)
//     out  = W2 lrelu(W1 s + b1) + b2 (+ s);       out = LN2(out);   pooled over the positions or written whole
//     masked(i, j) = (pad[j] and i != j) or (causal and j > i),  pad[j] = (ids[j] == 0) for j < L, pad[L] = false
// One workgroup of 256 threads works on one sample at a time in a grid-stride loop; X, Q, K, V, the scores of a group
// of heads and every intermediate live in LDS with odd row strides; fp32 FMAs; no atomics, so two launches give the
// same bits.  The attention (weight staging, P V, its backward loops, the per-thread weight-gradient sums) is
// the in-LDS core of fx_attn_lds.h, shared with fx_mhsa.hip; this file owns the assembly of X, the projection, the
// masked scores, the wave-cooperative soft-max, the FFN, LayerNorm, pooling, bias-gradient column sums and d position_emb.
// ONE launch forward, ONE launch backward per block (+ fx_colsum over the per-workgroup rows of weight gradients).
// The backward recomputes the forward with the forward's own device functions (the same bits; neither P nor a
// log-sum-exp is kept: fx_mhsa.hip says why), and Q, K, V a second time after the FFN half has used their LDS
// (6 L1 dm^2 flops, which keeps the image inside 160 KiB at L1 = dm = 64).
// The six weight-gradient matrices stay in registers over the workgroup's samples (entry e of a matrix belongs to
// thread e % 256), the bias / LayerNorm gradients and d position_emb in LDS (one owner thread per entry).
// Soft-max and LayerNorm rows are wave-cooperative: a row per wave, a lane per column (L1, dm <= 64 = one wave).
//
// Backward LDS map (N = L1 * (dm | 1) floats per array, S = max(N, HG * L1 * (L1 | 1))):
//   sX  X                                   (whole sample)
//   a1  Q -> s before LN1 -> xhat1 -> Q     a2  K -> s (after LN1) -> dO
//   a3  V -> h = lrelu(z1) -> K             a4  O -> V -> dV
//   a5  dQ                                  a6  dK
//   sp  P -> out before LN2 -> xhat2 -> dz1 -> P        sd  g -> d out -> ds -> d s -> dP / dS
//   + rstd1, rstd2, pad (64 each), the bias gradients (10 dm), d position_emb (L1 * D), the weights when they fit.
#include "fx_attn_lds.h"
#include "fx_seq_parts.h"

#define BT_T FX_ATTN_T
#define BT_MAX FX_ATTN_MAX
#define BT_FWD_GRID 1024
#define BT_BWD_GRID 256      // = rows of the weight-gradient partials
#define BT_SLOPE 0.01f       // nn.LeakyReLU()
#define BT_EPS 1e-5f         // nn.LayerNorm

enum { BT_POOL_NONE = 0, BT_POOL_MEAN = 1, BT_POOL_SUM = 2, BT_POOL_TARGET = 3 };

struct BstArgs {
    fx_seq_parts in;         // the sample's parts
    const float* pos;        // position_emb [L1, D] or null
    fx_seq_parts din;        // where the parts' gradients go (backward)
    const int32_t* ids;      // [B, L] ids of the first sequence field, row stride ids_ld; null: nothing is padded
    int64_t ids_ld;
    int64_t B;
    int L1, dm, H, hd, HG, D, np, S;
    const float* W[6];       // Wq, Wk, Wv (rows of in_proj_weight), out_proj, ffn.0, ffn.2: each [dm, dm]
    const float* in_b;       // [3 dm]
    const float* out_b;
    const float* b1;
    const float* b2;
    const float* ln[4];      // ln1 weight, bias, ln2 weight, bias
    float scale;
    int layer_norm, residual, causal, pool;
    float* Y;
    const float* dY;
    int dx_acc;
    float* partial;          // [grid, n_grad]
    int64_t n_grad;
};

// X of sample b, assembled from its parts, and the padding flags
__device__ __forceinline__ void bt_load_x(const BstArgs& p, int64_t b, float* sX, int* sPad) {
    const int L1 = p.L1, L = L1 - 1, dm = p.dm, D = p.D, DS = dm | 1;
    for (int idx = threadIdx.x; idx < L1 * dm; idx += BT_T) {
        const int f = idx / dm, c = idx - f * dm, part = c / D, cc = c - part * D;
        float v;
        if (part < p.np) {
            v = f == L ? p.in.tgt[part][fx_parts_tgt_off(p.in, part, b, cc)]
                       : p.in.seq[part][fx_parts_seq_off(p.in, part, b, f, cc)];
        } else {
            v = p.pos[f * D + cc];
        }
        sX[f * DS + c] = v;
    }
    for (int f = threadIdx.x; f < L1; f += BT_T)
        sPad[f] = (f < L && p.ids != nullptr && p.ids[b * p.ids_ld + f] == 0) ? 1 : 0;
}

__device__ __forceinline__ FxAttnDims bt_dims(const BstArgs& p) { return {p.L1, p.dm, p.dm, p.hd, p.HG, p.scale}; }

// Q, K, V = X in_w^T + in_b.  Private like mh_project: shared, it cost k_bst_bwd<false, 16> 3.7 %.
template <bool WLDS>
__device__ __forceinline__ void bt_project(const BstArgs& p, const FxAttnW<6, WLDS>& w, const float* sX, float* sQ,
                                           float* sK, float* sV) {
    const int L1 = p.L1, dm = p.dm, DS = dm | 1;
    for (int idx = threadIdx.x; idx < L1 * dm; idx += BT_T) {
        const int f = idx / dm, a = idx - f * dm;
        float q = 0.f, k = 0.f, v = 0.f;
        for (int d = 0; d < dm; ++d) {
            const float xv = sX[f * DS + d];
            q = fmaf(xv, w(0, a, d), q);
            k = fmaf(xv, w(1, a, d), k);
            v = fmaf(xv, w(2, a, d), v);
        }
        sQ[f * DS + a] = q + p.in_b[a];
        sK[f * DS + a] = k + p.in_b[dm + a];
        sV[f * DS + a] = v + p.in_b[2 * dm + a];
    }
}

// scores of the heads h0 .. h0+hg-1: sS[hh][i][j] = scale * Q_i . K_j, -inf where masked.  Private: through
// fx_attn_scores with the mask as a functor k_bst_fwd<false> measured 0.8 % slower.
__device__ __forceinline__ void bt_scores(const BstArgs& p, int h0, int hg, const float* sQ, const float* sK,
                                          const int* sPad, float* sS) {
    const int L1 = p.L1, DS = p.dm | 1, LS = L1 | 1, hd = p.hd, LL = L1 * L1;
    for (int idx = threadIdx.x; idx < hg * LL; idx += BT_T) {
        const int hh = idx / LL, r = idx - hh * LL, i = r / L1, j = r - i * L1;
        const float* q = sQ + i * DS + (h0 + hh) * hd;
        const float* k = sK + j * DS + (h0 + hh) * hd;
        float s = 0.f;
        for (int c = 0; c < hd; ++c) s = fmaf(q[c], k[c], s);
        const bool masked = (sPad[j] && i != j) || (p.causal && j > i);
        sS[(hh * L1 + i) * LS + j] = masked ? FX_ATTN_NEG_INF : s * p.scale;
    }
}

// this lane's entry of the stable soft-max of one score row (the diagonal is never masked: the maximum is finite).
// A wave per row, butterfly maximum and sum: fx_mhsa.hip's thread-per-row soft-max sums serially, so the two are
// not one function.
__device__ __forceinline__ float bt_softmax_lane(const float* row, int L1, int lane) {
    const float v = lane < L1 ? row[lane] : FX_ATTN_NEG_INF;
    const float m = fx_wave_max(v);
    const float e = lane < L1 ? expf(v - m) : 0.f;
    const float sum = fx_wave_sum(e);
    return e / sum;
}

// the heads h0 .. h0+hg-1: P into sS, O = P V into this group's columns of sO
__device__ __forceinline__ void bt_attend(const BstArgs& p, int h0, int hg, const float* sQ, const float* sK,
                                          const float* sV, const int* sPad, float* sS, float* sO) {
    const int L1 = p.L1, DS = p.dm | 1, LS = L1 | 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bt_scores(p, h0, hg, sQ, sK, sPad, sS);
    __syncthreads();
    for (int r = wave; r < hg * L1; r += BT_T / 64) {
        const float pv = bt_softmax_lane(sS + r * LS, L1, lane);
        if (lane < L1) sS[r * LS + lane] = pv;
    }
    __syncthreads();
    fx_attn_pv(bt_dims(p), h0, hg, sS, sV, [&](int i, int a, float o) { sO[i * DS + a] = o; });
}

// out[f][a] = in[f] . W_m[a] + bias[a] (+ add[f][a]), LeakyReLU on the way out when LRELU
template <bool WLDS, bool LRELU>
__device__ __forceinline__ void bt_linear(const FxAttnW<6, WLDS>& w, int m, const float* bias, const float* in,
                                          const float* add, float* out, int L1, int dm) {
    const int DS = dm | 1;
    for (int idx = threadIdx.x; idx < L1 * dm; idx += BT_T) {
        const int f = idx / dm, a = idx - f * dm;
        float s = 0.f;
        for (int d = 0; d < dm; ++d) s = fmaf(in[f * DS + d], w(m, a, d), s);
        s += bias[a];
        if (add != nullptr) s += add[f * DS + a];
        if constexpr (LRELU) s = s > 0.f ? s : BT_SLOPE * s;
        out[f * DS + a] = s;
    }
}

// LayerNorm of the rows of x: y = xhat * gamma + beta (y nullable, may be x); keep: xhat over x, 1 / std into sR
__device__ __forceinline__ void bt_layernorm(float* x, float* y, const float* gamma, const float* beta, float* sR,
                                             bool keep, int L1, int dm) {
    const int DS = dm | 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_n = 1.f / (float)dm;
    for (int f = wave; f < L1; f += BT_T / 64) {
        const float v = lane < dm ? x[f * DS + lane] : 0.f;
        const float mean = fx_wave_sum(v) * inv_n;
        const float d = lane < dm ? v - mean : 0.f;
        const float var = fx_wave_sum(d * d) * inv_n;
        const float rstd = 1.f / sqrtf(var + BT_EPS);
        const float xh = d * rstd;
        if (lane < dm) {
            if (keep) x[f * DS + lane] = xh;
            if (y != nullptr) y[f * DS + lane] = xh * gamma[lane] + beta[lane];
        }
        if (keep && lane == 0) sR[f] = rstd;
    }
}

// g (the gradient of LayerNorm's output, rows) -> the gradient of its input, in place
__device__ __forceinline__ void bt_layernorm_bwd(float* g, const float* xh, const float* sR, const float* gamma,
                                                 int L1, int dm) {
    const int DS = dm | 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_n = 1.f / (float)dm;
    for (int f = wave; f < L1; f += BT_T / 64) {
        const float gy = lane < dm ? g[f * DS + lane] * gamma[lane] : 0.f;
        const float x = lane < dm ? xh[f * DS + lane] : 0.f;
        const float m1 = fx_wave_sum(gy) * inv_n;
        const float m2 = fx_wave_sum(gy * x) * inv_n;
        if (lane < dm) g[f * DS + lane] = sR[f] * (gy - m1 - x * m2);
    }
}

// sum over the rows: acc_g[c] += sum_f g[f][c] * xh[f][c] (xh nullable: skipped), acc_b[c] += sum_f g[f][c]
__device__ __forceinline__ void bt_colsum(const float* g, const float* xh, float* acc_g, float* acc_b, int L1,
                                          int dm) {
    const int DS = dm | 1;
    for (int c = threadIdx.x; c < dm; c += BT_T) {
        float sg = 0.f, sb = 0.f;
        for (int f = 0; f < L1; ++f) {
            const float gv = g[f * DS + c];
            if (xh != nullptr) sg = fmaf(gv, xh[f * DS + c], sg);
            sb += gv;
        }
        if (xh != nullptr) acc_g[c] += sg;
        acc_b[c] += sb;
    }
}

// out[f][c] = sum_a in[f][a] W_m[a][c], times LeakyReLU' where h is given, onto out where add
template <bool WLDS>
__device__ __forceinline__ void bt_linear_t(const FxAttnW<6, WLDS>& w, int m, const float* in, const float* h, bool add,
                                            float* out, int L1, int dm) {
    const int DS = dm | 1;
    for (int idx = threadIdx.x; idx < L1 * dm; idx += BT_T) {
        const int f = idx / dm, c = idx - f * dm;
        float s = 0.f;
        for (int a = 0; a < dm; ++a) s = fmaf(in[f * DS + a], w(m, a, c), s);
        if (h != nullptr) s *= h[f * DS + c] > 0.f ? 1.f : BT_SLOPE;
        out[f * DS + c] = add ? out[f * DS + c] + s : s;
    }
}

// dX[f][c] of sample b through the description of the parts; the position columns go to the LDS sum
__device__ __forceinline__ void bt_put_dx(const BstArgs& p, int64_t b, int f, int c, float v, bool acc,
                                          float* sDpos) {
    const int D = p.D, part = c / D, cc = c - part * D;
    if (part < p.np) {
        const bool tgt = f == p.L1 - 1;
        fx_parts_put(tgt ? p.din.tgt[part] : p.din.seq[part],
                     tgt ? fx_parts_tgt_off(p.din, part, b, cc) : fx_parts_seq_off(p.din, part, b, f, cc), v, acc);
    } else {
        sDpos[f * D + cc] += v;
    }
}

template <bool WLDS>
__global__ __launch_bounds__(BT_T) void k_bst_fwd(BstArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L1 = p.L1, dm = p.dm, DS = dm | 1, N = L1 * DS;
    float* sX = smem;
    float* sQ = sX + N;
    float* sK = sQ + N;
    float* sV = sK + N;
    float* sO = sV + N;
    float* sS = sO + N;
    int* sPad = reinterpret_cast<int*>(sS + p.S);
    float* sW = reinterpret_cast<float*>(sPad + BT_MAX);
    const FxAttnW<6, WLDS> w = fx_attn_weights<6, WLDS>(p.W, 6, dm, dm, sW);
    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        __syncthreads();
        bt_load_x(p, b, sX, sPad);
        __syncthreads();
        bt_project<WLDS>(p, w, sX, sQ, sK, sV);
        for (int h0 = 0; h0 < p.H; h0 += p.HG) {
            __syncthreads();
            bt_attend(p, h0, p.H - h0 < p.HG ? p.H - h0 : p.HG, sQ, sK, sV, sPad, sS, sO);
        }
        __syncthreads();
        bt_linear<WLDS, false>(w, 3, p.out_b, sO, p.residual ? sX : nullptr, sQ, L1, dm);     // s
        __syncthreads();
        if (p.layer_norm) {
            bt_layernorm(sQ, sQ, p.ln[0], p.ln[1], nullptr, false, L1, dm);
            __syncthreads();
        }
        bt_linear<WLDS, true>(w, 4, p.b1, sQ, nullptr, sK, L1, dm);                           // h
        __syncthreads();
        bt_linear<WLDS, false>(w, 5, p.b2, sK, p.residual ? sQ : nullptr, sO, L1, dm);        // out
        __syncthreads();
        if (p.layer_norm) {
            bt_layernorm(sO, sO, p.ln[2], p.ln[3], nullptr, false, L1, dm);
            __syncthreads();
        }
        if (p.pool == BT_POOL_NONE) {
            for (int idx = threadIdx.x; idx < L1 * dm; idx += BT_T) {
                const int f = idx / dm, c = idx - f * dm;
                p.Y[(b * L1 + f) * dm + c] = sO[f * DS + c];
            }
        } else {
            for (int c = threadIdx.x; c < dm; c += BT_T) {
                float s = 0.f;
                if (p.pool == BT_POOL_TARGET) {
                    s = sO[(L1 - 1) * DS + c];
                } else {
                    int cnt = 0;
                    for (int f = 0; f < L1; ++f)
                        if (!sPad[f]) {
                            s += sO[f * DS + c];
                            ++cnt;
                        }
                    if (p.pool == BT_POOL_MEAN) s = s / ((float)cnt + 1e-12f);
                }
                p.Y[b * dm + c] = s;
            }
        }
    }
}

// R: entries per thread of one weight-gradient matrix (dm * dm <= 256 R)
template <bool WLDS, int R>
__global__ __launch_bounds__(BT_T) void k_bst_bwd(BstArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FxAttnDims g = bt_dims(p);
    const int L1 = p.L1, dm = p.dm, DS = dm | 1, N = L1 * DS, LS = L1 | 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* sX = smem;
    float* a1 = sX + N;
    float* a2 = a1 + N;
    float* a3 = a2 + N;
    float* a4 = a3 + N;
    float* a5 = a4 + N;
    float* a6 = a5 + N;
    float* sp = a6 + N;
    float* sd = sp + p.S;
    float* sR1 = sd + p.S;
    float* sR2 = sR1 + BT_MAX;
    int* sPad = reinterpret_cast<int*>(sR2 + BT_MAX);
    float* sDB = reinterpret_cast<float*>(sPad + BT_MAX);     // in_b 3dm | out_b | b1 | b2 | ln1 w, b | ln2 w, b
    float* sDpos = sDB + 10 * dm;
    const int n_pos = p.pos != nullptr ? L1 * p.D : 0;
    float* sW = sDpos + n_pos;
    const FxAttnW<6, WLDS> w = fx_attn_weights<6, WLDS>(p.W, 6, dm, dm, sW);
    for (int i = threadIdx.x; i < 10 * dm + n_pos; i += BT_T) sDB[i] = 0.f;
    float acc[6][R];
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
    float* s_in = p.layer_norm ? a2 : a1;       // s, the FFN's input

    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        __syncthreads();
        bt_load_x(p, b, sX, sPad);
        __syncthreads();
        // ---- the forward again, up to the input of LayerNorm 2
        bt_project<WLDS>(p, w, sX, a1, a2, a3);
        for (int h0 = 0; h0 < p.H; h0 += p.HG) {
            __syncthreads();
            bt_attend(p, h0, p.H - h0 < p.HG ? p.H - h0 : p.HG, a1, a2, a3, sPad, sp, a4);
        }
        __syncthreads();
        bt_linear<WLDS, false>(w, 3, p.out_b, a4, p.residual ? sX : nullptr, a1, L1, dm);
        __syncthreads();
        if (p.layer_norm) {
            bt_layernorm(a1, a2, p.ln[0], p.ln[1], sR1, true, L1, dm);          // a1 = xhat1, a2 = s
            __syncthreads();
        }
        bt_linear<WLDS, true>(w, 4, p.b1, s_in, nullptr, a3, L1, dm);           // a3 = h
        __syncthreads();
        bt_linear<WLDS, false>(w, 5, p.b2, a3, p.residual ? s_in : nullptr, sp, L1, dm);
        // ---- the upstream gradient of every position
        {
            int cnt = 0;
            if (p.pool == BT_POOL_MEAN)
                for (int f = 0; f < L1; ++f) cnt += sPad[f] ? 0 : 1;
            const float inv = 1.f / ((float)cnt + 1e-12f);
            for (int idx = threadIdx.x; idx < L1 * dm; idx += BT_T) {
                const int f = idx / dm, c = idx - f * dm;
                float g;
                if (p.pool == BT_POOL_NONE) g = p.dY[(b * L1 + f) * dm + c];
                else if (p.pool == BT_POOL_TARGET) g = f == L1 - 1 ? p.dY[b * dm + c] : 0.f;
                else if (sPad[f]) g = 0.f;
                else g = p.pool == BT_POOL_MEAN ? p.dY[b * dm + c] * inv : p.dY[b * dm + c];
                sd[f * DS + c] = g;
            }
        }
        __syncthreads();
        if (p.layer_norm) {
            bt_layernorm(sp, nullptr, nullptr, nullptr, sR2, true, L1, dm);     // sp = xhat2
            __syncthreads();
            bt_colsum(sd, sp, sDB + 8 * dm, sDB + 9 * dm, L1, dm);
            __syncthreads();
            bt_layernorm_bwd(sd, sp, sR2, p.ln[2], L1, dm);
            __syncthreads();
        }
        // ---- FFN: sd = d out
        fx_attn_acc_dw<R>(acc[5], sd, a3, L1, dm, dm);
        bt_colsum(sd, nullptr, nullptr, sDB + 5 * dm, L1, dm);
        bt_linear_t<WLDS>(w, 5, sd, a3, false, sp, L1, dm);                     // sp = dz1
        __syncthreads();
        fx_attn_acc_dw<R>(acc[4], sp, s_in, L1, dm, dm);
        bt_colsum(sp, nullptr, nullptr, sDB + 4 * dm, L1, dm);
        bt_linear_t<WLDS>(w, 4, sp, nullptr, p.residual != 0, sd, L1, dm);      // sd = ds
        __syncthreads();
        if (p.layer_norm) {
            bt_colsum(sd, a1, sDB + 6 * dm, sDB + 7 * dm, L1, dm);
            __syncthreads();
            bt_layernorm_bwd(sd, a1, sR1, p.ln[0], L1, dm);
            __syncthreads();
        }
        // ---- output projection: sd = d s before LayerNorm 1
        fx_attn_acc_dw<R>(acc[3], sd, a4, L1, dm, dm);
        bt_colsum(sd, nullptr, nullptr, sDB + 3 * dm, L1, dm);
        bt_linear_t<WLDS>(w, 3, sd, nullptr, false, a2, L1, dm);                // a2 = dO
        if (p.residual)       // the residual's share of dX; the same thread adds the rest below
            for (int idx = threadIdx.x; idx < L1 * dm; idx += BT_T) {
                const int f = idx / dm, c = idx - f * dm;
                bt_put_dx(p, b, f, c, sd[f * DS + c], p.dx_acc != 0, sDpos);
            }
        __syncthreads();
        // ---- attention: Q, K, V once more, then head group by head group
        bt_project<WLDS>(p, w, sX, a1, a3, a4);
        for (int h0 = 0; h0 < p.H; h0 += p.HG) {
            const int hg = p.H - h0 < p.HG ? p.H - h0 : p.HG;
            __syncthreads();
            bt_scores(p, h0, hg, a1, a3, sPad, sp);
            fx_attn_dp(g, h0, hg, a2, a4, sd);
            __syncthreads();
            // row by row: P = softmax(S), then dS = P (dP - sum_j P dP) * scale
            for (int r = wave; r < hg * L1; r += BT_T / 64) {
                const float pv = bt_softmax_lane(sp + r * LS, L1, lane);
                const float dp = lane < L1 ? sd[r * LS + lane] : 0.f;
                const float delta = fx_wave_sum(pv * dp);
                if (lane < L1) {
                    sp[r * LS + lane] = pv;
                    sd[r * LS + lane] = pv * (dp - delta) * p.scale;
                }
            }
            __syncthreads();
            fx_attn_dqkv(g, h0, hg, sp, sd, a2, a1, a3, a4, a5, a6);      // a4 = dV, a5 = dQ, a6 = dK
        }
        __syncthreads();
        // dX = dQ Wq + dK Wk + dV Wv (+ the residual's share, already there)
        fx_attn_dx(g, w, a5, a6, a4, [&](int f, int c, float s) {
            bt_put_dx(p, b, f, c, s, p.residual != 0 || p.dx_acc != 0, sDpos);
        });
        bt_colsum(a5, nullptr, nullptr, sDB, L1, dm);
        bt_colsum(a6, nullptr, nullptr, sDB + dm, L1, dm);
        bt_colsum(a4, nullptr, nullptr, sDB + 2 * dm, L1, dm);
        fx_attn_acc_dw<R>(acc[0], a5, sX, L1, dm, dm);
        fx_attn_acc_dw<R>(acc[1], a6, sX, L1, dm, dm);
        fx_attn_acc_dw<R>(acc[2], a4, sX, L1, dm, dm);
    }
    __syncthreads();
    float* part = p.partial + (int64_t)blockIdx.x * p.n_grad;
    const int DD = dm * dm;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = threadIdx.x + r * BT_T;
        if (e < DD) {
#pragma unroll
            for (int m = 0; m < 6; ++m) part[m * DD + e] = acc[m][r];
        }
    }
    for (int i = threadIdx.x; i < 10 * dm + n_pos; i += BT_T) part[6 * DD + i] = sDB[i];
}

static inline int64_t bt_n_grad(int L1, int dm, int pos_D) {
    return 6 * (int64_t)dm * dm + 10 * (int64_t)dm + (int64_t)L1 * pos_D;
}

static int bt_check(const char* who, const fx_seq_parts* in, const int32_t* ids, int64_t ids_ld, int64_t B, int32_t L1,
                    int32_t dm, int32_t H, const fx_bst_weights* w, int32_t layer_norm, int32_t pool) {
    FX_CHECK_ARG(in && w, "%s: null input / weights description", who);
    FX_CHECK_ARG(L1 >= 1 && L1 <= BT_MAX, "%s: L1=%d, limit 1 <= L1 <= 64", who, L1);
    FX_CHECK_ARG(dm >= 1 && dm <= BT_MAX, "%s: dm=%d, limit 1 <= dm <= 64", who, dm);
    FX_CHECK_ARG(H >= 1 && dm % H == 0, "%s: H=%d does not divide dm=%d", who, H, dm);
    FX_CHECK_ARG(in->n_parts >= 1 && in->n_parts <= 3, "%s: n_parts=%d, limit 1 <= n_parts <= 3", who, in->n_parts);
    FX_CHECK_ARG(in->D >= 1 && dm % in->D == 0 && dm / in->D <= 4, "%s: D=%d must divide dm=%d at most 4 times", who,
                 in->D, dm);
    FX_CHECK_ARG(dm / in->D == in->n_parts + (w->pos ? 1 : 0), "%s: dm=%d is not (n_parts=%d%s) * D=%d", who, dm,
                 in->n_parts, w->pos ? " + position_emb" : "", in->D);
    FX_CHECK_ARG(pool >= BT_POOL_NONE && pool <= BT_POOL_TARGET, "%s: pool=%d", who, pool);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    if (B == 0) return FX_OK;
    for (int i = 0; i < in->n_parts; ++i) {
        if (int st = fx_parts_check_tgt(who, "part", in, i, in->D, false)) return st;
        if (L1 == 1) continue;
        if (int st = fx_parts_check_seq(who, "part", in, i, in->D, L1 - 1, false)) return st;
    }
    FX_CHECK_ARG(!ids || ids_ld >= L1 - 1, "%s: ids stride %lld < L", who, (long long)ids_ld);
    FX_CHECK_ARG(w->in_w && w->in_b && w->out_w && w->out_b && w->w1 && w->b1 && w->w2 && w->b2,
                 "%s: null weight or bias", who);
    FX_CHECK_ARG(!layer_norm || (w->ln1_w && w->ln1_b && w->ln2_w && w->ln2_b), "%s: null LayerNorm parameter", who);
    return FX_OK;
}

static BstArgs bt_args(const fx_seq_parts* in, const int32_t* ids, int64_t ids_ld, int64_t B, int32_t L1, int32_t dm,
                       int32_t H, const fx_bst_weights* w, int32_t layer_norm, int32_t residual, int32_t causal,
                       int32_t pool) {
    BstArgs p;
    memset(&p, 0, sizeof(p));
    p.in = *in;
    p.pos = w->pos;
    p.ids = ids; p.ids_ld = ids_ld; p.B = B;
    p.L1 = L1; p.dm = dm; p.H = H; p.hd = dm / H; p.D = in->D; p.np = in->n_parts;
    p.HG = fx_attn_heads_per_pass(L1, H);
    const int N = L1 * (dm | 1), SS = p.HG * L1 * (L1 | 1);
    p.S = N > SS ? N : SS;
    for (int m = 0; m < 3; ++m) p.W[m] = w->in_w + (int64_t)m * dm * dm;
    p.W[3] = w->out_w; p.W[4] = w->w1; p.W[5] = w->w2;
    p.in_b = w->in_b; p.out_b = w->out_b; p.b1 = w->b1; p.b2 = w->b2;
    p.ln[0] = w->ln1_w; p.ln[1] = w->ln1_b; p.ln[2] = w->ln2_w; p.ln[3] = w->ln2_b;
    p.scale = (float)(1.0 / sqrt((double)p.hd));
    p.layer_norm = layer_norm ? 1 : 0;
    p.residual = residual ? 1 : 0;
    p.causal = causal ? 1 : 0;
    p.pool = pool;
    return p;
}

// LDS: X and n_rows more [L1, dm] arrays, n_score score buffers of S floats, the small arrays (+ the six weights)
static inline FxAttnLds bt_lds(const BstArgs& p, int n_rows, int n_score, size_t small) {
    return fx_attn_lds(fx_attn_lds_floats(p.L1, p.dm, p.dm, n_rows, n_score, p.S, small), 6, p.dm, p.dm);
}

extern "C" void fx_bst_limits(int32_t* limits) {
    limits[0] = BT_MAX;
    limits[1] = BT_MAX;
    limits[2] = BT_FWD_GRID;
    limits[3] = BT_BWD_GRID;
}

extern "C" int64_t fx_bst_grad_floats(int32_t L1, int32_t dm, int32_t pos_D) { return bt_n_grad(L1, dm, pos_D); }

extern "C" int64_t fx_bst_workspace_floats(int64_t B, int32_t L1, int32_t dm, int32_t pos_D) {
    const int64_t G = B < BT_BWD_GRID ? (B > 0 ? B : 1) : BT_BWD_GRID;
    const int64_t n4 = fx_al4(bt_n_grad(L1, dm, pos_D));
    return G * n4 + FX_COLSUM_CHUNKS * n4;
}

extern "C" int fx_bst_block_fwd(const fx_seq_parts* in, const int32_t* ids, int64_t ids_ld, int64_t B, int32_t L1,
                                int32_t dm, int32_t H, const fx_bst_weights* w, int32_t layer_norm, int32_t residual,
                                int32_t causal, int32_t pool, float* Y, fx_stream_t stream) {
    if (int st = bt_check("fx_bst_block_fwd", in, ids, ids_ld, B, L1, dm, H, w, layer_norm, pool)) return st;
    FX_CHECK_ARG(B == 0 || Y, "fx_bst_block_fwd: null Y");
    if (B == 0) return FX_OK;
    BstArgs p = bt_args(in, ids, ids_ld, B, L1, dm, H, w, layer_norm, residual, causal, pool);
    p.Y = Y;
    const FxAttnLds l = bt_lds(p, 4, 1, BT_MAX);      // (L1 = dm = 64 and 119 more shapes leave the weights in HBM)
    const unsigned grid = (unsigned)(B < BT_FWD_GRID ? B : BT_FWD_GRID);
    hipStream_t s = fx_hip_stream(stream);
    return l.wlds ? fx_attn_launch<k_bst_fwd<true>>(p, grid, l.bytes, s)
                  : fx_attn_launch<k_bst_fwd<false>>(p, grid, l.bytes, s);
}

template <bool WLDS>
static int bt_launch_bwd(const BstArgs& p, unsigned grid, size_t lds, hipStream_t s) {
    const int DD = p.dm * p.dm;
    if (DD <= BT_T) return fx_attn_launch<k_bst_bwd<WLDS, 1>>(p, grid, lds, s);
    if (DD <= 4 * BT_T) return fx_attn_launch<k_bst_bwd<WLDS, 4>>(p, grid, lds, s);
    if (DD <= 9 * BT_T) return fx_attn_launch<k_bst_bwd<WLDS, 9>>(p, grid, lds, s);
    return fx_attn_launch<k_bst_bwd<WLDS, 16>>(p, grid, lds, s);
}

extern "C" int fx_bst_block_bwd(const fx_seq_parts* in, const int32_t* ids, int64_t ids_ld, int64_t B, int32_t L1,
                                int32_t dm, int32_t H, const fx_bst_weights* w, int32_t layer_norm, int32_t residual,
                                int32_t causal, int32_t pool, const float* dY, const fx_seq_parts* din,
                                int32_t dx_accumulate, float* grads, float* workspace, fx_stream_t stream) {
    if (int st = bt_check("fx_bst_block_bwd", in, ids, ids_ld, B, L1, dm, H, w, layer_norm, pool)) return st;
    FX_CHECK_ARG(B > 0, "fx_bst_block_bwd: B=%lld", (long long)B);
    FX_CHECK_ARG(dY && din && grads && workspace, "fx_bst_block_bwd: null dY / gradient description / grads / workspace");
    FX_CHECK_ARG(fx_al16(workspace), "fx_bst_block_bwd: the workspace is not 16-byte aligned");
    for (int i = 0; i < in->n_parts; ++i) {
        if (int st = fx_parts_check_tgt("fx_bst_block_bwd", "gradient of part", din, i, in->D, true)) return st;
        if (L1 == 1) continue;
        if (int st = fx_parts_check_seq("fx_bst_block_bwd", "gradient of part", din, i, in->D, L1 - 1, true)) return st;
    }
    BstArgs p = bt_args(in, ids, ids_ld, B, L1, dm, H, w, layer_norm, residual, causal, pool);
    p.din = *din;
    p.dY = dY;
    p.dx_acc = dx_accumulate ? 1 : 0;
    const int pos_D = w->pos ? in->D : 0;
    const int64_t n = bt_n_grad(L1, dm, pos_D), n4 = fx_al4(n);
    p.partial = workspace;
    p.n_grad = n4;
    const size_t small = 3 * BT_MAX + 10 * (size_t)dm + (size_t)L1 * pos_D;
    const FxAttnLds l = bt_lds(p, 6, 2, small);
    FX_CHECK_ARG(l.bytes <= FX_ATTN_LDS_MAX, "fx_bst_block_bwd: %zu bytes of LDS", l.bytes);
    const unsigned grid = (unsigned)(B < BT_BWD_GRID ? B : BT_BWD_GRID);
    hipStream_t s = fx_hip_stream(stream);
    const int st = l.wlds ? bt_launch_bwd<true>(p, grid, l.bytes, s) : bt_launch_bwd<false>(p, grid, l.bytes, s);
    if (st) return st;
    // the workgroups' rows -> grads, two fixed-order stages
    return fx_colsum(workspace, n4, grid, n, grads, workspace + (int64_t)grid * n4, stream);
}
