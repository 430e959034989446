// fx_euler.hip — EulerNet's Euler interaction layer on the matrix cores, and its polar front end.
// Reference: model_zoo/EulerNet/src/EulerNet.py:139-170 (EulerInteractionLayer.forward), :90 (the front end).
// A layer's pair lives in ONE tensor RP [2, B, Fi, D] (r | p), its output in OP [2, B, O, D]:
//     a = 0.5 log(r^2 + p^2 + 1e-8),  t = atan2(p, r)
//     ul[b, o, d] = sum_f orders[f, o] a[b, f, d] + bias_lam[d, o],   ut likewise from t and bias_theta
//     o_r = relu(zr) + exp(ul) cos(ut),  o_p = relu(zp) + exp(ul) sin(ut),  then LayerNorm over d per (b, o)
// Z [2B, O D] = RP.view(2B, Fi D) im.weight^T + im.bias is the caller's GEMM (pre-activation: the kernel applies the
// ReLU, and the backward mask needs nothing but Z).  exp / cos / sin are never stored: the backward recomputes a, t,
// ul, ut and the pre-norm outputs from RP, Z and the saved (mean, rstd) [2, B, O].
//
// Work split (the skeleton of fx_lognet.hip): the column axis is n = b D + d, K = the fields, products on
// v_mfma_f32_16x16x4_f32 with lane (r16 = lane & 15, kk = lane >> 4) holding element (r16, k = kk) of A and of B and
// rows 4 kk + i of column r16 of the result.  A workgroup's tile is S whole samples (S D <= 128 columns, S <= 32), so
// every LayerNorm group lies in one workgroup; a wave owns 2 x 16 of the tile's columns.  A lane computes its slice
// of a AND t once from RP into registers (two operand sets, every log and atan2 taken once per pass); inter_orders
// [<= 64, <= 64] sits in LDS once per workgroup, transposed ([o, f], row stride 68 = 4 mod 64), and is the shared
// operand of both products.  a x orders gives u[n = 4 kk + i, o = r16]: a lane holds 4 consecutive columns of one
// neuron, 16-byte accesses to Z / OP / dOP / dZ when D % 4 == 0.
//   k_eu_fwd: per 16 neurons: both products, biases, exp / cos / sin, + relu(Z); with the norm on, the pre-norm tile
//     goes through LDS once ([column, 16 neurons], stride 17), one thread per (half, sample, neuron) group takes the
//     two-pass mean and centred squares, and every lane normalises the values it still holds; OP is written once.
//   k_eu_bwd: the same recompute, then per 16 neurons: LayerNorm backward in-group (dy and yhat staged, the group's
//     two sums by one thread), dZ (masked by Z > 0), dul and dut; those are staged [column, 16 neurons] and are the B
//     operand of da[f, n] += orders[f, o] dul[o, n] (K = O, the 4 x 2 x 2 accumulator tiles persist over the
//     neurons), and leave for k_eu_bwd_dw together with a, t.  The explicit part of dRP follows from da, dt and the
//     polar derivatives; atan2's are exactly 0 at r = p = 0, as torch masks them.  The bias and LayerNorm parameter
//     gradients are per-workgroup partial rows in global memory, each slot owned by one thread.
//   k_eu_bwd_dw: d orders[f, o] = sum_n a[n, f] dul[n, o] + t[n, f] dut[n, o] per slab of columns: a | t tiles through
//     LDS, dul | dut read in place as the chained B operand (K = the slab's columns).
//   k_eu_polar_fwd / _bwd: RP = mu (cos E | sin E); dE and the per-chunk partials of dmu.
// All partials meet in fx_rowsum in a fixed order; no atomics: two runs give the same bits, and launch counts depend
// on shapes only.  sinf, cosf, expf, logf, atan2f are the full-range library functions (ut is unbounded).
#include "fx_common.h"
#include "fx_rowsum.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define EU_MAX_F 64
#define EU_MAX_D 64
#define EU_MAX_O 64
#define EU_NT 256
#define EU_CT 2                 // 16-column tiles per wave
#define EU_COLS (64 * EU_CT)    // most columns of a workgroup tile
#define EU_MAX_S 32             // most samples of a workgroup tile
#define EU_WS 68                // LDS row stride of the [64, 64] orders tile: = 4 mod 64
#define EU_SS 17                // LDS stride of a staged column's 16 neurons
#define EU_KS (EU_MAX_F / 4)
#define EU_MAX_WG 512           // workgroups of the layer kernels: the rows of their partial sums
#define EU_MAX_SLABS 256        // column slabs of the orders-gradient kernel
#define EU_CHUNKS 256           // sample chunks of the polar backward
#define EU_LAM_EPS 1e-8f

struct EuArgs {
    const float* RP; const float* Z; float* OP;
    const float* dOP; float* dZ; float* dRP;
    int64_t B, N, half_in, half_out;            // N = B D columns; floats of one half of RP / of OP and Z
    int Fi, D, O, KS, FP, FT, OT, OS;           // KS = ceil(Fi / 4), FP = 4 KS, FT = ceil(Fi / 16), OT = ceil(O / 16)
    int S, TC, ln, vec4;                        // samples and columns of a tile; OS = O rounded up to 4
    const float* orders; const float *blam, *bth;
    const float *wr, *br, *wp, *bp; float eps;
    float* stats;                               // mean [2, B, O] | rstd [2, B, O]
    float* at;                                  // a | t [2, N, FP]
    float* du;                                  // dul | dut [2, N, OS]
    float* bpart;                               // [workgroups, 2, D, O]
    float* lnpart;                              // [workgroups, 16, 2, 2, D]
    float* dwpart;                              // [slabs, Fi, O]
};

__device__ __forceinline__ f32x4 eu_mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// inter_orders [Fi, O] into wt [o, f] (zeros past O and past Fi)
__device__ __forceinline__ void eu_stage_orders(const EuArgs* ka, float* wt) {
    for (int idx = threadIdx.x; idx < 64 * 64; idx += EU_NT) {
        const int f = idx >> 6, o = idx & 63;
        wt[o * EU_WS + f] = (f < ka->Fi && o < ka->O) ? ka->orders[f * ka->O + o] : 0.f;
    }
}

// the lane's slices of a and t for local column lc of the tile at sample b0: a[ks] = a[n, f = 4 ks + kk]
__device__ __forceinline__ void eu_at_regs(const EuArgs* ka, int64_t b0, int lc, int kk, float (&a)[EU_KS],
                                           float (&t)[EU_KS]) {
    const int D = ka->D, s = lc / D;
    const bool ok = lc < ka->TC && b0 + s < ka->B;
    const float* rp = ka->RP + (ok ? (b0 + s) * ka->Fi * D + (lc - s * D) : 0);
#pragma unroll
    for (int ks = 0; ks < EU_KS; ++ks) {
        const int f = 4 * ks + kk;
        a[ks] = 0.f;
        t[ks] = 0.f;
        if (ks < ka->KS && ok && f < ka->Fi) {
            const float r = rp[f * D], p = rp[ka->half_in + f * D];
            a[ks] = 0.5f * logf(r * r + p * p + EU_LAM_EPS);
            t[ks] = atan2f(p, r);
        }
    }
}

// the 4 consecutive local columns lc0 .. lc0 + 3: off[i] = where (b, d) starts in a half of Z / OP (without the
// neuron's o D), -1 outside the tile or the batch; sd[i] = (local sample) << 8 | d
__device__ __forceinline__ void eu_col_offsets(const EuArgs* ka, int64_t b0, int lc0, int64_t (&off)[4], int (&sd)[4]) {
    const int D = ka->D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int lc = lc0 + i, s = lc / D, d = lc - s * D;
        const bool ok = lc < ka->TC && b0 + s < ka->B;
        off[i] = ok ? (b0 + s) * ka->O * D + d : -1;
        sd[i] = s << 8 | d;
    }
}

__device__ __forceinline__ void eu_load4(const float* src, const int64_t (&off)[4], int64_t oD, bool ok, int vec4,
                                         float (&v)[4]) {
    if (vec4 && ok && off[0] >= 0) {
        const float4 t = *reinterpret_cast<const float4*>(src + off[0] + oD);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (ok && off[i] >= 0) ? src[off[i] + oD] : 0.f;
    }
}

__device__ __forceinline__ void eu_store4(float* dst, const int64_t (&off)[4], int64_t oD, bool ok, int vec4,
                                          const float (&v)[4]) {
    if (vec4 && ok && off[0] >= 0) {
        *reinterpret_cast<float4*>(dst + off[0] + oD) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (ok && off[i] >= 0) dst[off[i] + oD] = v[i];
    }
}

// both products of 16 neurons: accl[ct][i] = sum_f a orders, acct likewise from t, at [n = 4 kk + i, o = r16]
__device__ __forceinline__ void eu_products(const EuArgs* ka, const float* wt, int ot, int r16, int kk,
                                            const float (&a)[EU_CT][EU_KS], const float (&t)[EU_CT][EU_KS],
                                            f32x4 (&accl)[EU_CT], f32x4 (&acct)[EU_CT]) {
#pragma unroll
    for (int ct = 0; ct < EU_CT; ++ct) accl[ct] = acct[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wp = wt + (16 * ot + r16) * EU_WS + kk;
#pragma unroll
    for (int ks = 0; ks < EU_KS; ++ks) {
        if (ks < ka->KS) {
            const float w = wp[4 * ks];
#pragma unroll
            for (int ct = 0; ct < EU_CT; ++ct) {
                accl[ct] = eu_mfma(a[ct][ks], w, accl[ct]);
                acct[ct] = eu_mfma(t[ct][ks], w, acct[ct]);
            }
        }
    }
}

// ---- forward ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EU_NT) void k_eu_fwd(EuArgs args) {
    const EuArgs* ka = (const EuArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float wt[64 * EU_WS];
    __shared__ float stage[2 * EU_COLS * EU_SS];
    __shared__ float gstat[2 * EU_MAX_S * 16 * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int D = ka->D, O = ka->O, S = ka->S;
    const int64_t B = ka->B;
    eu_stage_orders(ka, wt);
    __syncthreads();
    const int64_t tiles = (B + S - 1) / S;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * S;
        float a[EU_CT][EU_KS], t[EU_CT][EU_KS];
        int64_t off[EU_CT][4];
        int sd[EU_CT][4];
#pragma unroll
        for (int ct = 0; ct < EU_CT; ++ct) {
            eu_at_regs(ka, b0, 32 * wave + 16 * ct + r16, kk, a[ct], t[ct]);
            eu_col_offsets(ka, b0, 32 * wave + 16 * ct + 4 * kk, off[ct], sd[ct]);
        }
        for (int ot = 0; ot < ka->OT; ++ot) {
            f32x4 accl[EU_CT], acct[EU_CT];
            eu_products(ka, wt, ot, r16, kk, a, t, accl, acct);
            const int o = 16 * ot + r16;
            const bool ook = o < O;
            const int64_t oD = (int64_t)o * D;
            float v[2][EU_CT][4];
#pragma unroll
            for (int ct = 0; ct < EU_CT; ++ct) {
                float zr[4], zp[4];
                eu_load4(ka->Z, off[ct], oD, ook, ka->vec4, zr);
                eu_load4(ka->Z + ka->half_out, off[ct], oD, ook, ka->vec4, zp);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = ook && off[ct][i] >= 0;
                    const int d = sd[ct][i] & 255;
                    const float ul = accl[ct][i] + (ok ? ka->blam[d * O + o] : 0.f);
                    const float ut = acct[ct][i] + (ok ? ka->bth[d * O + o] : 0.f);
                    const float e = expf(ul);
                    v[0][ct][i] = fmaxf(zr[i], 0.f) + e * cosf(ut);
                    v[1][ct][i] = fmaxf(zp[i], 0.f) + e * sinf(ut);
                }
            }
            if (ka->ln) {
#pragma unroll
                for (int ct = 0; ct < EU_CT; ++ct) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int lc = 32 * wave + 16 * ct + 4 * kk + i;
                        stage[lc * EU_SS + r16] = v[0][ct][i];
                        stage[(EU_COLS + lc) * EU_SS + r16] = v[1][ct][i];
                    }
                }
                __syncthreads();
                // one thread per (half, sample, neuron) group: mean, then centred squares
                for (int item = threadIdx.x; item < 2 * S * 16; item += EU_NT) {
                    const int o16 = item & 15, s = (item >> 4) % S, q = (item >> 4) / S;
                    if (b0 + s < B && 16 * ot + o16 < O) {
                        const float* sp = stage + (q * EU_COLS + s * D) * EU_SS + o16;
                        float m = 0.f, c2 = 0.f;
                        for (int d = 0; d < D; ++d) m += sp[d * EU_SS];
                        m /= (float)D;
                        for (int d = 0; d < D; ++d) {
                            const float c = sp[d * EU_SS] - m;
                            c2 += c * c;
                        }
                        const float rstd = 1.f / sqrtf(c2 / (float)D + ka->eps);
                        gstat[2 * item] = m;
                        gstat[2 * item + 1] = rstd;
                        if (ka->stats) {
                            const int64_t g = ((int64_t)q * B + b0 + s) * O + 16 * ot + o16;
                            ka->stats[g] = m;
                            ka->stats[2 * B * O + g] = rstd;
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int ct = 0; ct < EU_CT; ++ct) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (ook && off[ct][i] >= 0) {
                            const int s = sd[ct][i] >> 8, d = sd[ct][i] & 255;
                            const float* g0 = gstat + 2 * ((0 * S + s) * 16 + r16);
                            const float* g1 = gstat + 2 * ((1 * S + s) * 16 + r16);
                            v[0][ct][i] = (v[0][ct][i] - g0[0]) * g0[1] * ka->wr[d] + ka->br[d];
                            v[1][ct][i] = (v[1][ct][i] - g1[0]) * g1[1] * ka->wp[d] + ka->bp[d];
                        }
                    }
                }
            }
#pragma unroll
            for (int ct = 0; ct < EU_CT; ++ct) {
                eu_store4(ka->OP, off[ct], oD, ook, ka->vec4, v[0][ct]);
                eu_store4(ka->OP + ka->half_out, off[ct], oD, ook, ka->vec4, v[1][ct]);
            }
        }
    }
}

// ---- backward: everything but d orders -------------------------------------------------------------------------
__global__ __launch_bounds__(EU_NT) void k_eu_bwd(EuArgs args) {
    const EuArgs* ka = (const EuArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float wt[64 * EU_WS];
    __shared__ float stage[4 * EU_COLS * EU_SS];     // dy_r | dy_p | yhat_r | yhat_p, then dul | dut in the first two
    __shared__ float gstat[2 * EU_MAX_S * 16 * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int D = ka->D, O = ka->O, S = ka->S, Fi = ka->Fi, FP = ka->FP, OS = ka->OS;
    const int64_t B = ka->B, N = ka->N;
    const float inv_d = 1.f / (float)D;
    eu_stage_orders(ka, wt);
    // the workgroup's partial rows start at 0; a slot is only ever touched by the thread that clears it here
    float* bpart = ka->bpart + (int64_t)blockIdx.x * 2 * D * O;
    float* lnpart = ka->lnpart + (int64_t)blockIdx.x * 16 * 4 * D;
    for (int item = threadIdx.x; item < 2 * D * 16; item += EU_NT) {
        const int o16 = item & 15, rest = item >> 4;
        for (int ot = 0; ot < ka->OT; ++ot)
            if (16 * ot + o16 < O) bpart[rest * O + 16 * ot + o16] = 0.f;
        if (ka->ln) {
            const int d = rest % D, q = rest / D;
            lnpart[o16 * 4 * D + (2 * q) * D + d] = 0.f;
            lnpart[o16 * 4 * D + (2 * q + 1) * D + d] = 0.f;
        }
    }
    __syncthreads();
    const int64_t tiles = (B + S - 1) / S;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * S, n0 = b0 * D;
        float a[EU_CT][EU_KS], t[EU_CT][EU_KS];
        int64_t off[EU_CT][4];
        int sd[EU_CT][4];
        f32x4 dacc[2][4][EU_CT];
#pragma unroll
        for (int ct = 0; ct < EU_CT; ++ct) {
            const int lc = 32 * wave + 16 * ct + r16;
            eu_at_regs(ka, b0, lc, kk, a[ct], t[ct]);
            eu_col_offsets(ka, b0, 32 * wave + 16 * ct + 4 * kk, off[ct], sd[ct]);
            if (lc < ka->TC && n0 + lc < N) {
#pragma unroll
                for (int ks = 0; ks < EU_KS; ++ks) {
                    if (ks < ka->KS) {
                        ka->at[(n0 + lc) * FP + 4 * ks + kk] = a[ct][ks];
                        ka->at[(N + n0 + lc) * FP + 4 * ks + kk] = t[ct][ks];
                    }
                }
            }
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) dacc[0][ft][ct] = dacc[1][ft][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int ot = 0; ot < ka->OT; ++ot) {
            f32x4 accl[EU_CT], acct[EU_CT];
            eu_products(ka, wt, ot, r16, kk, a, t, accl, acct);
            const int o = 16 * ot + r16;
            const bool ook = o < O;
            const int64_t oD = (int64_t)o * D;
            // per element: ec = e cos, es = e sin, the ReLU masks, dy -> d(pre-norm), yhat and rstd with the norm on
            float ec[EU_CT][4], es[EU_CT][4], gr[EU_CT][4], gp[EU_CT][4], yr[EU_CT][4], yp[EU_CT][4];
            float rsr[EU_CT][4], rsp[EU_CT][4];
            unsigned mask = 0;
#pragma unroll
            for (int ct = 0; ct < EU_CT; ++ct) {
                float zr[4], zp[4];
                eu_load4(ka->Z, off[ct], oD, ook, ka->vec4, zr);
                eu_load4(ka->Z + ka->half_out, off[ct], oD, ook, ka->vec4, zp);
                eu_load4(ka->dOP, off[ct], oD, ook, ka->vec4, gr[ct]);
                eu_load4(ka->dOP + ka->half_out, off[ct], oD, ook, ka->vec4, gp[ct]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = ook && off[ct][i] >= 0;
                    const int s = sd[ct][i] >> 8, d = sd[ct][i] & 255;
                    const float ul = accl[ct][i] + (ok ? ka->blam[d * O + o] : 0.f);
                    const float ut = acct[ct][i] + (ok ? ka->bth[d * O + o] : 0.f);
                    const float e = expf(ul);
                    ec[ct][i] = e * cosf(ut);
                    es[ct][i] = e * sinf(ut);
                    if (zr[i] > 0.f) mask |= 1u << (8 * ct + i);
                    if (zp[i] > 0.f) mask |= 1u << (8 * ct + 4 + i);
                    if (ka->ln) {
                        float mr = 0.f, mp = 0.f;
                        rsr[ct][i] = rsp[ct][i] = 0.f;
                        if (ok) {
                            const int64_t g = (b0 + s) * O + o;
                            mr = ka->stats[g];
                            mp = ka->stats[B * O + g];
                            rsr[ct][i] = ka->stats[2 * B * O + g];
                            rsp[ct][i] = ka->stats[3 * B * O + g];
                        }
                        yr[ct][i] = (fmaxf(zr[i], 0.f) + ec[ct][i] - mr) * rsr[ct][i];
                        yp[ct][i] = (fmaxf(zp[i], 0.f) + es[ct][i] - mp) * rsp[ct][i];
                        const int lc = 32 * wave + 16 * ct + 4 * kk + i;
                        stage[(0 * EU_COLS + lc) * EU_SS + r16] = gr[ct][i];
                        stage[(1 * EU_COLS + lc) * EU_SS + r16] = gp[ct][i];
                        stage[(2 * EU_COLS + lc) * EU_SS + r16] = yr[ct][i];
                        stage[(3 * EU_COLS + lc) * EU_SS + r16] = yp[ct][i];
                    }
                }
            }
            if (ka->ln) {
                __syncthreads();
                // the group's two sums: sum_d w dy | sum_d w dy yhat
                for (int item = threadIdx.x; item < 2 * S * 16; item += EU_NT) {
                    const int o16 = item & 15, s = (item >> 4) % S, q = (item >> 4) / S;
                    if (b0 + s < B && 16 * ot + o16 < O) {
                        const float* dy = stage + (q * EU_COLS + s * D) * EU_SS + o16;
                        const float* yh = dy + 2 * EU_COLS * EU_SS;
                        const float* w = q ? ka->wp : ka->wr;
                        float s1 = 0.f, s2 = 0.f;
                        for (int d = 0; d < D; ++d) {
                            const float g = w[d] * dy[d * EU_SS];
                            s1 += g;
                            s2 += g * yh[d * EU_SS];
                        }
                        gstat[2 * item] = s1 * inv_d;
                        gstat[2 * item + 1] = s2 * inv_d;
                    }
                }
                // d norm.weight[d] += sum dy yhat, d norm.bias[d] += sum dy over the tile's samples, per neuron slot
                for (int item = threadIdx.x; item < 2 * D * 16; item += EU_NT) {
                    const int o16 = item & 15, d = (item >> 4) % D, q = (item >> 4) / D;
                    if (16 * ot + o16 < O) {
                        const float* dy = stage + (q * EU_COLS + d) * EU_SS + o16;
                        const float* yh = dy + 2 * EU_COLS * EU_SS;
                        float s1 = 0.f, s2 = 0.f;
                        for (int s = 0; s < S && b0 + s < B; ++s) {
                            s1 += dy[s * D * EU_SS] * yh[s * D * EU_SS];
                            s2 += dy[s * D * EU_SS];
                        }
                        lnpart[o16 * 4 * D + (2 * q) * D + d] += s1;
                        lnpart[o16 * 4 * D + (2 * q + 1) * D + d] += s2;
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int ct = 0; ct < EU_CT; ++ct) {
                float dzr[4], dzp[4], dul[4], dut[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = ook && off[ct][i] >= 0;
                    float dr = gr[ct][i], dp = gp[ct][i];
                    if (ka->ln) {
                        const int s = sd[ct][i] >> 8, d = sd[ct][i] & 255;
                        const float* g0 = gstat + 2 * ((0 * S + s) * 16 + r16);
                        const float* g1 = gstat + 2 * ((1 * S + s) * 16 + r16);
                        dr = ok ? rsr[ct][i] * (ka->wr[d] * dr - g0[0] - yr[ct][i] * g0[1]) : 0.f;
                        dp = ok ? rsp[ct][i] * (ka->wp[d] * dp - g1[0] - yp[ct][i] * g1[1]) : 0.f;
                    }
                    dzr[i] = (mask >> (8 * ct + i) & 1u) ? dr : 0.f;
                    dzp[i] = (mask >> (8 * ct + 4 + i) & 1u) ? dp : 0.f;
                    dul[i] = ok ? dr * ec[ct][i] + dp * es[ct][i] : 0.f;
                    dut[i] = ok ? dp * ec[ct][i] - dr * es[ct][i] : 0.f;
                    const int lc = 32 * wave + 16 * ct + 4 * kk + i;
                    stage[lc * EU_SS + r16] = dul[i];
                    stage[(EU_COLS + lc) * EU_SS + r16] = dut[i];
                    if (ok) {
                        ka->du[(n0 + lc) * OS + o] = dul[i];
                        ka->du[(N + n0 + lc) * OS + o] = dut[i];
                    }
                }
                eu_store4(ka->dZ, off[ct], oD, ook, ka->vec4, dzr);
                eu_store4(ka->dZ + ka->half_out, off[ct], oD, ook, ka->vec4, dzp);
            }
            __syncthreads();
            // d bias_lam[d, o] | d bias_theta[d, o] += the tile's samples
            for (int item = threadIdx.x; item < 2 * D * 16; item += EU_NT) {
                const int o16 = item & 15, d = (item >> 4) % D, q = (item >> 4) / D;
                if (16 * ot + o16 < O) {
                    const float* src = stage + (q * EU_COLS + d) * EU_SS + o16;
                    float s1 = 0.f;
                    for (int s = 0; s < S && b0 + s < B; ++s) s1 += src[s * D * EU_SS];
                    bpart[(q * D + d) * O + 16 * ot + o16] += s1;
                }
            }
            // da[f, n] += orders[f, o] dul[o, n], dt likewise: K = the 16 neurons, the staged tile is the B operand
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                float bl[EU_CT], bt[EU_CT];
#pragma unroll
                for (int ct = 0; ct < EU_CT; ++ct) {
                    const int lc = 32 * wave + 16 * ct + r16;
                    bl[ct] = stage[lc * EU_SS + 4 * ks + kk];
                    bt[ct] = stage[(EU_COLS + lc) * EU_SS + 4 * ks + kk];
                }
                const float* wq = wt + (16 * ot + 4 * ks + kk) * EU_WS + r16;
#pragma unroll
                for (int ft = 0; ft < 4; ++ft) {
                    if (ft < ka->FT) {
                        const float w = wq[16 * ft];
#pragma unroll
                        for (int ct = 0; ct < EU_CT; ++ct) {
                            dacc[0][ft][ct] = eu_mfma(w, bl[ct], dacc[0][ft][ct]);
                            dacc[1][ft][ct] = eu_mfma(w, bt[ct], dacc[1][ft][ct]);
                        }
                    }
                }
            }
            __syncthreads();                     // the stage is free for the next 16 neurons
        }
        // dacc[.][ft][ct][i] = da | dt [f = 16 ft + 4 kk + i, n = column r16 of tile ct]: the explicit part of dRP
#pragma unroll
        for (int ct = 0; ct < EU_CT; ++ct) {
            const int lc = 32 * wave + 16 * ct + r16, s = lc / D;
            if (lc < ka->TC && b0 + s < B) {
                const int64_t base = (b0 + s) * Fi * D + (lc - s * D);
#pragma unroll
                for (int ft = 0; ft < 4; ++ft) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int f = 16 * ft + 4 * kk + i;
                        if (f < Fi) {
                            const float r = ka->RP[base + f * D], p = ka->RP[ka->half_in + base + f * D];
                            const float m2 = r * r + p * p, da = dacc[0][ft][ct][i] / (m2 + EU_LAM_EPS);
                            const float dt = m2 > 0.f ? dacc[1][ft][ct][i] / m2 : 0.f;    // 0 / 0 -> 0, as torch masks it
                            ka->dRP[base + f * D] = da * r - dt * p;
                            ka->dRP[ka->half_in + base + f * D] = da * p + dt * r;
                        }
                    }
                }
            }
        }
    }
}

// ---- d orders[f, o] = sum_n a[n, f] dul[n, o] + t[n, f] dut[n, o]: one slab of columns per workgroup -----------------
__global__ __launch_bounds__(EU_NT) void k_eu_bwd_dw(EuArgs args) {
    const EuArgs* ka = (const EuArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float at[2][64 * EU_WS];          // a | t of 64 columns: [n, f]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int O = ka->O, Fi = ka->Fi, FP = ka->FP, OS = ka->OS;
    const int64_t N = ka->N;
    const int o = 16 * wave + r16;
    f32x4 dacc[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) dacc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t tiles = (N + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * 64;
        __syncthreads();
        for (int idx = threadIdx.x; idx < 2 * 64 * 64; idx += EU_NT) {
            const int q = idx >> 12, r = (idx >> 6) & 63, f = idx & 63;
            at[q][r * EU_WS + f] = (n0 + r < N && f < FP) ? ka->at[(q * N + n0 + r) * FP + f] : 0.f;
        }
        __syncthreads();
        if (16 * wave < O) {
            for (int j = 0; j < 4 && n0 + 16 * j < N; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t n = n0 + 16 * j + 4 * kk + i;
                    const bool ok = n < N && o < O;
                    const float dl = ok ? ka->du[n * OS + o] : 0.f, dt = ok ? ka->du[(N + n) * OS + o] : 0.f;
                    const int row = (16 * j + 4 * kk + i) * EU_WS + r16;
#pragma unroll
                    for (int ft = 0; ft < 4; ++ft) {
                        if (ft < ka->FT) {
                            dacc[ft] = eu_mfma(at[0][row + 16 * ft], dl, dacc[ft]);
                            dacc[ft] = eu_mfma(at[1][row + 16 * ft], dt, dacc[ft]);
                        }
                    }
                }
            }
        }
    }
    // dacc[ft][i] = d orders[f = 16 ft + 4 kk + i, o] of this slab
    if (o < O) {
        float* dst = ka->dwpart + (int64_t)blockIdx.x * Fi * O;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = 16 * ft + 4 * kk + i;
                if (f < Fi) dst[f * O + o] = dacc[ft][i];
            }
        }
    }
}

// ---- the polar front end: RP = mu (cos E | sin E) -------------------------------------------------------------------
__global__ __launch_bounds__(EU_NT) void k_eu_polar_fwd(const float* E, int64_t x_ld, const float* mu, int64_t B, int F,
                                                        int D, float* RP) {
    const int FD = F * D;
    const int64_t total = B * FD;
    for (int64_t idx = (int64_t)blockIdx.x * EU_NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * EU_NT) {
        const int64_t b = idx / FD;
        const int r = (int)(idx - b * FD);
        const float e = E[b * x_ld + r], m = mu[r / D];
        RP[idx] = m * cosf(e);
        RP[total + idx] = m * sinf(e);
    }
}

// dE = mu (-sin E dr + cos E dp); part[chunk, f] = the chunk's share of dmu[f] = sum_{b, d} cos E dr + sin E dp
__global__ __launch_bounds__(EU_NT) void k_eu_polar_bwd(const float* E, int64_t x_ld, const float* mu, int64_t B, int F,
                                                        int D, const float* dRP, float* dE, int64_t de_ld,
                                                        int64_t per, float* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t lo = (int64_t)blockIdx.x * per * D, hi = (lo + per * D < B * D) ? lo + per * D : B * D;
    const int64_t half = B * F * D;
    for (int f = wave; f < F; f += 4) {
        const float m = mu[f];
        float s = 0.f;
        for (int64_t n = lo + lane; n < hi; n += 64) {
            const int64_t b = n / D;
            const int d = (int)(n - b * D);
            const float e = E[b * x_ld + f * D + d], c = cosf(e), sn = sinf(e);
            const float dr = dRP[(b * F + f) * D + d], dp = dRP[half + (b * F + f) * D + d];
            dE[b * de_ld + f * D + d] = m * (dp * c - dr * sn);
            s += c * dr + sn * dp;
        }
        s = fx_wave_sum(s);
        if (lane == 0) part[(int64_t)blockIdx.x * F + f] = s;
    }
}

// ---- hosts ------------------------------------------------------------------------------------------------------
static int64_t eu_up4(int64_t n) { return (n + 3) / 4 * 4; }

static int eu_tile_samples(int D) {
    const int s = EU_COLS / D;
    return s < 1 ? 1 : s > EU_MAX_S ? EU_MAX_S : s;
}

static int64_t eu_workgroups(int64_t B, int D) {
    const int64_t tiles = fx_ceil_div(B > 0 ? B : 1, eu_tile_samples(D));
    return tiles < EU_MAX_WG ? tiles : EU_MAX_WG;
}

static int eu_slabs(int64_t N) {
    const int64_t tiles = fx_ceil_div(N > 0 ? N : 1, 64);
    return (int)(tiles < EU_MAX_SLABS ? tiles : EU_MAX_SLABS);
}

static int64_t eu_polar_per(int64_t B) { return fx_ceil_div(B > 0 ? B : 1, EU_CHUNKS); }

static bool eu_shape_ok(int64_t B, int32_t Fi, int32_t D, int32_t O) {
    return B >= 0 && Fi >= 1 && Fi <= EU_MAX_F && D >= 1 && D <= EU_MAX_D && O >= 1 && O <= EU_MAX_O;
}

static int eu_fill(const char* who, EuArgs& p, const float* RP, const float* Z, int64_t B, int32_t Fi, int32_t D,
                   int32_t O, const float* orders, const float* blam, const float* bth, int32_t layer_norm,
                   const float* wr, const float* br, const float* wp, const float* bp, float eps) {
    FX_CHECK_ARG(Fi >= 1 && Fi <= EU_MAX_F, "%s: Fi=%d, limit 1 <= Fi <= %d", who, Fi, EU_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= EU_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, EU_MAX_D);
    FX_CHECK_ARG(O >= 1 && O <= EU_MAX_O, "%s: O=%d, limit 1 <= O <= %d", who, O, EU_MAX_O);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    memset(&p, 0, sizeof(p));
    p.RP = RP; p.Z = Z; p.B = B; p.N = B * D; p.half_in = B * Fi * D; p.half_out = B * O * D;
    p.Fi = Fi; p.D = D; p.O = O; p.KS = (Fi + 3) / 4; p.FP = 4 * p.KS; p.FT = (Fi + 15) / 16; p.OT = (O + 15) / 16;
    p.OS = (int)eu_up4(O); p.S = eu_tile_samples(D); p.TC = p.S * D; p.ln = layer_norm ? 1 : 0;
    p.orders = orders; p.blam = blam; p.bth = bth; p.wr = wr; p.br = br; p.wp = wp; p.bp = bp; p.eps = eps;
    return FX_OK;
}

extern "C" void fx_euler_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = EU_MAX_F;
    limits[1] = EU_MAX_D;
    limits[2] = EU_MAX_O;
    limits[3] = EU_COLS;
    limits[4] = EU_MAX_S;
    limits[5] = EU_MAX_WG;
    limits[6] = EU_MAX_SLABS;
    limits[7] = EU_CHUNKS;
}

extern "C" int64_t fx_euler_workspace_floats(int64_t B, int32_t Fi, int32_t D, int32_t O) {
    if (!eu_shape_ok(B, Fi, D, O)) return 0;
    const int64_t N = B * D, wg = eu_workgroups(B, D), FP = (Fi + 3) / 4 * 4;
    const int64_t bwd = 2 * N * FP + 2 * N * eu_up4(O) + eu_up4(wg * 2 * D * O) + wg * 16 * 4 * D +
                        (int64_t)eu_slabs(N) * Fi * O;
    const int64_t polar = (int64_t)EU_CHUNKS * Fi;
    return bwd > polar ? bwd : polar;
}

extern "C" int fx_euler_polar_fwd(const float* E, int64_t x_ld, const float* mu, int64_t B, int32_t F, int32_t D,
                                  float* RP, fx_stream_t stream) {
    const char* who = "fx_euler_polar_fwd";
    FX_CHECK_ARG(F >= 1 && F <= EU_MAX_F, "%s: F=%d, limit 1 <= F <= %d", who, F, EU_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= EU_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, EU_MAX_D);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: E sample stride %lld < F*D", who, (long long)x_ld);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(E && mu && RP, "%s: null E / mu / RP", who);
    const int64_t blocks = fx_ceil_div(B * F * D, EU_NT);
    hipLaunchKernelGGL(k_eu_polar_fwd, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(EU_NT), 0,
                       fx_hip_stream(stream), E, x_ld, mu, B, F, D, RP);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_euler_polar_bwd(const float* E, int64_t x_ld, const float* mu, int64_t B, int32_t F, int32_t D,
                                  const float* dRP, float* dE, int64_t de_ld, float* dmu, float* workspace,
                                  fx_stream_t stream) {
    const char* who = "fx_euler_polar_bwd";
    FX_CHECK_ARG(F >= 1 && F <= EU_MAX_F, "%s: F=%d, limit 1 <= F <= %d", who, F, EU_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= EU_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, EU_MAX_D);
    FX_CHECK_ARG(B >= 1, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D && de_ld >= (int64_t)F * D, "%s: E / dE sample stride %lld / %lld < F*D", who,
                 (long long)x_ld, (long long)de_ld);
    FX_CHECK_ARG(E && mu && dRP && dE && dmu && workspace, "%s: null E / mu / dRP / dE / dmu / workspace", who);
    hipStream_t s = fx_hip_stream(stream);
    const int64_t per = eu_polar_per(B);
    const int chunks = (int)fx_ceil_div(B, per);
    hipLaunchKernelGGL(k_eu_polar_bwd, dim3((unsigned)chunks), dim3(EU_NT), 0, s, E, x_ld, mu, B, F, D, dRP, dE, de_ld,
                       per, workspace);
    FX_CHECK_LAUNCH();
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, chunks, F, fx_rowsum_out(dmu, F));
}

extern "C" int fx_euler_fwd(const float* RP, const float* Z, int64_t B, int32_t Fi, int32_t D, int32_t O,
                            const float* inter_orders, const float* bias_lam, const float* bias_theta,
                            int32_t layer_norm, const float* norm_r_weight, const float* norm_r_bias,
                            const float* norm_p_weight, const float* norm_p_bias, float eps, float* stats, float* OP,
                            fx_stream_t stream) {
    const char* who = "fx_euler_fwd";
    EuArgs p;
    if (int st = eu_fill(who, p, RP, Z, B, Fi, D, O, inter_orders, bias_lam, bias_theta, layer_norm, norm_r_weight,
                         norm_r_bias, norm_p_weight, norm_p_bias, eps))
        return st;
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(RP && Z && inter_orders && bias_lam && bias_theta && OP, "%s: null RP / Z / inter_orders / bias / OP",
                 who);
    FX_CHECK_ARG(!layer_norm || (norm_r_weight && norm_r_bias && norm_p_weight && norm_p_bias),
                 "%s: null LayerNorm weight / bias with layer_norm on", who);
    p.OP = OP; p.stats = layer_norm ? stats : nullptr;
    p.vec4 = D % 4 == 0 && fx_al16(Z) && fx_al16(OP);
    hipLaunchKernelGGL(k_eu_fwd, dim3((unsigned)eu_workgroups(B, D)), dim3(EU_NT), 0, fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_euler_bwd(const float* RP, const float* Z, int64_t B, int32_t Fi, int32_t D, int32_t O,
                            const float* inter_orders, const float* bias_lam, const float* bias_theta,
                            int32_t layer_norm, const float* norm_r_weight, const float* norm_p_weight, float eps,
                            const float* stats, const float* dOP, float* dZ, float* dRP, float* d_inter_orders,
                            float* d_bias, float* d_norm, float* workspace, fx_stream_t stream) {
    const char* who = "fx_euler_bwd";
    EuArgs p;
    if (int st = eu_fill(who, p, RP, Z, B, Fi, D, O, inter_orders, bias_lam, bias_theta, layer_norm, norm_r_weight,
                         nullptr, norm_p_weight, nullptr, eps))
        return st;
    FX_CHECK_ARG(B >= 1, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(RP && Z && inter_orders && bias_lam && bias_theta && dOP && dZ && dRP && d_inter_orders && d_bias &&
                 workspace, "%s: null RP / Z / inter_orders / bias / dOP / dZ / dRP / gradient / workspace", who);
    FX_CHECK_ARG(!layer_norm || (norm_r_weight && norm_p_weight && stats && d_norm),
                 "%s: null LayerNorm weight / stats / d_norm with layer_norm on", who);
    hipStream_t s = fx_hip_stream(stream);
    const int64_t wg = eu_workgroups(B, D);
    const int slabs = eu_slabs(p.N);
    p.at = workspace;
    p.du = p.at + 2 * p.N * p.FP;
    p.bpart = p.du + 2 * p.N * p.OS;
    p.lnpart = p.bpart + eu_up4(wg * 2 * D * O);
    p.dwpart = p.lnpart + wg * 16 * 4 * D;
    p.stats = const_cast<float*>(stats);
    p.dOP = dOP; p.dZ = dZ; p.dRP = dRP;
    p.vec4 = D % 4 == 0 && fx_al16(Z) && fx_al16(dOP) && fx_al16(dZ);
    hipLaunchKernelGGL(k_eu_bwd, dim3((unsigned)wg), dim3(EU_NT), 0, s, p);
    FX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eu_bwd_dw, dim3((unsigned)slabs), dim3(EU_NT), 0, s, p);
    FX_CHECK_LAUNCH();
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, p.dwpart, slabs, (int64_t)Fi * O,
                                                   fx_rowsum_out(d_inter_orders, (int64_t)Fi * O)))
        return st;
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, p.bpart, (int)wg, 2 * (int64_t)D * O,
                                                   fx_rowsum_out(d_bias, 2 * (int64_t)D * O)))
        return st;
    if (layer_norm)
        return fx_rowsum<double, FX_ROWS_SLICES>(s, p.lnpart, (int)wg * 16, 4 * (int64_t)D, fx_rowsum_out(d_norm, 4 * D));
    return FX_OK;
}
