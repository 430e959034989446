// fx_lognet.hip — AFN's logarithmic transformation layer on the matrix cores.
// Reference: model_zoo/AFN/src/AFN.py:121-138 (logarithmic_net).  From E [B, F, D] and W [L, F]:
//     a = log(max(|x|, 1e-5)),  ahat = BN_log(a)  (training-mode BatchNorm1d(F): statistics over the B D elements of a
//     field),  u[b, l, d] = sum_f W[l, f] ahat[b, f, d],  c = exp(u),  Y[b, l D + d] = BN_exp(c)  (BatchNorm1d(L)).
// x is tiny (B F D floats) and c is huge (B L D floats), so c never reaches memory: the forward writes Y alone, the
// backward reads dY alone, and c is recomputed from x (K = F MFMAs and one exp per element against 8 bytes of HBM
// traffic) wherever it is needed.
//
// The N axis of the product is the flattened column n = b D + d (N = B D columns), so no tile is padded to D and a
// column's neurons l land D floats apart in Y: 16 consecutive columns are 64 consecutive bytes.  All products run
// on v_mfma_f32_16x16x4_f32 with the operand layout of fx_crossmix.hip: lane (r16 = lane & 15, kk = lane >> 4) holds
// element (r16, k = kk) of A and of B and rows 4 kk + i of column r16 of the result.  Both operands have the same
// lane layout, so swapping them transposes the result, and a result chains into the next product as its B operand
// with no LDS round trip when the summation index is walked in the order k-slot kk <-> row 4 kk + i (step i).
//   column kernels (k_ln_cols: the exp statistics, the output, the BN_exp backward sums; k_ln_bwd_da): a workgroup
//     owns LN_COLS = 128 columns (a wave 2 x 16) and strides over the tiles.  A lane computes its 16-column slice of
//     ahat ONCE from x into registers (ahat[n = r16, f = 4 ks + kk], 16 registers per column tile: every log is taken
//     once per pass) and loops over L in chunks of 64 rows of W staged in LDS (row stride 68 = 4 mod 64: both reads
//     below hit 64 different banks).  ahat x W^T gives u[n = 4 kk + i, l = r16]: 4 consecutive columns per lane,
//     16-byte accesses to Y / dY when D % 4 == 0, a wave covering 16 neurons x 16 columns.
//   k_ln_bwd_da takes W x ahat^T instead (u[l = 4 kk + i, n = r16]) so that du = dc c is the B operand of
//     dahat[f, n] += W[l, f]^T du[l, n]: K = L, the 4 x 2 accumulator tiles persist over the L loop.
//   k_ln_bwd_dw is per (64 neurons, slab of columns): W in registers, ahat tiles [64 columns, F] streamed through LDS
//     from the workspace copy that k_ln_bwd_da left; du^T[n = 4 kk + i, l = r16] chains into dW^T[f, l] += ahat[n, f]^T
//     du^T[n, l]: K = the slab's columns, a [F, 16] accumulator per wave; [slabs, L, F] partials meet in fx_rowsum.
// Statistics: BN_log merges per-chunk (mean, centred squares) pairs by Chan's formula in fp64: freshly initialised
// tables have a = -9.5 +- 1, where plain sums of a and a^2 lose the variance.  BN_exp sums c - p_l and (c - p_l)^2 about the
// pivot p_l = exp(sum_f W[l, f] beta1[f]), the value of c at E[ahat] (a small W makes c = 1 +- eps).  Every reduce
// has a fixed order and there are no atomics: two runs give the same bits, and launch counts depend on shapes only.
#include "fx_common.h"
#include "fx_rowsum.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define LN_MAX_F 64
#define LN_MAX_D 64
#define LN_MAX_L 2048
#define LN_NT 256
#define LN_CT 2                 // 16-column tiles per wave
#define LN_COLS (64 * LN_CT)    // columns per workgroup tile
#define LN_LC 64                // rows of W in LDS at a time
#define LN_WS 68                // LDS row stride of a [64, 64] operand tile: = 4 mod 64
#define LN_KS (LN_MAX_F / 4)    // k steps of the F-long product
#define LN_MAX_WG 1024          // workgroups of a column kernel: the rows of its partial sums
#define LN_CHUNKS 256           // chunks of the per-field statistics
#define LN_MAX_SLABS 256        // column slabs of the weight-gradient kernel
#define LN_CLAMP 1e-5f

struct LnArgs {
    const float* X; int64_t x_ld;
    int64_t B, N, NP;                       // N = B D columns; NP: row stride of dahat [F, NP]
    int F, D, L, KS, FP, FT;                // KS = ceil(F / 4), FP = 4 KS, FT = ceil(F / 16)
    const float* W;
    const float *g1, *b1, *g2, *b2;
    const float *mean1, *var1, *mean2, *var2;
    float eps;
    const float* pivot;
    float* part;                            // [workgroups, 2, L]
    float* Y; const float* dY; int vec4;
    const float *sdy, *sdyc;                // sum dY, sum dY chat per neuron (= dbeta2, dgamma2)
    float* ahat;                            // [N, FP]
    float* dahat;                           // [F, NP]
    float* dwpart;                          // [slabs, L, F]
};

__device__ __forceinline__ f32x4 ln_mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float ln_log(float x) { return logf(fmaxf(fabsf(x), LN_CLAMP)); }

// bn1[0 | 1 | 2][f] = mean1 | gamma1 rstd1 | beta1 of field f (zeros past F)
__device__ __forceinline__ void ln_stage_bn1(const LnArgs* ka, float (*bn1)[64]) {
    if (threadIdx.x < 64) {
        const int f = threadIdx.x;
        const bool ok = f < ka->F;
        bn1[0][f] = ok ? ka->mean1[f] : 0.f;
        bn1[1][f] = ok ? ka->g1[f] * (1.f / sqrtf(ka->var1[f] + ka->eps)) : 0.f;
        bn1[2][f] = ok ? ka->b1[f] : 0.f;
    }
}

// the lane's slice of ahat for column n: a[ks] = ahat[n, f = 4 ks + kk]; zeros past F and past N
__device__ __forceinline__ void ln_ahat_regs(const LnArgs* ka, const float (*bn1)[64], int64_t n, int kk,
                                             float (&a)[LN_KS]) {
    const bool ok = n < ka->N;
    const int64_t b = ok ? n / ka->D : 0;
    const float* xp = ka->X + b * ka->x_ld + (ok ? n - b * ka->D : 0);
#pragma unroll
    for (int ks = 0; ks < LN_KS; ++ks) {
        const int f = 4 * ks + kk;
        a[ks] = 0.f;
        if (ks < ka->KS && ok && f < ka->F) a[ks] = (ln_log(xp[f * ka->D]) - bn1[0][f]) * bn1[1][f] + bn1[2][f];
    }
}

// rows lb .. lb + 63 of W into wl [64, LN_WS] (zeros past L and past F), and the per-neuron constants of the chunk:
// lc[0..4][li] = mean2 | rstd2 | gamma2 rstd2 | beta2 or (sum dY) / N | pivot or (sum dY chat) / N
__device__ __forceinline__ void ln_stage_chunk(const LnArgs* ka, int lb, float* wl, float (*lc)[64]) {
    const int F = ka->F, L = ka->L;
    for (int idx = threadIdx.x; idx < LN_LC * 64; idx += LN_NT) {
        const int r = idx >> 6, f = idx & 63;
        wl[r * LN_WS + f] = (lb + r < L && f < F) ? ka->W[(int64_t)(lb + r) * F + f] : 0.f;
    }
    if (threadIdx.x < 64) {
        const int li = threadIdx.x, l = lb + li;
        const bool ok = l < L;
        const float inv_n = 1.f / (float)ka->N;
        const float rstd = (ok && ka->var2) ? 1.f / sqrtf(ka->var2[l] + ka->eps) : 0.f;
        lc[0][li] = (ok && ka->mean2) ? ka->mean2[l] : 0.f;
        lc[1][li] = rstd;
        lc[2][li] = (ok && ka->g2) ? ka->g2[l] * rstd : 0.f;
        lc[3][li] = !ok ? 0.f : ka->b2 ? ka->b2[l] : ka->sdy ? ka->sdy[l] * inv_n : 0.f;
        lc[4][li] = !ok ? 0.f : ka->pivot ? ka->pivot[l] : ka->sdyc ? ka->sdyc[l] * inv_n : 0.f;
    }
}

// where the 4 consecutive columns nb .. nb + 3 start in Y / dY (without the neuron's l D): off[i], -1 past N
__device__ __forceinline__ void ln_col_offsets(const LnArgs* ka, int64_t nb, int64_t (&off)[4]) {
    const int D = ka->D;
    const int64_t ldy = (int64_t)ka->L * D;
    const int64_t b = nb < ka->N ? nb / D : 0;
    const int d = nb < ka->N ? (int)(nb - b * D) : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = (d + i) / D;
        off[i] = nb + i < ka->N ? (b + q) * ldy + (d + i - q * D) : -1;
    }
}

// ---- (a) BN_log statistics: per chunk of columns and field the mean and the centred squares -------------------
__global__ __launch_bounds__(LN_NT) void k_ln_log_stats(LnArgs args, int64_t per, float* lpart) {
    const LnArgs* ka = (const LnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = ka->D, F = ka->F;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < ka->N ? lo + per : ka->N;
    for (int f = wave; f < F; f += 4) {
        float s = 0.f;
        for (int64_t n = lo + lane; n < hi; n += 64) {
            const int64_t b = n / D;
            s += ln_log(ka->X[b * ka->x_ld + f * D + (n - b * D)]);
        }
        const float mean = fx_wave_sum(s) / (float)(hi - lo);
        float q = 0.f;
        for (int64_t n = lo + lane; n < hi; n += 64) {
            const int64_t b = n / D;
            const float t = ln_log(ka->X[b * ka->x_ld + f * D + (n - b * D)]) - mean;
            q += t * t;
        }
        q = fx_wave_sum(q);
        if (lane == 0) {
            lpart[((int64_t)blockIdx.x * 2 + 0) * F + f] = mean;
            lpart[((int64_t)blockIdx.x * 2 + 1) * F + f] = q;
        }
    }
}

// BatchNorm1d's running update, momentum m, from the batch mean and BIASED variance over n elements
__device__ __forceinline__ void ln_running(double mean, double var, double n, float m, float* rm, float* rv) {
    *rm = (float)((1.0 - m) * *rm + m * mean);
    *rv = (float)((1.0 - m) * *rv + m * (var * n / (n - 1.0)));
}

// the chunks merged in a fixed order (Chan): mean1 | var1 (biased), the running update; and the pivots of (b)
__global__ __launch_bounds__(LN_NT) void k_ln_log_finish(LnArgs args, const float* lpart, int chunks, int64_t per,
                                                         float momentum, float* mean1, float* var1, float* rm,
                                                         float* rv, int64_t* nbt, float* pivot) {
    const LnArgs* ka = (const LnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int F = ka->F, l = blockIdx.x * LN_NT + threadIdx.x;
    if (l < ka->L) {
        float p = 0.f;
        for (int f = 0; f < F; ++f) p += ka->W[(int64_t)l * F + f] * ka->b1[f];
        pivot[l] = expf(p);
    }
    if (blockIdx.x != 0 || threadIdx.x >= F) return;
    const int f = threadIdx.x;
    const double n = (double)ka->N;
    double mean = 0.0, m2 = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double cnt = (double)((c + 1) * per < ka->N ? per : ka->N - c * per);
        mean += cnt * (double)lpart[((int64_t)c * 2) * F + f];
    }
    mean /= n;
    for (int c = 0; c < chunks; ++c) {
        const double cnt = (double)((c + 1) * per < ka->N ? per : ka->N - c * per);
        const double d = (double)lpart[((int64_t)c * 2) * F + f] - mean;
        m2 += (double)lpart[((int64_t)c * 2 + 1) * F + f] + cnt * d * d;
    }
    mean1[f] = (float)mean;
    var1[f] = (float)(m2 / n);
    ln_running(mean, m2 / n, n, momentum, rm + f, rv + f);
    if (f == 0) *nbt += 1;
}

// ---- (b), (c), (d): the column kernel ---------------------------------------------------------------------
enum { LN_STATS, LN_OUT, LN_BSUMS };

template <int MODE>
__global__ __launch_bounds__(LN_NT) void k_ln_cols(LnArgs args) {
    const LnArgs* ka = (const LnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float wl[LN_LC * LN_WS];
    __shared__ float lc[5][64];
    __shared__ float bn1[3][64];
    __shared__ float red[4][2][64];
    extern __shared__ __attribute__((aligned(16))) float sacc[];       // [2, LP]: the workgroup's sums per neuron
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int L = ka->L, D = ka->D, LP = (L + 63) / 64 * 64;
    const int64_t N = ka->N;
    ln_stage_bn1(ka, bn1);
    if (MODE != LN_OUT)
        for (int i = threadIdx.x; i < 2 * LP; i += LN_NT) sacc[i] = 0.f;
    __syncthreads();
    const int64_t tiles = (N + LN_COLS - 1) / LN_COLS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * LN_COLS + wave * (16 * LN_CT);
        float a[LN_CT][LN_KS];
        int64_t off[LN_CT][4];
#pragma unroll
        for (int ct = 0; ct < LN_CT; ++ct) {
            ln_ahat_regs(ka, bn1, n0 + 16 * ct + r16, kk, a[ct]);
            ln_col_offsets(ka, n0 + 16 * ct + 4 * kk, off[ct]);
        }
        for (int lb = 0; lb < L; lb += LN_LC) {
            __syncthreads();                     // wl, lc and red are free
            ln_stage_chunk(ka, lb, wl, lc);
            __syncthreads();
            for (int lt = 0; lt < LN_LC / 16 && lb + 16 * lt < L; ++lt) {
                f32x4 acc[LN_CT];
#pragma unroll
                for (int ct = 0; ct < LN_CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                const float* wp = wl + (16 * lt + r16) * LN_WS + kk;
#pragma unroll
                for (int ks = 0; ks < LN_KS; ++ks) {
                    if (ks < ka->KS) {
                        const float w = wp[4 * ks];
#pragma unroll
                        for (int ct = 0; ct < LN_CT; ++ct) acc[ct] = ln_mfma(a[ct][ks], w, acc[ct]);
                    }
                }
                // acc[ct][i] = u[n = n0 + 16 ct + 4 kk + i, l = lb + 16 lt + r16]
                const int li = 16 * lt + r16, l = lb + li;
                const bool lok = l < L;
                const int64_t lD = (int64_t)l * D;
                const float m2 = lc[0][li], r2 = lc[1][li], s2 = lc[2][li], b2 = lc[3][li], pv = lc[4][li];
                float t0 = 0.f, t1 = 0.f;
#pragma unroll
                for (int ct = 0; ct < LN_CT; ++ct) {
                    float v[4];
                    if (MODE == LN_BSUMS) {
                        if (ka->vec4 && lok && off[ct][0] >= 0) {
                            const float4 t = *reinterpret_cast<const float4*>(ka->dY + off[ct][0] + lD);
                            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] = (lok && off[ct][i] >= 0) ? ka->dY[off[ct][i] + lD] : 0.f;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const bool ok = lok && off[ct][i] >= 0;
                        const float c = expf(acc[ct][i]);
                        if (MODE == LN_STATS) {
                            const float e = ok ? c - pv : 0.f;
                            t0 += e;
                            t1 += e * e;
                        } else if (MODE == LN_BSUMS) {
                            t0 += v[i];
                            t1 += ok ? v[i] * ((c - m2) * r2) : 0.f;
                        } else {
                            v[i] = (c - m2) * s2 + b2;
                        }
                    }
                    if (MODE == LN_OUT) {
                        if (ka->vec4 && lok && off[ct][0] >= 0) {
                            *reinterpret_cast<float4*>(ka->Y + off[ct][0] + lD) = make_float4(v[0], v[1], v[2], v[3]);
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (lok && off[ct][i] >= 0) ka->Y[off[ct][i] + lD] = v[i];
                        }
                    }
                }
                if (MODE != LN_OUT) {            // the wave's 32 columns of neuron li: the four kk groups meet
                    t0 += __shfl_xor(t0, 16); t0 += __shfl_xor(t0, 32);
                    t1 += __shfl_xor(t1, 16); t1 += __shfl_xor(t1, 32);
                    if (kk == 0) { red[wave][0][li] = t0; red[wave][1][li] = t1; }
                }
            }
            if (MODE != LN_OUT) {
                __syncthreads();
                if (threadIdx.x < 128) {
                    const int q = threadIdx.x >> 6, li = threadIdx.x & 63;
                    if (lb + li < L)
                        sacc[q * LP + lb + li] += (red[0][q][li] + red[1][q][li]) + (red[2][q][li] + red[3][q][li]);
                }
            }
        }
    }
    if (MODE != LN_OUT) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * L; i += LN_NT) {
            const int q = i / L, l = i - q * L;
            ka->part[((int64_t)blockIdx.x * 2 + q) * L + l] = sacc[q * LP + l];
        }
    }
}

// the workgroups' sums about the pivot in a fixed order: mean2 | var2 (biased) and the running update
__global__ __launch_bounds__(256) void k_ln_exp_finish(const float* part, int rows, int L, const float* pivot,
                                                       double n, float momentum, float* mean2, float* var2, float* rm,
                                                       float* rv, int64_t* nbt) {
    const int64_t l = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const bool live = l < L;
    const float s1 = fx_rowsum_col<double, FX_ROWS_SLICES>(part, rows, 2 * (int64_t)L, l, live);
    __syncthreads();
    const float s2 = fx_rowsum_col<double, FX_ROWS_SLICES>(part + L, rows, 2 * (int64_t)L, l, live);
    if (blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
    if (threadIdx.x >= 64 || !live) return;
    const double d = (double)s1 / n;
    double var = (double)s2 / n - d * d;
    if (var < 0.0) var = 0.0;
    const double mean = (double)pivot[l] + d;
    mean2[l] = (float)mean;
    var2[l] = (float)var;
    ln_running(mean, var, n, momentum, rm + l, rv + l);
}

// ---- (e) dahat[f, n] = sum_l W[l, f] du[l, n]; leaves ahat [N, FP] for k_ln_bwd_dw ---------------------------
__global__ __launch_bounds__(LN_NT) void k_ln_bwd_da(LnArgs args) {
    const LnArgs* ka = (const LnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float wl[LN_LC * LN_WS];
    __shared__ float lc[5][64];
    __shared__ float bn1[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int L = ka->L, D = ka->D, F = ka->F, FP = ka->FP;
    const int64_t N = ka->N, ldy = (int64_t)L * D;
    ln_stage_bn1(ka, bn1);
    __syncthreads();
    const int64_t tiles = (N + LN_COLS - 1) / LN_COLS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * LN_COLS + wave * (16 * LN_CT);
        float a[LN_CT][LN_KS];
        int64_t yo[LN_CT];                       // the lane's column n0 + 16 ct + r16 in dY; -1 past N
        f32x4 dacc[4][LN_CT];
#pragma unroll
        for (int ct = 0; ct < LN_CT; ++ct) {
            const int64_t n = n0 + 16 * ct + r16;
            ln_ahat_regs(ka, bn1, n, kk, a[ct]);
            const int64_t b = n < N ? n / D : 0;
            yo[ct] = n < N ? b * ldy + (n - b * D) : -1;
            if (n < N) {
#pragma unroll
                for (int ks = 0; ks < LN_KS; ++ks)
                    if (ks < ka->KS) ka->ahat[n * FP + 4 * ks + kk] = a[ct][ks];
            }
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) dacc[ft][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int lb = 0; lb < L; lb += LN_LC) {
            __syncthreads();
            ln_stage_chunk(ka, lb, wl, lc);
            __syncthreads();
            for (int lt = 0; lt < LN_LC / 16 && lb + 16 * lt < L; ++lt) {
                f32x4 acc[LN_CT];
#pragma unroll
                for (int ct = 0; ct < LN_CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                const float* wp = wl + (16 * lt + r16) * LN_WS + kk;
#pragma unroll
                for (int ks = 0; ks < LN_KS; ++ks) {
                    if (ks < ka->KS) {
                        const float w = wp[4 * ks];
#pragma unroll
                        for (int ct = 0; ct < LN_CT; ++ct) acc[ct] = ln_mfma(w, a[ct][ks], acc[ct]);
                    }
                }
                // acc[ct][i] = u[l = lb + 16 lt + 4 kk + i, n = n0 + 16 ct + r16] -> du in place
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int li = 16 * lt + 4 * kk + i, l = lb + li;
                    const float m2 = lc[0][li], r2 = lc[1][li], s2 = lc[2][li], mdy = lc[3][li], mdyc = lc[4][li];
#pragma unroll
                    for (int ct = 0; ct < LN_CT; ++ct) {
                        const bool ok = l < L && yo[ct] >= 0;
                        const float c = expf(acc[ct][i]);
                        const float dy = ok ? ka->dY[yo[ct] + (int64_t)l * D] : 0.f;
                        const float dc = s2 * (dy - mdy - ((c - m2) * r2) * mdyc);
                        acc[ct][i] = ok ? dc * c : 0.f;
                    }
                }
                // k-slot kk of step i is neuron 16 lt + 4 kk + i: du is the B operand as it lies
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* wq = wl + (16 * lt + 4 * kk + i) * LN_WS + r16;
#pragma unroll
                    for (int ft = 0; ft < 4; ++ft) {
                        if (ft < ka->FT) {
                            const float w = wq[16 * ft];
#pragma unroll
                            for (int ct = 0; ct < LN_CT; ++ct) dacc[ft][ct] = ln_mfma(w, acc[ct][i], dacc[ft][ct]);
                        }
                    }
                }
            }
        }
        // dacc[ft][ct][i] = dahat[f = 16 ft + 4 kk + i, n = n0 + 16 ct + r16]
#pragma unroll
        for (int ct = 0; ct < LN_CT; ++ct) {
            const int64_t n = n0 + 16 * ct + r16;
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = 16 * ft + 4 * kk + i;
                    if (n < N && f < F) ka->dahat[(int64_t)f * ka->NP + n] = dacc[ft][ct][i];
                }
            }
        }
    }
}

// ---- (e) dW[l, f] = sum_n du[l, n] ahat[f, n]: workgroup (64 neurons, slab), partial [slabs, L, F] -------------
__global__ __launch_bounds__(LN_NT) void k_ln_bwd_dw(LnArgs args) {
    const LnArgs* ka = (const LnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float at[64 * LN_WS];             // ahat of 64 columns: [n, f]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int L = ka->L, D = ka->D, F = ka->F, FP = ka->FP;
    const int64_t N = ka->N;
    const int l = blockIdx.x * LN_LC + 16 * wave + r16;
    const bool lok = l < L;
    float wreg[LN_KS];
#pragma unroll
    for (int ks = 0; ks < LN_KS; ++ks) {
        const int f = 4 * ks + kk;
        wreg[ks] = (lok && f < F) ? ka->W[(int64_t)l * F + f] : 0.f;
    }
    float m2 = 0.f, r2 = 0.f, s2 = 0.f, mdy = 0.f, mdyc = 0.f;
    if (lok) {
        const float inv_n = 1.f / (float)N;
        m2 = ka->mean2[l];
        r2 = 1.f / sqrtf(ka->var2[l] + ka->eps);
        s2 = ka->g2[l] * r2;
        mdy = ka->sdy[l] * inv_n;
        mdyc = ka->sdyc[l] * inv_n;
    }
    const int64_t lD = (int64_t)l * D;
    f32x4 dacc[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) dacc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t tiles = (N + 63) / 64;
    for (int64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const int64_t n0 = tile * 64;
        __syncthreads();
        for (int idx = threadIdx.x; idx < 64 * 64; idx += LN_NT) {
            const int r = idx >> 6, f = idx & 63;
            at[r * LN_WS + f] = (n0 + r < N && f < FP) ? ka->ahat[(n0 + r) * FP + f] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < 4 && n0 + 16 * j < N; ++j) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* ap = at + (16 * j + r16) * LN_WS + kk;
#pragma unroll
            for (int ks = 0; ks < LN_KS; ++ks)
                if (ks < ka->KS) acc = ln_mfma(ap[4 * ks], wreg[ks], acc);
            // acc[i] = u[n = n0 + 16 j + 4 kk + i, l] -> du
            int64_t off[4];
            ln_col_offsets(ka, n0 + 16 * j + 4 * kk, off);
            float dy[4];
            if (ka->vec4 && lok && off[0] >= 0) {
                const float4 t = *reinterpret_cast<const float4*>(ka->dY + off[0] + lD);
                dy[0] = t.x; dy[1] = t.y; dy[2] = t.z; dy[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) dy[i] = (lok && off[i] >= 0) ? ka->dY[off[i] + lD] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float c = expf(acc[i]);
                const float dc = s2 * (dy[i] - mdy - ((c - m2) * r2) * mdyc);
                acc[i] = (lok && off[i] >= 0) ? dc * c : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* aq = at + (16 * j + 4 * kk + i) * LN_WS + r16;
#pragma unroll
                for (int ft = 0; ft < 4; ++ft)
                    if (ft < ka->FT) dacc[ft] = ln_mfma(aq[16 * ft], acc[i], dacc[ft]);
            }
        }
    }
    // dacc[ft][i] = dW[l, f = 16 ft + 4 kk + i] of this slab
    if (lok) {
        float* dst = ka->dwpart + ((int64_t)blockIdx.y * L + l) * F;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = 16 * ft + 4 * kk + i;
                if (f < F) dst[f] = dacc[ft][i];
            }
        }
    }
}

// ---- (f) BN_log backward: per chunk and field sum dahat | sum dahat a0, then dx ---------------------------
__global__ __launch_bounds__(LN_NT) void k_ln_da_stats(LnArgs args, int64_t per, float* dpart) {
    const LnArgs* ka = (const LnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = ka->D, F = ka->F;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < ka->N ? lo + per : ka->N;
    for (int f = wave; f < F; f += 4) {
        const float mean = ka->mean1[f], rstd = 1.f / sqrtf(ka->var1[f] + ka->eps);
        float s = 0.f, q = 0.f;
        for (int64_t n = lo + lane; n < hi; n += 64) {
            const int64_t b = n / D;
            const float da = ka->dahat[(int64_t)f * ka->NP + n];
            s += da;
            q += da * ((ln_log(ka->X[b * ka->x_ld + f * D + (n - b * D)]) - mean) * rstd);
        }
        s = fx_wave_sum(s);
        q = fx_wave_sum(q);
        if (lane == 0) {
            dpart[((int64_t)blockIdx.x * 2 + 0) * F + f] = s;
            dpart[((int64_t)blockIdx.x * 2 + 1) * F + f] = q;
        }
    }
}

__global__ __launch_bounds__(LN_NT) void k_ln_dx(LnArgs args, const float* dbeta1, const float* dgamma1, float* dX,
                                                 int64_t dx_ld, int accumulate) {
    const LnArgs* ka = (const LnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int D = ka->D, FD = ka->F * D;
    const int64_t total = ka->B * FD;
    const float inv_n = 1.f / (float)ka->N;
    for (int64_t idx = (int64_t)blockIdx.x * LN_NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * LN_NT) {
        const int64_t b = idx / FD;
        const int r = (int)(idx - b * FD), f = r / D, d = r - f * D;
        const float x = ka->X[b * ka->x_ld + r];
        const float rstd = 1.f / sqrtf(ka->var1[f] + ka->eps);
        const float a0 = (ln_log(x) - ka->mean1[f]) * rstd;
        const float dah = ka->dahat[(int64_t)f * ka->NP + b * D + d];
        const float da = ka->g1[f] * rstd * (dah - dbeta1[f] * inv_n - a0 * (dgamma1[f] * inv_n));
        // clamp passes the gradient where |x| >= 1e-5, abs gives it the sign of x: da sign(x) / |x| = da / x
        const float g = fabsf(x) >= LN_CLAMP ? da / x : 0.f;
        float* dst = dX + b * dx_ld + r;
        *dst = accumulate ? *dst + g : g;
    }
}

// ---- hosts ----------------------------------------------------------------------------------------------
static int64_t ln_up4(int64_t n) { return (n + 3) / 4 * 4; }

static int64_t ln_workgroups(int64_t N) {
    const int64_t tiles = fx_ceil_div(N > 0 ? N : 1, LN_COLS);
    return tiles < LN_MAX_WG ? tiles : LN_MAX_WG;
}

// the per-field statistics: chunks of `per` columns, at most LN_CHUNKS of them
static int64_t ln_chunk_cols(int64_t N) {
    const int64_t per = fx_ceil_div(N > 0 ? N : 1, LN_CHUNKS);
    return per < 64 ? 64 : per;
}

static int ln_slabs(int64_t N, int L) {
    const int64_t tiles = fx_ceil_div(N > 0 ? N : 1, 64), want = LN_MAX_WG / fx_ceil_div(L, LN_LC);
    const int64_t s = want < 1 ? 1 : want > LN_MAX_SLABS ? LN_MAX_SLABS : want;
    return (int)(s < tiles ? s : tiles);
}

static bool ln_shape_ok(int64_t B, int32_t F, int32_t D, int32_t L) {
    return B >= 0 && F >= 1 && F <= LN_MAX_F && D >= 1 && D <= LN_MAX_D && L >= 1 && L <= LN_MAX_L;
}

static int ln_fill(const char* who, LnArgs& p, const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D,
                   const float* W, int32_t L, float eps) {
    FX_CHECK_ARG(F >= 1 && F <= LN_MAX_F, "%s: F=%d, limit 1 <= F <= %d", who, F, LN_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= LN_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, LN_MAX_D);
    FX_CHECK_ARG(L >= 1 && L <= LN_MAX_L, "%s: L=%d, limit 1 <= L <= %d", who, L, LN_MAX_L);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: X sample stride %lld < F*D", who, (long long)x_ld);
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B; p.N = B * D; p.NP = ln_up4(B * D);
    p.F = F; p.D = D; p.L = L; p.KS = (F + 3) / 4; p.FP = 4 * p.KS; p.FT = (F + 15) / 16;
    p.W = W; p.eps = eps;
    return FX_OK;
}

extern "C" void fx_lognet_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = LN_MAX_F;
    limits[1] = LN_MAX_D;
    limits[2] = LN_MAX_L;
    limits[3] = LN_COLS;
    limits[4] = LN_MAX_WG;
    limits[5] = LN_CHUNKS;
}

extern "C" int64_t fx_lognet_workspace_floats(int64_t B, int32_t F, int32_t D, int32_t L) {
    if (!ln_shape_ok(B, F, D, L)) return 0;
    const int64_t N = B * D, wg = ln_workgroups(N), FP = (F + 3) / 4 * 4;
    const int64_t fwd = ln_up4(LN_CHUNKS * 2 * F) + ln_up4(L) + wg * 2 * L;
    const int64_t bwd = N * FP + (int64_t)F * ln_up4(N) + ln_up4(wg * 2 * L) + ln_up4(LN_CHUNKS * 2 * F) +
                        (int64_t)ln_slabs(N, L) * L * F;
    return fwd > bwd ? fwd : bwd;
}

extern "C" int fx_lognet_fwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W, int32_t L,
                             const float* gamma1, const float* beta1, const float* gamma2, const float* beta2,
                             float eps, float momentum, int32_t training, float* running_mean1, float* running_var1,
                             int64_t* num_batches_tracked1, float* running_mean2, float* running_var2,
                             int64_t* num_batches_tracked2, float* stats, float* Y, float* workspace,
                             fx_stream_t stream) {
    const char* who = "fx_lognet_fwd";
    LnArgs p;
    if (int st = ln_fill(who, p, X, x_ld, B, F, D, W, L, eps)) return st;
    FX_CHECK_ARG(!training || p.N >= 2, "%s: B*D=%lld: training-mode batch statistics need more than 1 value per "
                 "channel", who, (long long)p.N);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(X && W && gamma1 && beta1 && gamma2 && beta2 && Y, "%s: null X / W / gamma / beta / Y", who);
    FX_CHECK_ARG(running_mean1 && running_var1 && running_mean2 && running_var2, "%s: null running statistics", who);
    FX_CHECK_ARG(!training || (stats && workspace && num_batches_tracked1 && num_batches_tracked2),
                 "%s: null stats / workspace / num_batches_tracked in training", who);
    hipStream_t s = fx_hip_stream(stream);
    p.g1 = gamma1; p.b1 = beta1; p.g2 = gamma2;
    p.Y = Y; p.vec4 = D % 4 == 0 && fx_al16(Y);
    const int64_t wg = ln_workgroups(p.N);
    const size_t sacc_bytes = sizeof(float) * 2 * ((L + 63) / 64 * 64);
    if (training) {
        float* lpart = workspace;
        float* pivot = lpart + ln_up4(LN_CHUNKS * 2 * F);
        p.part = pivot + ln_up4(L);
        p.mean1 = stats; p.var1 = stats + F; p.mean2 = nullptr; p.var2 = nullptr;
        const int64_t per = ln_chunk_cols(p.N);
        const int chunks = (int)fx_ceil_div(p.N, per);
        hipLaunchKernelGGL(k_ln_log_stats, dim3((unsigned)chunks), dim3(LN_NT), 0, s, p, per, lpart);
        FX_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ln_log_finish, dim3((unsigned)fx_ceil_div(L, LN_NT)), dim3(LN_NT), 0, s, p, lpart, chunks,
                           per, momentum, stats, stats + F, running_mean1, running_var1, num_batches_tracked1, pivot);
        FX_CHECK_LAUNCH();
        p.pivot = pivot;
        hipLaunchKernelGGL(k_ln_cols<LN_STATS>, dim3((unsigned)wg), dim3(LN_NT), sacc_bytes, s, p);
        FX_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ln_exp_finish, dim3((unsigned)fx_ceil_div(L, 64)), dim3(256), 0, s, p.part, (int)wg, L,
                           pivot, (double)p.N, momentum, stats + 2 * F, stats + 2 * F + L, running_mean2,
                           running_var2, num_batches_tracked2);
        FX_CHECK_LAUNCH();
        p.pivot = nullptr;
        p.mean2 = stats + 2 * F; p.var2 = stats + 2 * F + L;
    } else {
        p.mean1 = running_mean1; p.var1 = running_var1; p.mean2 = running_mean2; p.var2 = running_var2;
    }
    p.b2 = beta2;
    hipLaunchKernelGGL(k_ln_cols<LN_OUT>, dim3((unsigned)wg), dim3(LN_NT), 0, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_lognet_bwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W, int32_t L,
                             const float* gamma1, const float* beta1, const float* gamma2, float eps,
                             const float* stats, const float* dY, float* dX, int64_t dx_ld, int32_t dx_accumulate,
                             float* dW, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2,
                             float* workspace, fx_stream_t stream) {
    const char* who = "fx_lognet_bwd";
    LnArgs p;
    if (int st = ln_fill(who, p, X, x_ld, B, F, D, W, L, eps)) return st;
    FX_CHECK_ARG(dx_ld >= (int64_t)F * D, "%s: dX sample stride %lld < F*D", who, (long long)dx_ld);
    FX_CHECK_ARG(p.N >= 2, "%s: B*D=%lld (the batch statistics' gradient needs more than 1 value per channel)", who,
                 (long long)p.N);
    FX_CHECK_ARG(X && W && gamma1 && beta1 && gamma2 && stats && dY && dX && dW && dgamma1 && dbeta1 && dgamma2 &&
                 dbeta2 && workspace, "%s: null X / W / gamma / beta / stats / dY / dX / gradient / workspace", who);
    hipStream_t s = fx_hip_stream(stream);
    const int64_t wg = ln_workgroups(p.N), per = ln_chunk_cols(p.N);
    const int chunks = (int)fx_ceil_div(p.N, per), slabs = ln_slabs(p.N, L);
    p.ahat = workspace;
    p.dahat = p.ahat + p.N * p.FP;
    p.part = p.dahat + (int64_t)F * p.NP;
    float* dpart = p.part + ln_up4(wg * 2 * L);
    p.dwpart = dpart + ln_up4(LN_CHUNKS * 2 * F);
    p.g1 = gamma1; p.b1 = beta1; p.g2 = gamma2;
    p.mean1 = stats; p.var1 = stats + F; p.mean2 = stats + 2 * F; p.var2 = stats + 2 * F + L;
    p.dY = dY; p.vec4 = D % 4 == 0 && fx_al16(dY);
    // (d) dbeta2 = sum dY, dgamma2 = sum dY chat
    const size_t sacc_bytes = sizeof(float) * 2 * ((L + 63) / 64 * 64);
    hipLaunchKernelGGL(k_ln_cols<LN_BSUMS>, dim3((unsigned)wg), dim3(LN_NT), sacc_bytes, s, p);
    FX_CHECK_LAUNCH();
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, p.part, (int)wg, 2 * (int64_t)L,
                                                   fx_rowsum_out(dbeta2, L, dgamma2, L)))
        return st;
    // (e) dahat (and ahat), then dW
    p.sdy = dbeta2; p.sdyc = dgamma2;
    hipLaunchKernelGGL(k_ln_bwd_da, dim3((unsigned)wg), dim3(LN_NT), 0, s, p);
    FX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ln_bwd_dw, dim3((unsigned)fx_ceil_div(L, LN_LC), (unsigned)slabs), dim3(LN_NT), 0, s, p);
    FX_CHECK_LAUNCH();
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, p.dwpart, slabs, (int64_t)L * F,
                                                   fx_rowsum_out(dW, (int64_t)L * F)))
        return st;
    // (f) BN_log backward and the log / clamp / abs chain
    hipLaunchKernelGGL(k_ln_da_stats, dim3((unsigned)chunks), dim3(LN_NT), 0, s, p, per, dpart);
    FX_CHECK_LAUNCH();
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, dpart, chunks, 2 * (int64_t)F,
                                                   fx_rowsum_out(dbeta1, F, dgamma1, F)))
        return st;
    const int64_t total = B * F * D;
    const int64_t blocks = fx_ceil_div(total, LN_NT);
    hipLaunchKernelGGL(k_ln_dx, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(LN_NT), 0, s, p, dbeta1, dgamma1,
                       dX, dx_ld, dx_accumulate);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
