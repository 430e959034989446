// fx_sam.hip — SAM's self-attentive interactions: SAM2A / SAM2E with the model's final linear folded in (below), and the
// stackable layers SAM3A / SAM3E (second half of the file).
// Reference: model_zoo/SAM/src/SAM.py:150-204 (SAM2A.forward, SAM2E.forward) and :67, :88 (fc on the flattened block).
// The reference forms out [B, F, F, D] = S (.) W (2A) or S (.) U (2E), S = X X^T, U[n, m, d] = X[n, d] X[m, d], and feeds
// it flattened to fc = Linear(F F D, 1).  With w = fc.weight viewed [F, F, D] the logit never needs that tensor:
//     2A: logit_b = <S_b, G> + bias,  G[n, m] = sum_d W[n, m, d] w[n, m, d]               (G is the same for every sample)
//     2E: logit_b = sum_{n, m} S_b[n, m] T_b[n, m] + bias,  T_b[n, m] = sum_d X[n, d] X[m, d] w[n, m, d]
// S and U are symmetric in (n, m), so only the symmetric part of G and of w counts: a prologue launch writes
// Gsym = G + G^T [F, F] (2A) or wsym[n, m, d] = w[n, m, d] + w[m, n, d] in two layouts, [D, F, F] and [F, F, D] (2E), into
// workspace; the main passes read W and w nowhere else, take the pairs n <= m only, and count the diagonal half.
//
// Work split: 256-thread workgroups grid-strided over tiles of ST <= 4 samples; a tile's X sits in LDS as ST images
// [FP, XS] (FP = F rounded up to 16, row stride XS = D rounded up to 16, + 1: odd), zeros past F and D.
// Products on v_mfma_f32_16x16x4_f32: lane (r16 = lane & 15, kk = lane >> 4) holds element (r16, k = kk) of A and
// (k = kk, r16) of B and rows 4 kk + i of column r16 of the result; sam_mm reads both operands from LDS with free row
// and column strides, so a transposed operand costs nothing.
//   k_sam_prep       : Gsym, or wsym in both layouts.
//   k_sam_logit_fwd  : 2A: per sample the upper-triangle 16 x 16 tiles of S = X X^T on the MFMA, multiplied in registers
//     with the staged coefficient tile (Gsym above the diagonal, half of it on it, 0 below) and summed: S never leaves
//     the registers.  2E: a thread owns a pair (n <= m) and walks d: p = X[n, d] X[m, d] gives S (sum p) and T
//     (sum p wsym) together, wsym read [D, F, F] (coalesced over the pairs) once per tile of samples.  One float per
//     sample leaves the kernel.
//   k_sam_logit_bwd  : 2A: dX_b = dlogit_b Gsym X_b on the MFMA; dG = sum_b dlogit_b X_b X_b^T accumulates over the
//     workgroup's samples in persistent upper-triangle accumulator tiles (K = the samples' d) and leaves as one partial
//     row per workgroup (tile list, <= 10 x 256 floats).  2E: the pair walk again gives S and Tsym (staged in LDS,
//     mirrored) and dlogit_b S_b -> workspace [B, F, F]; then a thread per (n, d) walks m:
//     dX[n, d] = dlogit sum_m (Tsym[n, m] + S[n, m] wsym[n, m, d]) X[m, d], wsym read [F, F, D].
//   k_sam_dw2a       : dW = dG (.) w, dw = dG (.) W, broadcast over d (after the fixed-order sum of the partial rows).
//   k_sam_dw2e       : dw[n, m, d] = sum_b (dlogit_b S_b[n, m]) X_b[n, d] X_b[m, d]: a workgroup owns 64 outputs (n <= m, d),
//     its four waves walk a quarter of the batch each, in order and in fp64; both triangles are written.
// dbias rides as one more column of the partial rows.  fx_rowsum adds them in a fixed order; no atomics: two runs give
// the same bits, launch counts depend on shapes only (forward 2, backward 2A 4, 2E 4).
#include "fx_common.h"
#include "fx_rowsum.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SAM_MAX_F 64
#define SAM_MAX_D 64
#define SAM_NT 256
#define SAM_MAX_ST 4            // most samples of a tile
#define SAM_MAX_WG 512          // workgroups of the main passes: the rows of their partial sums
#define SAM_TILE_FLOATS 12288   // LDS floats a tile's images aim at (48 KiB); one sample always fits in 160 KiB
#define SAM_LDS_MAX (160 * 1024)
#define SAM_2A 0
#define SAM_2E 1

struct SamArgs {
    const float* X; int64_t x_ld; int64_t B;
    int F, D, FP, NT, XS, GS, KS, FK, DT, ST, type;     // NT = FP / 16, GS = FP + 1, KS = ceil(D / 4), FK = ceil(F / 4)
    int ntri, bcol; int64_t ldp;                        // DT = ceil(D / 16); bcol: dbias's column of a partial row
    const float* W; const float* w; const float* bias;
    float* gsym;                                        // [F, F]
    float* wsT; float* wsf;                             // wsym [D, F, F] | [F, F, D]
    float* logit; const float* dlogit;
    float* dX; int64_t dx_ld; int dx_acc;
    float* gS;                                          // dlogit_b S_b [B, F, F]
    float* part;                                        // [workgroups, ldp]
    float* dgt;                                         // the summed tile list of dG, then dbias
    float* dW; float* dw;
};

__device__ __forceinline__ f32x4 sam_mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc[i] += sum_k A[16 mt + r, k] B[k, 16 nt + c] at (r = 4 kk + i, c = r16); A[r, k] = A[r ars + k acs], B alike
__device__ __forceinline__ f32x4 sam_mm(const float* A, int ars, int acs, const float* B, int brs, int bcs, int mt,
                                        int nt, int k4, int r16, int kk, float scale, f32x4 acc) {
    const float* ap = A + (16 * mt + r16) * ars + kk * acs;
    const float* bp = B + kk * brs + (16 * nt + r16) * bcs;
    for (int ks = 0; ks < k4; ++ks) acc = sam_mfma(scale * ap[4 * ks * acs], bp[4 * ks * brs], acc);
    return acc;
}

// tile t of the upper triangle of [NT, NT] tiles, row by row -> (mt <= nt)
__device__ __forceinline__ void sam_tri(int t, int NT, int& mt, int& nt) {
    mt = 0;
    while (t >= NT - mt) { t -= NT - mt; ++mt; }
    nt = mt + t;
}

__host__ __device__ __forceinline__ int sam_tri_index(int mt, int nt, int NT) {
    return mt * NT - mt * (mt - 1) / 2 + (nt - mt);
}

// the tile's X images: xs[s][n, d], zeros past F, D and the batch
__device__ __forceinline__ void sam_stage_x(const SamArgs* ka, int64_t b0, float* xs) {
    const int per = ka->FP * ka->XS;
    for (int s = 0; s < ka->ST; ++s) {
        const bool live = b0 + s < ka->B;
        const float* x = ka->X + (live ? (b0 + s) * ka->x_ld : 0);
        for (int idx = threadIdx.x; idx < per; idx += SAM_NT) {
            const int n = idx / ka->XS, d = idx - n * ka->XS;
            xs[s * per + idx] = (live && n < ka->F && d < ka->D) ? x[n * ka->D + d] : 0.f;
        }
    }
}

// ---- prologue: the symmetric parts ---------------------------------------------------------------------------------
__global__ __launch_bounds__(SAM_NT) void k_sam_prep(SamArgs args) {
    const SamArgs* ka = (const SamArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int F = ka->F, D = ka->D, FF = F * F;
    const int total = ka->type == SAM_2A ? FF : FF * D;
    for (int idx = blockIdx.x * SAM_NT + threadIdx.x; idx < total; idx += gridDim.x * SAM_NT) {
        if (ka->type == SAM_2A) {
            const int n = idx / F, m = idx - n * F;
            const float *W1 = ka->W + (int64_t)idx * D, *w1 = ka->w + (int64_t)idx * D;
            const float *W2 = ka->W + (int64_t)(m * F + n) * D, *w2 = ka->w + (int64_t)(m * F + n) * D;
            float g1 = 0.f, g2 = 0.f;
            for (int d = 0; d < D; ++d) {
                g1 += W1[d] * w1[d];
                g2 += W2[d] * w2[d];
            }
            ka->gsym[idx] = g1 + g2;
        } else {
            const int p = idx / D, d = idx - p * D, n = p / F, m = p - n * F;
            const float v = ka->w[idx] + ka->w[(int64_t)(m * F + n) * D + d];
            ka->wsf[idx] = v;
            ka->wsT[(int64_t)d * FF + p] = v;
        }
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAM_NT) void k_sam_logit_fwd(SamArgs args) {
    const SamArgs* ka = (const SamArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) float sam_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int F = ka->F, D = ka->D, FP = ka->FP, XS = ka->XS, GS = ka->GS, ST = ka->ST, FF = F * F;
    const int64_t B = ka->B;
    float* red = sam_lds;                       // [SAM_MAX_ST, 4]
    float* xs = red + 4 * SAM_MAX_ST;           // [ST, FP, XS]
    float* gc = xs + ST * FP * XS;              // 2A: the coefficient image [FP, GS]
    if (ka->type == SAM_2A) {
        for (int idx = threadIdx.x; idx < FP * GS; idx += SAM_NT) {
            const int n = idx / GS, m = idx - n * GS;
            const float g = (n < F && m < F && n <= m) ? ka->gsym[n * F + m] : 0.f;
            gc[idx] = n == m ? 0.5f * g : g;
        }
    }
    const float bias = ka->bias[0];
    const int64_t tiles = (B + ST - 1) / ST;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * ST;
        __syncthreads();                        // the last tile's readers are done
        sam_stage_x(ka, b0, xs);
        __syncthreads();
        float part[SAM_MAX_ST];
#pragma unroll
        for (int s = 0; s < SAM_MAX_ST; ++s) part[s] = 0.f;
        if (ka->type == SAM_2A) {
            for (int t = wave; t < ka->ntri; t += 4) {
                int mt, nt;
                sam_tri(t, ka->NT, mt, nt);
                const float* gp = gc + (16 * mt + 4 * kk) * GS + 16 * nt + r16;
#pragma unroll
                for (int s = 0; s < SAM_MAX_ST; ++s) {
                    if (s < ST) {
                        const float* x = xs + s * FP * XS;
                        const f32x4 acc = sam_mm(x, XS, 1, x, 1, XS, mt, nt, ka->KS, r16, kk, 1.f,
                                                 f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                        for (int i = 0; i < 4; ++i) part[s] += acc[i] * gp[i * GS];
                    }
                }
            }
        } else {
            for (int p = threadIdx.x; p < FF; p += SAM_NT) {
                const int n = p / F, m = p - n * F;
                if (n > m) continue;
                float S[SAM_MAX_ST], T[SAM_MAX_ST];
#pragma unroll
                for (int s = 0; s < SAM_MAX_ST; ++s) S[s] = T[s] = 0.f;
                for (int d = 0; d < D; ++d) {
                    const float wv = ka->wsT[(int64_t)d * FF + p];
#pragma unroll
                    for (int s = 0; s < SAM_MAX_ST; ++s) {
                        if (s < ST) {
                            const float pr = xs[s * FP * XS + n * XS + d] * xs[s * FP * XS + m * XS + d];
                            S[s] += pr;
                            T[s] += pr * wv;
                        }
                    }
                }
                const float c = n == m ? 0.5f : 1.f;
#pragma unroll
                for (int s = 0; s < SAM_MAX_ST; ++s) part[s] += c * (S[s] * T[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < SAM_MAX_ST; ++s) {
            const float v = fx_wave_sum(part[s]);
            if (lane == 0) red[4 * s + wave] = v;
        }
        __syncthreads();
        if ((int)threadIdx.x < ST && b0 + threadIdx.x < B) {
            const float* r = red + 4 * threadIdx.x;
            ka->logit[b0 + threadIdx.x] = ((r[0] + r[1]) + (r[2] + r[3])) + bias;
        }
    }
}

// ---- backward: dX, dbias, and what the parameter-gradient launch needs ---------------------------------------------
__global__ __launch_bounds__(SAM_NT) void k_sam_logit_bwd(SamArgs args) {
    const SamArgs* ka = (const SamArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) float sam_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int F = ka->F, D = ka->D, FP = ka->FP, XS = ka->XS, GS = ka->GS, ST = ka->ST, FF = F * F;
    const int64_t B = ka->B;
    float* xs = sam_lds;                        // [ST, FP, XS]
    float* gs = xs + ST * FP * XS;              // 2A: Gsym [FP, GS];  2E: S [ST, FP, GS], then Tsym [ST, FP, GS]
    float* ts = gs + ST * FP * GS;
    if (ka->type == SAM_2A) {
        for (int idx = threadIdx.x; idx < FP * GS; idx += SAM_NT) {
            const int n = idx / GS, m = idx - n * GS;
            gs[idx] = (n < F && m < F) ? ka->gsym[n * F + m] : 0.f;
        }
    }
    f32x4 dg[3];                                // 2A: this wave's upper-triangle tiles of dG
#pragma unroll
    for (int j = 0; j < 3; ++j) dg[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbias = 0.f;                          // thread 0's
    const int64_t tiles = (B + ST - 1) / ST;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * ST;
        __syncthreads();
        sam_stage_x(ka, b0, xs);
        __syncthreads();
        float g[SAM_MAX_ST];
#pragma unroll
        for (int s = 0; s < SAM_MAX_ST; ++s) {
            g[s] = (s < ST && b0 + s < B) ? ka->dlogit[b0 + s] : 0.f;
            dbias += g[s];
        }
        if (ka->type == SAM_2A) {
            // dX_b[n, d] = g_b sum_m Gsym[n, m] X_b[m, d]
            for (int t = wave; t < ST * ka->NT * ka->DT; t += 4) {
                const int s = t / (ka->NT * ka->DT), r = t - s * ka->NT * ka->DT, mt = r / ka->DT, nt = r - mt * ka->DT;
                const f32x4 acc = sam_mm(gs, GS, 1, xs + s * FP * XS, XS, 1, mt, nt, ka->FK, r16, kk, 1.f,
                                         f32x4{0.f, 0.f, 0.f, 0.f});
                const int d = 16 * nt + r16;
                if (b0 + s < B && d < D) {
                    const float gb = ka->dlogit[b0 + s];
                    float* dx = ka->dX + (b0 + s) * ka->dx_ld + d;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int n = 16 * mt + 4 * kk + i;
                        if (n < F) dx[n * D] = gb * acc[i] + (ka->dx_acc ? dx[n * D] : 0.f);
                    }
                }
            }
            // dG[n, m] += g_b sum_d X_b[n, d] X_b[m, d], n <= m tiles
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int t = wave + 4 * j;
                if (t < ka->ntri) {
                    int mt, nt;
                    sam_tri(t, ka->NT, mt, nt);
#pragma unroll
                    for (int s = 0; s < SAM_MAX_ST; ++s) {
                        if (s < ST) {
                            const float* x = xs + s * FP * XS;
                            dg[j] = sam_mm(x, XS, 1, x, 1, XS, mt, nt, ka->KS, r16, kk, g[s], dg[j]);
                        }
                    }
                }
            }
        } else {
            // the pair walk: S and Tsym of every sample of the tile, mirrored; g S leaves for the dw launch
            for (int p = threadIdx.x; p < FF; p += SAM_NT) {
                const int n = p / F, m = p - n * F;
                if (n > m) continue;
                float S[SAM_MAX_ST], T[SAM_MAX_ST];
#pragma unroll
                for (int s = 0; s < SAM_MAX_ST; ++s) S[s] = T[s] = 0.f;
                for (int d = 0; d < D; ++d) {
                    const float wv = ka->wsT[(int64_t)d * FF + p];
#pragma unroll
                    for (int s = 0; s < SAM_MAX_ST; ++s) {
                        if (s < ST) {
                            const float pr = xs[s * FP * XS + n * XS + d] * xs[s * FP * XS + m * XS + d];
                            S[s] += pr;
                            T[s] += pr * wv;
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < SAM_MAX_ST; ++s) {
                    if (s < ST) {
                        gs[s * FP * GS + n * GS + m] = gs[s * FP * GS + m * GS + n] = S[s];
                        ts[s * FP * GS + n * GS + m] = ts[s * FP * GS + m * GS + n] = T[s];
                        if (b0 + s < B) {
                            float* o = ka->gS + (b0 + s) * FF;
                            o[n * F + m] = o[m * F + n] = g[s] * S[s];
                        }
                    }
                }
            }
            __syncthreads();
            // dX_b[n, d] = g_b sum_m (Tsym[n, m] + S[n, m] wsym[n, m, d]) X_b[m, d]
            for (int q = threadIdx.x; q < F * D; q += SAM_NT) {
                const int n = q / D, d = q - n * D;
                float acc[SAM_MAX_ST];
#pragma unroll
                for (int s = 0; s < SAM_MAX_ST; ++s) acc[s] = 0.f;
                for (int m = 0; m < F; ++m) {
                    const float wv = ka->wsf[(int64_t)(n * F + m) * D + d];
#pragma unroll
                    for (int s = 0; s < SAM_MAX_ST; ++s) {
                        if (s < ST)
                            acc[s] += (ts[s * FP * GS + n * GS + m] + gs[s * FP * GS + n * GS + m] * wv) *
                                      xs[s * FP * XS + m * XS + d];
                    }
                }
#pragma unroll
                for (int s = 0; s < SAM_MAX_ST; ++s) {
                    if (s < ST && b0 + s < B) {
                        float* dx = ka->dX + (b0 + s) * ka->dx_ld + q;
                        *dx = g[s] * acc[s] + (ka->dx_acc ? *dx : 0.f);
                    }
                }
            }
        }
    }
    // the workgroup's partial row: the tile list of dG (2A), then dbias
    float* row = ka->part + (int64_t)blockIdx.x * ka->ldp;
    if (ka->type == SAM_2A) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int t = wave + 4 * j;
            if (t < ka->ntri) {
#pragma unroll
                for (int i = 0; i < 4; ++i) row[t * 256 + (4 * kk + i) * 16 + r16] = dg[j][i];
            }
        }
    }
    if (threadIdx.x == 0) row[ka->bcol] = dbias;
}

// ---- 2A: dW = dG (.) w, dw = dG (.) W ------------------------------------------------------------------------------
__global__ __launch_bounds__(SAM_NT) void k_sam_dw2a(SamArgs args) {
    const SamArgs* ka = (const SamArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int F = ka->F, D = ka->D;
    const int total = F * F * D;
    for (int idx = blockIdx.x * SAM_NT + threadIdx.x; idx < total; idx += gridDim.x * SAM_NT) {
        const int p = idx / D, n = p / F, m = p - n * F;
        const int a = n < m ? n : m, b = n < m ? m : n;
        const float g = ka->dgt[sam_tri_index(a >> 4, b >> 4, ka->NT) * 256 + (a & 15) * 16 + (b & 15)];
        ka->dW[idx] = g * ka->w[idx];
        ka->dw[idx] = g * ka->W[idx];
    }
}

// ---- 2E: dw[n, m, d] = sum_b (g_b S_b[n, m]) X_b[n, d] X_b[m, d], both triangles ------------------------------------
// 64 outputs per workgroup; wave q walks the q-th quarter of the batch in order, in fp64; the quarters meet as
// (q0 + q1) + (q2 + q3)
__global__ __launch_bounds__(SAM_NT) void k_sam_dw2e(SamArgs args) {
    const SamArgs* ka = (const SamArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int F = ka->F, D = ka->D, FF = F * F;
    const int idx = blockIdx.x * 64 + lane;      // over the F (F + 1) / 2 pairs n <= m, row by row, times D
    const bool live = idx < F * (F + 1) / 2 * D;
    int q = idx / D, n = 0;
    const int d = idx - q * D;
    while (live && q >= F - n) { q -= F - n; ++n; }
    const int m = n + q;
    double acc = 0.0;
    if (live) {
        const int64_t per = (ka->B + 3) / 4, lo = wave * per, hi = lo + per < ka->B ? lo + per : ka->B;
        const float* gS = ka->gS + n * F + m;
        const float *xn = ka->X + n * D + d, *xm = ka->X + m * D + d;
        for (int64_t b = lo; b < hi; ++b) acc += (double)(gS[b * FF] * (xn[b * ka->x_ld] * xm[b * ka->x_ld]));
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && live) {
        const float v = (float)((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
        ka->dw[(int64_t)(n * F + m) * D + d] = v;
        ka->dw[(int64_t)(m * F + n) * D + d] = v;
    }
}

// ---- hosts ---------------------------------------------------------------------------------------------------------
static int64_t sam_up4(int64_t n) { return (n + 3) / 4 * 4; }
static int sam_fp(int F) { return (F + 15) / 16 * 16; }
static int sam_xs(int D) { return (D + 15) / 16 * 16 + 1; }
static int sam_ntri(int F) { const int nt = sam_fp(F) / 16; return nt * (nt + 1) / 2; }

// floats of one sample's LDS images, and the samples of a tile
static int sam_sample_floats(int F, int D, int type, bool bwd) {
    const int FP = sam_fp(F);
    return FP * sam_xs(D) + ((bwd && type == SAM_2E) ? 2 * FP * (FP + 1) : 0);
}

static int sam_tile_samples(int F, int D, int type, bool bwd) {
    const int s = SAM_TILE_FLOATS / sam_sample_floats(F, D, type, bwd);
    return s < 1 ? 1 : s > SAM_MAX_ST ? SAM_MAX_ST : s;
}

static size_t sam_lds_bytes(int F, int D, int type, bool bwd) {
    const int FP = sam_fp(F);
    return sizeof(float) * (4 * SAM_MAX_ST + (size_t)sam_tile_samples(F, D, type, bwd) * sam_sample_floats(F, D, type, bwd) +
                            (type == SAM_2A ? FP * (FP + 1) : 0));
}

static int64_t sam_workgroups(int64_t B, int st) {
    const int64_t tiles = fx_ceil_div(B > 0 ? B : 1, st);
    return tiles < SAM_MAX_WG ? tiles : SAM_MAX_WG;
}

static bool sam_shape_ok(int64_t B, int32_t F, int32_t D, int32_t type) {
    return B >= 0 && F >= 1 && F <= SAM_MAX_F && D >= 1 && D <= SAM_MAX_D && (type == SAM_2A || type == SAM_2E);
}

static int sam_bcol(int F, int type) { return type == SAM_2A ? sam_ntri(F) * 256 : 0; }
static int64_t sam_ldp(int F, int type) { return sam_up4(sam_bcol(F, type) + 1); }

template <auto Kernel>
static int sam_launch(const SamArgs& p, unsigned grid, size_t lds, hipStream_t s) {
    static const hipError_t lds_ok = fx_allow_lds(Kernel, SAM_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(SAM_NT), lds, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

static int sam_fill(const char* who, SamArgs& p, const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D,
                    int32_t type, bool bwd) {
    FX_CHECK_ARG(F >= 1 && F <= SAM_MAX_F, "%s: F=%d, limit 1 <= F <= %d", who, F, SAM_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= SAM_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, SAM_MAX_D);
    FX_CHECK_ARG(type == SAM_2A || type == SAM_2E, "%s: type=%d (0: SAM2A, 1: SAM2E)", who, type);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: X sample stride %lld < F*D", who, (long long)x_ld);
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B; p.F = F; p.D = D; p.type = type;
    p.FP = sam_fp(F); p.NT = p.FP / 16; p.XS = sam_xs(D); p.GS = p.FP + 1; p.KS = (D + 3) / 4; p.FK = (F + 3) / 4;
    p.DT = (D + 15) / 16; p.ST = sam_tile_samples(F, D, type, bwd); p.ntri = sam_ntri(F); p.bcol = sam_bcol(F, type);
    p.ldp = sam_ldp(F, type);
    return FX_OK;
}

// workspace: the symmetric parts first (both directions), then the backward's own
static void sam_carve(SamArgs& p, float* workspace, const float* W, const float* w) {
    const int64_t FF = (int64_t)p.F * p.F;
    p.W = W; p.w = w;
    if (p.type == SAM_2A) {
        p.gsym = workspace;
        p.part = workspace + sam_up4(FF);
        p.dgt = p.part + sam_workgroups(p.B, p.ST) * p.ldp;
    } else {
        p.wsT = workspace;
        p.wsf = p.wsT + sam_up4(FF * p.D);
        p.gS = p.wsf + sam_up4(FF * p.D);
        p.part = p.gS + sam_up4(p.B * FF);
        p.dgt = p.part + sam_workgroups(p.B, p.ST) * p.ldp;
    }
}

static int sam_prep(const SamArgs& p, hipStream_t s) {
    const int64_t total = (int64_t)p.F * p.F * (p.type == SAM_2A ? 1 : p.D);
    hipLaunchKernelGGL(k_sam_prep, dim3((unsigned)fx_ceil_div(total, SAM_NT)), dim3(SAM_NT), 0, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

static int64_t sam_layer_workspace(int64_t B, int32_t F, int32_t D, int32_t type);

extern "C" void fx_sam_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = SAM_MAX_F;
    limits[1] = SAM_MAX_D;
    limits[2] = SAM_MAX_WG;
    limits[3] = SAM_MAX_ST;
    limits[4] = 8;          // SAM_MAX_SLABS
    limits[5] = 256;        // SAM_SLAB_ROWS
}

// 2A: Gsym [F, F] | one partial row per workgroup (the tile list of dG, dbias) | their sum
// 2E: wsym [D, F, F] | wsym [F, F, D] | dlogit S [B, F, F] | the partial rows (dbias alone: 4 floats each) | 4
extern "C" int64_t fx_sam_workspace_floats(int64_t B, int32_t F, int32_t D, int32_t type) {
    if ((type == 2 || type == 3) && sam_shape_ok(B, F, D, SAM_2A)) return sam_layer_workspace(B, F, D, type);
    if (!sam_shape_ok(B, F, D, type)) return 0;
    const int64_t FF = (int64_t)F * F, ldp = sam_ldp(F, type);
    const int64_t rows = sam_workgroups(B, sam_tile_samples(F, D, type, true)) * ldp + ldp;
    if (type == SAM_2A) return sam_up4(FF) + rows;
    return 2 * sam_up4(FF * D) + sam_up4(B * FF) + rows;
}

extern "C" int fx_sam_logit_fwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, int32_t type,
                                const float* W, const float* w, const float* bias, float* logit, float* workspace,
                                fx_stream_t stream) {
    const char* who = "fx_sam_logit_fwd";
    SamArgs p;
    if (int st = sam_fill(who, p, X, x_ld, B, F, D, type, false)) return st;
    FX_CHECK_ARG(B >= 1, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(X && w && bias && logit && workspace, "%s: null X / w / bias / logit / workspace", who);
    FX_CHECK_ARG(type != SAM_2A || W, "%s: null W with SAM2A", who);
    hipStream_t s = fx_hip_stream(stream);
    sam_carve(p, workspace, W, w);                  // (the symmetric parts come first: the forward uses nothing else)
    p.bias = bias; p.logit = logit;
    if (int st = sam_prep(p, s)) return st;
    return sam_launch<k_sam_logit_fwd>(p, (unsigned)sam_workgroups(B, p.ST), sam_lds_bytes(F, D, type, false), s);
}

extern "C" int fx_sam_logit_bwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, int32_t type,
                                const float* W, const float* w, const float* dlogit, float* dX, int64_t dx_ld,
                                int32_t dx_accumulate, float* dW, float* dw, float* dbias, float* workspace,
                                fx_stream_t stream) {
    const char* who = "fx_sam_logit_bwd";
    SamArgs p;
    if (int st = sam_fill(who, p, X, x_ld, B, F, D, type, true)) return st;
    FX_CHECK_ARG(B >= 1, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(dx_ld >= (int64_t)F * D, "%s: dX sample stride %lld < F*D", who, (long long)dx_ld);
    FX_CHECK_ARG(X && w && dlogit && dX && dw && dbias && workspace,
                 "%s: null X / w / dlogit / dX / dw / dbias / workspace", who);
    FX_CHECK_ARG(type != SAM_2A || (W && dW), "%s: null W / dW with SAM2A", who);
    hipStream_t s = fx_hip_stream(stream);
    sam_carve(p, workspace, W, w);
    p.dlogit = dlogit; p.dX = dX; p.dx_ld = dx_ld; p.dx_acc = dx_accumulate ? 1 : 0; p.dW = dW; p.dw = dw;
    const int64_t wg = sam_workgroups(B, p.ST);
    if (int st = sam_prep(p, s)) return st;
    if (int st = sam_launch<k_sam_logit_bwd>(p, (unsigned)wg, sam_lds_bytes(F, D, type, true), s)) return st;
    // the tile list of dG stays in workspace (2A: bcol columns; 2E: none), dbias goes out
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, p.part, (int)wg, p.ldp, fx_rowsum_out(p.dgt, p.bcol, dbias, 1)))
        return st;
    const int64_t total = (int64_t)F * F * D;
    if (type == SAM_2A)
        hipLaunchKernelGGL(k_sam_dw2a, dim3((unsigned)fx_ceil_div(total, SAM_NT)), dim3(SAM_NT), 0, s, p);
    else
        hipLaunchKernelGGL(k_sam_dw2e, dim3((unsigned)fx_ceil_div((int64_t)F * (F + 1) / 2 * D, 64)), dim3(SAM_NT), 0, s,
                           p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ==== the stackable layers SAM3A / SAM3E (SAM.py:207-275): [B, F, D] -> [B, F, D] ===================================
//     KF = X K^T,  S = X KF^T,  out = sum_m S[n, m] W[n, m, :] (3A)  |  X (.) (S X) (3E),  (+ X Q^T with the residual)
// k_sam_layer_fwd / _bwd: one sample per workgroup iteration, grid-strided; K and Q [DP, XS] staged once per workgroup,
// X, KF and S (and dout, one [F, D] scratch in the backward) as LDS images; every product on the MFMA through sam_mm.
// A wave owns the same [F, D] tiles through a sample, so every term of dX chains into one accumulator; dK and dQ
// accumulate over all of the workgroup's samples in persistent tiles and leave as one partial row per workgroup.
// 3A's [F, F, D] operand never enters a workgroup's LDS: the layer kernel writes S_b to workspace [B, F, F] and
// k_sam_fgemm, a strided per-field GEMM on the MFMA with operands streamed from L2, takes a tile of 16 samples per
// wave: out[:, n, :] (+)= S[:, n, :] W[n] forward, dS[:, n, :] = dout[:, n, :] W[n]^T (into the same workspace; the
// layer backward reads dS_b, then writes S_b over it) and dW[n] = S[:, n, :]^T dout[:, n, :] (K = B, in at most
// SAM_MAX_SLABS batch slabs summed by fx_rowsum) backward.
#define SAM_3A 2
#define SAM_3E 3
#define SAM_MAX_SLABS 8
#define SAM_SLAB_ROWS 256

struct SamLayerArgs {
    const float* X; int64_t x_ld; int64_t B;
    int F, D, FP, NT, XS, GS, KS, FK, DT, type, res;
    const float *K, *Q;
    float* out; const float* dout;
    float* sws;                                         // S (forward), dS then S (backward) [B, F, F]
    float* dX; int64_t dx_ld; int dx_acc;
    float* part;                                        // [workgroups, 2 D D]: dK | dQ
};

struct SamGemmArgs {                                    // C[i, j] (+)= sum_k A[i ai + k ak] B[k bk + j bj] per field
    const float *A, *B; float* C;
    int64_t M, K, kper; int N, beta;
    int64_t ai, ak, an, bk, bj, bn, ci, cj, cn, cz;
};

__global__ __launch_bounds__(SAM_NT) void k_sam_fgemm(SamGemmArgs args) {
    const SamGemmArgs* ka = (const SamGemmArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int ntn = (ka->N + 15) / 16;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave, mt = tile / ntn;
    const int nt = (int)(tile - mt * ntn);
    if (mt * 16 >= ka->M) return;
    const int64_t n = blockIdx.y, k0 = (int64_t)blockIdx.z * ka->kper;
    const int64_t k1 = k0 + ka->kper < ka->K ? k0 + ka->kper : ka->K;
    const int64_t row = mt * 16 + r16;
    const int col = nt * 16 + r16;
    const float* A = ka->A + n * ka->an + row * ka->ai;
    const float* Bm = ka->B + n * ka->bn + col * ka->bj;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t k = k0 + kk; k - kk < k1; k += 4) {
        const float a = (row < ka->M && k < k1) ? A[k * ka->ak] : 0.f;
        const float b = (col < ka->N && k < k1) ? Bm[k * ka->bk] : 0.f;
        acc = sam_mfma(a, b, acc);
    }
    if (col < ka->N) {
        float* C = ka->C + blockIdx.z * ka->cz + n * ka->cn + col * ka->cj;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t r = mt * 16 + 4 * kk + i;
            if (r < ka->M) C[r * ka->ci] = acc[i] + (ka->beta ? C[r * ka->ci] : 0.f);
        }
    }
}

// [rows, D] of src (row stride D) as an LDS image [RP, XS], zeros outside
__device__ __forceinline__ void sam_stage(const float* src, int rows, int cols, int RP, int XS, float* dst) {
    for (int idx = threadIdx.x; idx < RP * XS; idx += SAM_NT) {
        const int r = idx / XS, c = idx - r * XS;
        dst[idx] = (src && r < rows && c < cols) ? src[r * cols + c] : 0.f;
    }
}

__device__ __forceinline__ void sam_put(float* dst, int stride, int mt, int nt, int r16, int kk, f32x4 v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[(16 * mt + 4 * kk + i) * stride + 16 * nt + r16] = v[i];
}

#define SAM_Z4 (f32x4{0.f, 0.f, 0.f, 0.f})

// KF = X K^T into kf, then S = X KF^T into ss (3E, or when `s_lds`) and / or to workspace (3A)
__device__ __forceinline__ void sam_kf_s(const SamLayerArgs* ka, int64_t b, const float* xs, const float* ks, float* kf,
                                         float* ss, bool to_ws, int wave, int r16, int kk) {
    const int XS = ka->XS, GS = ka->GS, F = ka->F;
    for (int t = wave; t < ka->NT * ka->DT; t += 4) {
        const int mt = t / ka->DT, nt = t - mt * ka->DT;
        sam_put(kf, XS, mt, nt, r16, kk, sam_mm(xs, XS, 1, ks, 1, XS, mt, nt, ka->KS, r16, kk, 1.f, SAM_Z4));
    }
    __syncthreads();
    for (int t = wave; t < ka->NT * ka->NT; t += 4) {
        const int mt = t / ka->NT, nt = t - mt * ka->NT;
        const f32x4 s = sam_mm(xs, XS, 1, kf, 1, XS, mt, nt, ka->KS, r16, kk, 1.f, SAM_Z4);
        if (to_ws) {
            const int m = 16 * nt + r16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = 16 * mt + 4 * kk + i;
                if (n < F && m < F) ka->sws[b * F * F + n * F + m] = s[i];
            }
        } else {
            sam_put(ss, GS, mt, nt, r16, kk, s);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(SAM_NT) void k_sam_layer_fwd(SamLayerArgs args) {
    const SamLayerArgs* ka = (const SamLayerArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) float sam_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int F = ka->F, D = ka->D, FP = ka->FP, XS = ka->XS, GS = ka->GS, DP = XS - 1;
    float* ks = sam_lds;                        // K | Q [DP, XS], X | KF [FP, XS], S [FP, GS]
    float* qs = ks + DP * XS;
    float* xs = qs + DP * XS;
    float* kf = xs + FP * XS;
    float* ss = kf + FP * XS;
    sam_stage(ka->K, D, D, DP, XS, ks);
    sam_stage(ka->res ? ka->Q : nullptr, D, D, DP, XS, qs);
    for (int64_t b = blockIdx.x; b < ka->B; b += gridDim.x) {
        __syncthreads();
        sam_stage(ka->X + b * ka->x_ld, F, D, FP, XS, xs);
        __syncthreads();
        sam_kf_s(ka, b, xs, ks, kf, ss, ka->type == SAM_3A, wave, r16, kk);
        if (ka->type == SAM_3A && !ka->res) continue;       // out = S W alone: the per-field GEMM writes it
        for (int t = wave; t < ka->NT * ka->DT; t += 4) {
            const int mt = t / ka->DT, nt = t - mt * ka->DT, d = 16 * nt + r16;
            f32x4 o = SAM_Z4;
            if (ka->res) o = sam_mm(xs, XS, 1, qs, 1, XS, mt, nt, ka->KS, r16, kk, 1.f, o);
            if (ka->type == SAM_3E) {
                const f32x4 y = sam_mm(ss, GS, 1, xs, XS, 1, mt, nt, ka->FK, r16, kk, 1.f, SAM_Z4);
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] += xs[(16 * mt + 4 * kk + i) * XS + d] * y[i];
            }
            if (d < D) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int n = 16 * mt + 4 * kk + i;
                    if (n < F) ka->out[(b * F + n) * D + d] = o[i];
                }
            }
        }
    }
}

__global__ __launch_bounds__(SAM_NT) void k_sam_layer_bwd(SamLayerArgs args) {
    const SamLayerArgs* ka = (const SamLayerArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) float sam_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int F = ka->F, D = ka->D, FP = ka->FP, XS = ka->XS, GS = ka->GS, DP = XS - 1, NT = ka->NT, DT = ka->DT;
    const bool e3 = ka->type == SAM_3E;
    float* ks = sam_lds;                        // K | Q [DP, XS], X | KF | dout | scratch [FP, XS], S / dS [FP, GS]
    float* qs = ks + DP * XS;
    float* xs = qs + DP * XS;
    float* kf = xs + FP * XS;
    float* gs = kf + FP * XS;
    float* ts = gs + FP * XS;
    float* ss = ts + FP * XS;
    sam_stage(ka->K, D, D, DP, XS, ks);
    sam_stage(ka->res ? ka->Q : nullptr, D, D, DP, XS, qs);
    f32x4 dk[4], dq[4];                         // this wave's [D, D] tiles of dK and dQ, over all its samples
#pragma unroll
    for (int j = 0; j < 4; ++j) dk[j] = dq[j] = SAM_Z4;
    for (int64_t b = blockIdx.x; b < ka->B; b += gridDim.x) {
        __syncthreads();
        sam_stage(ka->X + b * ka->x_ld, F, D, FP, XS, xs);
        sam_stage(ka->dout + b * F * D, F, D, FP, XS, gs);
        if (!e3) {                              // dS_b from the per-field GEMM
            for (int idx = threadIdx.x; idx < FP * GS; idx += SAM_NT) {
                const int n = idx / GS, m = idx - n * GS;
                ss[idx] = (n < F && m < F) ? ka->sws[b * F * F + n * F + m] : 0.f;
            }
        }
        __syncthreads();
        sam_kf_s(ka, b, xs, ks, kf, ss, !e3, wave, r16, kk);        // 3A: S_b over dS_b in workspace, for dW
        f32x4 dx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) dx[j] = SAM_Z4;
        if (e3) {
            // out = X (.) Y + R, Y = S X:  dX = dout (.) Y,  dY = dout (.) X -> scratch
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = wave + 4 * j;
                if (t < NT * DT) {
                    const int mt = t / DT, nt = t - mt * DT;
                    const f32x4 y = sam_mm(ss, GS, 1, xs, XS, 1, mt, nt, ka->FK, r16, kk, 1.f, SAM_Z4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int at = (16 * mt + 4 * kk + i) * XS + 16 * nt + r16;
                        dx[j][i] = gs[at] * y[i];
                        ts[at] = gs[at] * xs[at];
                    }
                }
            }
            __syncthreads();
            // dX += S^T dY
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = wave + 4 * j;
                if (t < NT * DT) dx[j] = sam_mm(ss, 1, GS, ts, XS, 1, t / DT, t % DT, ka->FK, r16, kk, 1.f, dx[j]);
            }
            __syncthreads();
            // dS = dY X^T over S
            for (int t = wave; t < NT * NT; t += 4)
                sam_put(ss, GS, t / NT, t % NT, r16, kk,
                        sam_mm(ts, XS, 1, xs, 1, XS, t / NT, t % NT, ka->KS, r16, kk, 1.f, SAM_Z4));
            __syncthreads();
        }
        // S = X KF^T:  dX += dS KF,  dKF = dS^T X -> scratch
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = wave + 4 * j;
            if (t < NT * DT) {
                const int mt = t / DT, nt = t - mt * DT;
                dx[j] = sam_mm(ss, GS, 1, kf, XS, 1, mt, nt, ka->FK, r16, kk, 1.f, dx[j]);
                sam_put(ts, XS, mt, nt, r16, kk, sam_mm(ss, 1, GS, xs, XS, 1, mt, nt, ka->FK, r16, kk, 1.f, SAM_Z4));
            }
        }
        __syncthreads();
        // KF = X K^T:  dX += dKF K,  dK += dKF^T X;  R = X Q^T:  dX += dout Q,  dQ += dout^T X
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = wave + 4 * j;
            if (t < NT * DT) {
                const int mt = t / DT, nt = t - mt * DT;
                dx[j] = sam_mm(ts, XS, 1, ks, XS, 1, mt, nt, ka->KS, r16, kk, 1.f, dx[j]);
                if (ka->res) dx[j] = sam_mm(gs, XS, 1, qs, XS, 1, mt, nt, ka->KS, r16, kk, 1.f, dx[j]);
                const int d = 16 * nt + r16;
                if (d < D) {
                    float* o = ka->dX + b * ka->dx_ld + d;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int n = 16 * mt + 4 * kk + i;
                        if (n < F) o[n * D] = dx[j][i] + (ka->dx_acc ? o[n * D] : 0.f);
                    }
                }
            }
            if (t < DT * DT) {
                dk[j] = sam_mm(ts, 1, XS, xs, XS, 1, t / DT, t % DT, ka->FK, r16, kk, 1.f, dk[j]);
                if (ka->res) dq[j] = sam_mm(gs, 1, XS, xs, XS, 1, t / DT, t % DT, ka->FK, r16, kk, 1.f, dq[j]);
            }
        }
    }
    float* row = ka->part + (int64_t)blockIdx.x * 2 * D * D;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wave + 4 * j;
        if (t < DT * DT) {
            const int c = 16 * (t % DT) + r16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * (t / DT) + 4 * kk + i;
                if (r < D && c < D) {
                    row[r * D + c] = dk[j][i];
                    row[D * D + r * D + c] = dq[j][i];
                }
            }
        }
    }
}

static int64_t sam_layer_wg(int64_t B) { return B < 1 ? 1 : B < SAM_MAX_WG ? B : SAM_MAX_WG; }
static int sam_slabs(int64_t B) {
    const int64_t s = fx_ceil_div(B > 0 ? B : 1, SAM_SLAB_ROWS);
    return (int)(s < SAM_MAX_SLABS ? s : SAM_MAX_SLABS);
}

static size_t sam_layer_lds(int F, int D, bool bwd) {
    const int FP = sam_fp(F), XS = sam_xs(D);
    return sizeof(float) * (size_t)(2 * (XS - 1) * XS + (bwd ? 4 : 2) * FP * XS + FP * (FP + 1));
}

static int sam_layer_fill(const char* who, SamLayerArgs& p, const float* X, int64_t x_ld, int64_t B, int32_t F,
                          int32_t D, int32_t type, const float* K, const float* Q) {
    FX_CHECK_ARG(F >= 1 && F <= SAM_MAX_F, "%s: F=%d, limit 1 <= F <= %d", who, F, SAM_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= SAM_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, SAM_MAX_D);
    FX_CHECK_ARG(type == SAM_3A || type == SAM_3E, "%s: type=%d (2: SAM3A, 3: SAM3E)", who, type);
    FX_CHECK_ARG(B >= 1, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: X sample stride %lld < F*D", who, (long long)x_ld);
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B; p.F = F; p.D = D; p.type = type; p.K = K; p.Q = Q; p.res = Q ? 1 : 0;
    p.FP = sam_fp(F); p.NT = p.FP / 16; p.XS = sam_xs(D); p.GS = p.FP + 1; p.KS = (D + 3) / 4; p.FK = (F + 3) / 4;
    p.DT = (D + 15) / 16;
    return FX_OK;
}

template <auto Kernel>
static int sam_layer_launch(const SamLayerArgs& p, size_t lds, hipStream_t s) {
    static const hipError_t lds_ok = fx_allow_lds(Kernel, SAM_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    hipLaunchKernelGGL(Kernel, dim3((unsigned)sam_layer_wg(p.B)), dim3(SAM_NT), lds, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

static int sam_fgemm(const SamGemmArgs& g, int fields, int slabs, hipStream_t s) {
    const int64_t tiles = fx_ceil_div(g.M, 16) * ((g.N + 15) / 16);
    hipLaunchKernelGGL(k_sam_fgemm, dim3((unsigned)fx_ceil_div(tiles, 4), (unsigned)fields, (unsigned)slabs),
                       dim3(SAM_NT), 0, s, g);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// 3A: S / dS [B, F, F] | 3A and 3E: one partial row [2 D D] per workgroup | 3A with more than one slab: [slabs, F F D]
static int64_t sam_layer_workspace(int64_t B, int32_t F, int32_t D, int32_t type) {
    const int64_t FF = (int64_t)F * F;
    const int slabs = sam_slabs(B);
    return (type == SAM_3A ? sam_up4(B * FF) : 0) + sam_layer_wg(B) * sam_up4(2 * D * D) +
           ((type == SAM_3A && slabs > 1) ? slabs * FF * D : 0);
}

extern "C" int fx_sam_layer_fwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, int32_t type,
                                const float* K, const float* Q, const float* W, float* out, float* workspace,
                                fx_stream_t stream) {
    const char* who = "fx_sam_layer_fwd";
    SamLayerArgs p;
    if (int st = sam_layer_fill(who, p, X, x_ld, B, F, D, type, K, Q)) return st;
    FX_CHECK_ARG(X && K && out, "%s: null X / K / out", who);
    FX_CHECK_ARG(type != SAM_3A || (W && workspace), "%s: null W / workspace with SAM3A", who);
    hipStream_t s = fx_hip_stream(stream);
    p.out = out; p.sws = workspace;
    if (int st = sam_layer_launch<k_sam_layer_fwd>(p, sam_layer_lds(F, D, false), s)) return st;
    if (type != SAM_3A) return FX_OK;
    const int64_t FF = (int64_t)F * F, FD = (int64_t)F * D;
    SamGemmArgs g = {workspace, W, out, B, F, F, D, p.res, FF, 1, F, D, 1, FD, FD, 1, D, 0};
    return sam_fgemm(g, F, 1, s);
}

extern "C" int fx_sam_layer_bwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, int32_t type,
                                const float* K, const float* Q, const float* W, const float* dout, float* dX,
                                int64_t dx_ld, int32_t dx_accumulate, float* dK, float* dQ, float* dW,
                                float* workspace, fx_stream_t stream) {
    const char* who = "fx_sam_layer_bwd";
    SamLayerArgs p;
    if (int st = sam_layer_fill(who, p, X, x_ld, B, F, D, type, K, Q)) return st;
    FX_CHECK_ARG(dx_ld >= (int64_t)F * D, "%s: dX sample stride %lld < F*D", who, (long long)dx_ld);
    FX_CHECK_ARG(X && K && dout && dX && dK && workspace, "%s: null X / K / dout / dX / dK / workspace", who);
    FX_CHECK_ARG(!Q || dQ, "%s: null dQ with the residual", who);
    FX_CHECK_ARG(type != SAM_3A || (W && dW), "%s: null W / dW with SAM3A", who);
    hipStream_t s = fx_hip_stream(stream);
    const int64_t FF = (int64_t)F * F, FD = (int64_t)F * D, wg = sam_layer_wg(B), ldp = sam_up4(2 * D * D);
    p.dout = dout; p.dX = dX; p.dx_ld = dx_ld; p.dx_acc = dx_accumulate ? 1 : 0;
    p.sws = workspace;
    p.part = workspace + (type == SAM_3A ? sam_up4(B * FF) : 0);
    float* slab = p.part + wg * ldp;
    if (type == SAM_3A) {                       // dS[b, n, m] = sum_d dout[b, n, d] W[n, m, d]
        SamGemmArgs g = {dout, W, workspace, B, D, D, F, 0, FD, 1, D, 1, D, FD, FF, 1, F, 0};
        if (int st = sam_fgemm(g, F, 1, s)) return st;
    }
    // (the kernel's rows are 2 D D floats apart; ldp only pads the region)
    if (int st = sam_layer_launch<k_sam_layer_bwd>(p, sam_layer_lds(F, D, true), s)) return st;
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, p.part, (int)wg, 2 * (int64_t)D * D,
                                                   fx_rowsum_out(dK, (int64_t)D * D, Q ? dQ : nullptr, (int64_t)D * D)))
        return st;
    if (type != SAM_3A) return FX_OK;
    const int slabs = sam_slabs(B);             // dW[n, m, d] = sum_b S[b, n, m] dout[b, n, d]
    const int64_t kper = fx_ceil_div(B, slabs);
    SamGemmArgs g = {workspace, dout, slabs > 1 ? slab : dW, F, B, kper, D, 0, 1, FF, F, FD, 1, D, D, 1, FD, FF * D};
    if (int st = sam_fgemm(g, F, slabs, s)) return st;
    if (slabs > 1) return fx_rowsum<double, FX_ROWS_SLICES>(s, slab, slabs, FF * D, fx_rowsum_out(dW, FF * D));
    return FX_OK;
}
