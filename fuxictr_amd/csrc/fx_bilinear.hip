// fx_bilinear.hip — FiBiNET's two layers over the fields of a sample (model_zoo/FiBiNET/src/FiBiNET.py:83-104):
//   squeeze-excitation (fuxictr/pytorch/layers/attentions/squeeze_excitation.py:51-64)
//     Z[b,f] = mean_d X[b,f,d];  A = act(W2 relu(W1 Z));  V = X * A[:,:,None]
//   bilinear interaction (fuxictr/pytorch/layers/interactions/bilinear_interaction.py:127-150), pairs p = (i, j),
//   i < j, in torch.triu_indices(F, F, 1) order
//     out[b,p,:] = ((a_i x_i) W_w(p)) * (a_j x_j),   w(p) = 0 | i | p  (field_all | field_each | field_interaction)
//   with an optional per-(sample, field) scale a = A[b,:]: the interaction of V = A * X without V in memory.
// fp32 FMAs out of LDS.  Three shapes of grid:
//   forward, dW pass : a workgroup owns PG consecutive pairs, keeps their matrices in LDS for its lifetime and
//                      walks sample tiles; the left / right vectors of a tile are gathered into LDS.  The forward
//                      stores 16 bytes per lane, consecutive lanes consecutive addresses; the dW pass keeps a
//                      4 x 4 block of one matrix' gradient per thread in registers and writes one partial per
//                      (sample slab, pair); two fixed-order launches sum them: the slabs (fx_rowsum.h's shared
//                      row sum, as for the squeeze-excitation's weights), then the pairs of a matrix.
//   dX / dA pass     : a workgroup owns a sample tile with V and dV of all fields in LDS and streams the matrices
//                      chunk by chunk (pairs of one left field): every (sample, field) sum is formed by one
//                      workgroup in a fixed order.
// No atomics anywhere: two launches on the same inputs give the same bits.
#include "fx_common.h"
#include "fx_rowsum.h"

#define BL_T 256
#define BL_MAX 64                 // F, D, R
#define BL_LDS_STATIC (64 * 1024) // what a kernel may take without asking
#define SE_LDS_MAX (96 * 1024)
#define SE_BWD_GRID 256

// ---------------------------------------------------------------------------------------------------------
// pairs
__device__ __forceinline__ int bl_left_of(int F, int p) {
    int i = 0;
    while (i + 1 < F - 1 && fx_pair_off(i + 1, F) <= p) ++i;
    return i;
}

struct BlArgs {
    const float* X; int64_t x_ld;
    int64_t B;
    int F, D, P, type;
    const float* W;
    const float* A;             // [B, F] or null
    float* out; int64_t out_ld; // (column offset already added)
    const float* dOut; int64_t dout_ld;
    float* dX; int64_t dx_ld; int dx_acc;
    float* dA;
    float* partial;             // [nslab, P, D, D]
    int PG, TB, WS;             // pairs per group / chunk, samples per tile, floats between two matrices in LDS
};

struct BlPlan {
    int PG, TB, WS, ngroups, nslab, fwd_y;
    int PGa, TBa;
    size_t lds_pg, lds_dx;
};

static inline int bl_clamp(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

static BlPlan bl_plan(int64_t B, int F, int D, bool vec4) {
    BlPlan q;
    const int P = F * (F - 1) / 2, DD = D * D;
    q.WS = DD + (vec4 ? 4 : 1);                  // matrices of neighbouring pairs start in different banks
    q.PG = bl_clamp(4096 / DD, 1, 64);
    if (q.PG > P) q.PG = P;
    q.TB = bl_clamp(2048 / (q.PG * D), 1, 16);
    q.ngroups = (int)fx_ceil_div(P, q.PG);
    const int64_t ntiles = fx_ceil_div(B > 0 ? B : 1, q.TB);
    q.nslab = bl_clamp(fx_ceil_div(1024, q.ngroups), 1, 64);
    if (q.nslab > ntiles) q.nslab = (int)ntiles;
    q.fwd_y = bl_clamp(fx_ceil_div(2048, q.ngroups), 1, 1024);
    if (q.fwd_y > ntiles) q.fwd_y = (int)ntiles;
    q.lds_pg = 4 * ((size_t)q.PG * q.WS + 2 * (size_t)q.TB * q.PG * D) + 8 * (size_t)q.PG;
    q.PGa = q.PG < F - 1 ? q.PG : F - 1;
    q.TBa = bl_clamp(4096 / (F * D), 1, 8);
    if (B > 0 && q.TBa > B) q.TBa = (int)B;
    auto lds_dx = [&]() {
        return 4 * (2 * (size_t)q.TBa * F * D + (size_t)q.PGa * q.WS + 2 * (size_t)q.TBa * q.PGa * D);
    };
    while (lds_dx() > BL_LDS_STATIC && q.PGa > 1) --q.PGa;
    while (lds_dx() > BL_LDS_STATIC && q.TBa > 1) --q.TBa;
    q.lds_dx = lds_dx();
    return q;
}

// the matrices of `npl` pairs from p0 on -> sW[pl * WS + d * D + e]; one_matrix: all of them are W[w]
template <int VEC>
__device__ __forceinline__ void bl_stage_w(const BlArgs& p, float* sW, int p0, int npl, int left, bool one_matrix) {
    const int DD = p.D * p.D, n = one_matrix ? 1 : npl;
    for (int idx = threadIdx.x * VEC; idx < n * DD; idx += BL_T * VEC) {
        const int pl = idx / DD, r = idx - pl * DD;
        const int w = p.type == 2 ? p0 + pl : (p.type == 1 ? left : 0);
        float v[VEC];
        fx_load<VEC>(p.W + (int64_t)w * DD + r, v);
        fx_store<VEC>(sW + pl * p.WS + r, v);
    }
}

// acc[k] += sum_d l[d] * W[d][c*VEC + k]
template <int VEC>
__device__ __forceinline__ void bl_row_times_w(const float* l, const float* w, int D, int c, float (&acc)[VEC]) {
    for (int d = 0; d < D; ++d) {
        const float lv = l[d];
        float wv[VEC];
        fx_load<VEC>(w + d * D + c * VEC, wv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = fmaf(lv, wv[k], acc[k]);
    }
}

// sI / sJ of a group of pairs; sL = a_i x_i, sR = (dOut *) a_j x_j of a tile of samples
template <int VEC, bool BWD>
__device__ __forceinline__ void bl_gather_tile(const BlArgs& p, int64_t b0, int nb, int p0, int npl, const int* sI,
                                               const int* sJ, float* sL, float* sR) {
    const int D = p.D, C = D / VEC;
    for (int idx = threadIdx.x; idx < nb * npl * C; idx += BL_T) {
        const int s = idx / (npl * C), r = idx - s * npl * C, pl = r / C, c = r - pl * C;
        const int64_t b = b0 + s;
        const int i = sI[pl], j = sJ[pl];
        float xl[VEC], xr[VEC];
        fx_load<VEC>(p.X + b * p.x_ld + i * D + c * VEC, xl);
        fx_load<VEC>(p.X + b * p.x_ld + j * D + c * VEC, xr);
        if (p.A != nullptr) {
            const float ai = p.A[b * p.F + i], aj = p.A[b * p.F + j];
#pragma unroll
            for (int k = 0; k < VEC; ++k) { xl[k] *= ai; xr[k] *= aj; }
        }
        if constexpr (BWD) {
            float g[VEC];
            fx_load<VEC>(p.dOut + b * p.dout_ld + (int64_t)(p0 + pl) * D + c * VEC, g);
#pragma unroll
            for (int k = 0; k < VEC; ++k) xr[k] *= g[k];
        }
        fx_store<VEC>(sL + (s * p.PG + pl) * D + c * VEC, xl);
        fx_store<VEC>(sR + (s * p.PG + pl) * D + c * VEC, xr);
    }
}

// ---------------------------------------------------------------------------------------------------------
// forward: grid (pair groups, sample splits)
template <int VEC>
__global__ __launch_bounds__(BL_T) void k_bl_fwd(BlArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int D = p.D, C = D / VEC, PG = p.PG, TB = p.TB;
    float* sW = smem;
    float* sL = sW + PG * p.WS;
    float* sR = sL + TB * PG * D;
    int* sI = reinterpret_cast<int*>(sR + TB * PG * D);
    int* sJ = sI + PG;
    const int p0 = blockIdx.x * PG;
    const int npl = p.P - p0 < PG ? p.P - p0 : PG;
    if ((int)threadIdx.x < npl) {
        const int i = bl_left_of(p.F, p0 + threadIdx.x);
        sI[threadIdx.x] = i;
        sJ[threadIdx.x] = i + 1 + (p0 + threadIdx.x - fx_pair_off(i, p.F));
    }
    __syncthreads();
    if (p.type == 2) {
        bl_stage_w<VEC>(p, sW, p0, npl, 0, false);
    } else {                                   // the group's pairs may have different left fields: one copy per pair
        const int DD = D * D;
        for (int idx = threadIdx.x * VEC; idx < npl * DD; idx += BL_T * VEC) {
            const int pl = idx / DD, r = idx - pl * DD;
            const int w = p.type == 1 ? sI[pl] : 0;
            float v[VEC];
            fx_load<VEC>(p.W + (int64_t)w * DD + r, v);
            fx_store<VEC>(sW + pl * p.WS + r, v);
        }
    }
    const int64_t ntiles = (p.B + TB - 1) / TB;
    for (int64_t t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int64_t b0 = t * TB;
        const int nb = p.B - b0 < TB ? (int)(p.B - b0) : TB;
        __syncthreads();
        bl_gather_tile<VEC, false>(p, b0, nb, p0, npl, sI, sJ, sL, sR);
        __syncthreads();
        // two samples per item share the reads of the matrix
        const int nb2 = (nb + 1) / 2;
        for (int idx = threadIdx.x; idx < nb2 * npl * C; idx += BL_T) {
            const int s2 = idx / (npl * C), r = idx - s2 * npl * C, pl = r / C, c = r - pl * C;
            const int sa = 2 * s2, sb = sa + 1 < nb ? sa + 1 : sa;
            const float* la = sL + (sa * PG + pl) * D;
            const float* lb = sL + (sb * PG + pl) * D;
            const float* w = sW + pl * p.WS;
            float ya[VEC], yb[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) ya[k] = yb[k] = 0.f;
            for (int d = 0; d < D; ++d) {
                float wv[VEC];
                fx_load<VEC>(w + d * D + c * VEC, wv);
                const float va = la[d], vb = lb[d];
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    ya[k] = fmaf(va, wv[k], ya[k]);
                    yb[k] = fmaf(vb, wv[k], yb[k]);
                }
            }
            float ra[VEC], rb[VEC];
            fx_load<VEC>(sR + (sa * PG + pl) * D + c * VEC, ra);
            fx_load<VEC>(sR + (sb * PG + pl) * D + c * VEC, rb);
#pragma unroll
            for (int k = 0; k < VEC; ++k) { ya[k] *= ra[k]; yb[k] *= rb[k]; }
            const int64_t col = (int64_t)(p0 + pl) * D + c * VEC;
            fx_store<VEC>(p.out + (b0 + sa) * p.out_ld + col, ya);
            if (sb != sa) fx_store<VEC>(p.out + (b0 + sb) * p.out_ld + col, yb);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// dW pass: grid (pair groups, sample slabs); partial[slab][pair][d][e] = sum_b (a_i x_i)[d] * (dOut a_j x_j)[e]
// VEC 4: thread = one 4 x 4 block of one pair's matrix;  VEC 1: up to 16 single entries per thread
template <int VEC>
__global__ __launch_bounds__(BL_T) void k_bl_dw(BlArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int D = p.D, DD = D * D, PG = p.PG, TB = p.TB;
    float* sL = smem + PG * p.WS;              // (the forward's layout; the matrices' room stays unused)
    float* sG = sL + TB * PG * D;
    int* sI = reinterpret_cast<int*>(sG + TB * PG * D);
    int* sJ = sI + PG;
    const int p0 = blockIdx.x * PG;
    const int npl = p.P - p0 < PG ? p.P - p0 : PG;
    if ((int)threadIdx.x < npl) {
        const int i = bl_left_of(p.F, p0 + threadIdx.x);
        sI[threadIdx.x] = i;
        sJ[threadIdx.x] = i + 1 + (p0 + threadIdx.x - fx_pair_off(i, p.F));
    }
    constexpr int NACC = 16;
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
    int offL[VEC == 4 ? 1 : NACC], offG[VEC == 4 ? 1 : NACC];
    const int C = D / VEC;
    bool live = false;
    if constexpr (VEC == 4) {
        const int blk = threadIdx.x;
        live = blk < npl * C * C;
        const int pl = live ? blk / (C * C) : 0, r = blk - pl * C * C;
        offL[0] = pl * D + (r / C) * 4;
        offG[0] = pl * D + (r % C) * 4;
    } else {
#pragma unroll
        for (int k = 0; k < NACC; ++k) {
            const int e = threadIdx.x + k * BL_T;
            const bool ok = e < npl * DD;
            const int pl = ok ? e / DD : 0, r = ok ? e - pl * DD : 0;
            offL[k] = ok ? pl * D + r / D : -1;
            offG[k] = pl * D + r % D;
        }
    }
    const int64_t ntiles = (p.B + TB - 1) / TB;
    for (int64_t t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int64_t b0 = t * TB;
        const int nb = p.B - b0 < TB ? (int)(p.B - b0) : TB;
        __syncthreads();
        bl_gather_tile<VEC, true>(p, b0, nb, p0, npl, sI, sJ, sL, sG);
        __syncthreads();
        if constexpr (VEC == 4) {
            if (live) {
                for (int s = 0; s < nb; ++s) {
                    float l[4], g[4];
                    fx_load<4>(sL + s * PG * D + offL[0], l);
                    fx_load<4>(sG + s * PG * D + offG[0], g);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[a * 4 + e] = fmaf(l[a], g[e], acc[a * 4 + e]);
                }
            }
        } else {
            for (int s = 0; s < nb; ++s) {
#pragma unroll
                for (int k = 0; k < NACC; ++k)
                    if (offL[k] >= 0) acc[k] = fmaf(sL[s * PG * D + offL[k]], sG[s * PG * D + offG[k]], acc[k]);
            }
        }
    }
    float* part = p.partial + ((int64_t)blockIdx.y * p.P + p0) * DD;
    if constexpr (VEC == 4) {
        if (live) {
            const int blk = threadIdx.x, pl = blk / (C * C), r = blk - pl * C * C, dq = r / C, eq = r % C;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float row[4] = {acc[a * 4], acc[a * 4 + 1], acc[a * 4 + 2], acc[a * 4 + 3]};
                fx_store<4>(part + (int64_t)pl * DD + (dq * 4 + a) * D + eq * 4, row);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < NACC; ++k) {
            const int e = threadIdx.x + k * BL_T;
            if (e < npl * DD) part[e] = acc[k];
        }
    }
}

// field_all / field_each: dW[w] = sum over the pairs of matrix w of perpair[p] (blockIdx.y = w), 16 slices in fp64
// (not fx_rowsum: the rows it adds are a per-matrix range of pairs, in 16 slices)
__global__ __launch_bounds__(BL_T) void k_bl_reduce_pairs(const float* perpair, int F, int P, int DD, int type,
                                                          float* dW) {
    __shared__ double red[16][16];
    const int lane = threadIdx.x & 15, slice = threadIdx.x >> 4;
    const int w = blockIdx.y;
    const int pa = type == 0 ? 0 : (w < F - 1 ? fx_pair_off(w, F) : P);
    const int pb = type == 0 ? P : (w < F - 1 ? fx_pair_off(w + 1, F) : P);
    const int o = blockIdx.x * 16 + lane;
    double s = 0.0;
    if (o < DD)
        for (int q = pa + slice; q < pb; q += 16) s += (double)perpair[(int64_t)q * DD + o];
    red[slice][lane] = s;
    __syncthreads();
    if (slice == 0 && o < DD) {
        double tot = 0.0;
        for (int k = 0; k < 16; ++k) tot += red[k][lane];
        dW[(int64_t)w * DD + o] = (float)tot;
    }
}

// ---------------------------------------------------------------------------------------------------------
// dX / dA pass: a workgroup per sample tile, V = A * X and dV of all fields in LDS
template <int VEC>
__global__ __launch_bounds__(BL_T) void k_bl_dx(BlArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = p.F, D = p.D, FD = F * D, C = D / VEC, PG = p.PG, TB = p.TB;
    float* sV = smem;
    float* sdV = sV + TB * FD;
    float* sW = sdV + TB * FD;
    float* sDY = sW + PG * p.WS;
    float* sPT = sDY + TB * PG * D;
    const int64_t ntiles = (p.B + TB - 1) / TB;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t b0 = t * TB;
        const int nb = p.B - b0 < TB ? (int)(p.B - b0) : TB;
        __syncthreads();
        for (int idx = threadIdx.x; idx < nb * F * C; idx += BL_T) {
            const int s = idx / (F * C), r = idx - s * F * C, f = r / C, c = r - f * C;
            float x[VEC], z[VEC];
            fx_load<VEC>(p.X + (b0 + s) * p.x_ld + f * D + c * VEC, x);
            const float a = p.A != nullptr ? p.A[(b0 + s) * F + f] : 1.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) { x[k] = p.A != nullptr ? x[k] * a : x[k]; z[k] = 0.f; }
            fx_store<VEC>(sV + s * FD + f * D + c * VEC, x);
            fx_store<VEC>(sdV + s * FD + f * D + c * VEC, z);
        }
        for (int i = 0; i < F - 1; ++i) {
            for (int j0 = i + 1; j0 < F; j0 += PG) {
                const int npl = F - j0 < PG ? F - j0 : PG;
                const int pbase = fx_pair_off(i, F) + (j0 - i - 1);
                const bool one = p.type != 2;
                __syncthreads();             // the last chunk's readers of sW / sPT are done; sV / sdV are written
                const bool stage = p.type == 2 || (p.type == 1 ? j0 == i + 1 : (i == 0 && j0 == 1));
                if (stage) bl_stage_w<VEC>(p, sW, pbase, npl, i, one);
                __syncthreads();
                // y = v_i W;  dv_j += g * y;  dy = g * v_j
                for (int idx = threadIdx.x; idx < nb * npl * C; idx += BL_T) {
                    const int s = idx / (npl * C), r = idx - s * npl * C, pl = r / C, c = r - pl * C;
                    const int j = j0 + pl;
                    const float* w = sW + (one ? 0 : pl * p.WS);
                    float y[VEC], g[VEC], vj[VEC], dvj[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) y[k] = 0.f;
                    bl_row_times_w<VEC>(sV + s * FD + i * D, w, D, c, y);
                    fx_load<VEC>(p.dOut + (b0 + s) * p.dout_ld + (int64_t)(pbase + pl) * D + c * VEC, g);
                    fx_load<VEC>(sV + s * FD + j * D + c * VEC, vj);
                    fx_load<VEC>(sdV + s * FD + j * D + c * VEC, dvj);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        dvj[k] = fmaf(g[k], y[k], dvj[k]);
                        vj[k] *= g[k];
                    }
                    fx_store<VEC>(sdV + s * FD + j * D + c * VEC, dvj);
                    fx_store<VEC>(sDY + (s * PG + pl) * D + c * VEC, vj);
                }
                __syncthreads();
                // this pair's share of dv_i: W dy, VEC rows of the matrix per item
                for (int idx = threadIdx.x; idx < nb * npl * C; idx += BL_T) {
                    const int s = idx / (npl * C), r = idx - s * npl * C, pl = r / C, c = r - pl * C;
                    const float* w = sW + (one ? 0 : pl * p.WS) + c * VEC * D;
                    const float* dy = sDY + (s * PG + pl) * D;
                    float part[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) part[k] = 0.f;
                    for (int e = 0; e < D; e += VEC) {
                        float dv[VEC];
                        fx_load<VEC>(dy + e, dv);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) {
                            float wv[VEC];
                            fx_load<VEC>(w + k * D + e, wv);
#pragma unroll
                            for (int m = 0; m < VEC; ++m) part[k] = fmaf(wv[m], dv[m], part[k]);
                        }
                    }
                    fx_store<VEC>(sPT + (s * PG + pl) * D + c * VEC, part);
                }
                __syncthreads();
                for (int idx = threadIdx.x; idx < nb * D; idx += BL_T) {
                    const int s = idx / D, d = idx - s * D;
                    float sum = sdV[s * FD + i * D + d];
                    for (int pl = 0; pl < npl; ++pl) sum += sPT[(s * PG + pl) * D + d];
                    sdV[s * FD + i * D + d] = sum;
                }
            }
        }
        __syncthreads();
        // dX = a * dV;  dA = dV . X
        for (int idx = threadIdx.x; idx < nb * F * C; idx += BL_T) {
            const int s = idx / (F * C), r = idx - s * F * C, f = r / C, c = r - f * C;
            float dv[VEC];
            fx_load<VEC>(sdV + s * FD + f * D + c * VEC, dv);
            if (p.A != nullptr) {
                const float a = p.A[(b0 + s) * F + f];
#pragma unroll
                for (int k = 0; k < VEC; ++k) dv[k] *= a;
            }
            float* dx = p.dX + (b0 + s) * p.dx_ld + f * D + c * VEC;
            if (p.dx_acc) {
                float old[VEC];
                fx_load<VEC>(dx, old);
#pragma unroll
                for (int k = 0; k < VEC; ++k) dv[k] += old[k];
            }
            fx_store<VEC>(dx, dv);
        }
        if (p.dA != nullptr) {
            for (int idx = threadIdx.x; idx < nb * F; idx += BL_T) {
                const int s = idx / F, f = idx - s * F;
                const float* x = p.X + (b0 + s) * p.x_ld + f * D;
                float sum = 0.f;
                for (int d = 0; d < D; ++d) sum = fmaf(sdV[s * FD + f * D + d], x[d], sum);
                p.dA[(b0 + s) * F + f] = sum;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
static int bl_check(const char* who, const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W,
                    int32_t type) {
    FX_CHECK_ARG(F >= 2 && F <= BL_MAX, "%s: F=%d, limit 2 <= F <= 64", who, F);
    FX_CHECK_ARG(D >= 1 && D <= BL_MAX, "%s: D=%d, limit 1 <= D <= 64", who, D);
    FX_CHECK_ARG(type >= 0 && type <= 2, "%s: bilinear type %d (0 field_all, 1 field_each, 2 field_interaction)", who,
                 type);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(B == 0 || (X && W), "%s: null X / W", who);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: sample stride %lld < F*D", who, (long long)x_ld);
    return FX_OK;
}

extern "C" int64_t fx_bilinear_workspace_floats(int64_t B, int32_t F, int32_t D) {
    if (F < 2 || F > BL_MAX || D < 1 || D > BL_MAX) return 0;
    const BlPlan q = bl_plan(B, F, D, D % 4 == 0);
    return (int64_t)q.nslab * (F * (F - 1) / 2) * D * D;
}

extern "C" int fx_bilinear_fwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W,
                               int32_t type, const float* A, float* out, int64_t out_ld, int64_t out_col,
                               fx_stream_t stream) {
    if (int st = bl_check("fx_bilinear_fwd", X, x_ld, B, F, D, W, type)) return st;
    const int P = F * (F - 1) / 2;
    FX_CHECK_ARG(B == 0 || out, "fx_bilinear_fwd: null out");
    FX_CHECK_ARG(out_col >= 0 && out_ld >= out_col + (int64_t)P * D,
                 "fx_bilinear_fwd: row stride %lld < column offset %lld + P*D", (long long)out_ld, (long long)out_col);
    if (B == 0) return FX_OK;
    const bool vec4 = D % 4 == 0 && out_col % 4 == 0 && fx_vec_ok(X, x_ld) && fx_al16(W) && fx_vec_ok(out, out_ld);
    const BlPlan q = bl_plan(B, F, D, vec4);
    FX_CHECK_ARG(q.lds_pg <= BL_LDS_STATIC, "fx_bilinear_fwd: %zu bytes of LDS", q.lds_pg);
    BlArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B; p.F = F; p.D = D; p.P = P; p.type = type; p.W = W; p.A = A;
    p.out = out + out_col; p.out_ld = out_ld;
    p.PG = q.PG; p.TB = q.TB; p.WS = q.WS;
    const dim3 grid((unsigned)q.ngroups, (unsigned)q.fwd_y);
    if (vec4) hipLaunchKernelGGL(k_bl_fwd<4>, grid, dim3(BL_T), q.lds_pg, fx_hip_stream(stream), p);
    else hipLaunchKernelGGL(k_bl_fwd<1>, grid, dim3(BL_T), q.lds_pg, fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_bilinear_bwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W,
                               int32_t type, const float* A, const float* dOut, int64_t dout_ld, int64_t dout_col,
                               float* dX, int64_t dx_ld, int32_t dx_accumulate, float* dA, float* dW,
                               float* workspace, fx_stream_t stream) {
    if (int st = bl_check("fx_bilinear_bwd", X, x_ld, B, F, D, W, type)) return st;
    const int P = F * (F - 1) / 2, DD = D * D;
    FX_CHECK_ARG(B > 0, "fx_bilinear_bwd: B=%lld", (long long)B);
    FX_CHECK_ARG(dOut && dX && dW && workspace, "fx_bilinear_bwd: null dOut / dX / dW / workspace");
    FX_CHECK_ARG((A == nullptr) == (dA == nullptr), "fx_bilinear_bwd: dA goes with the scale A, and only with it");
    FX_CHECK_ARG(dout_col >= 0 && dout_ld >= dout_col + (int64_t)P * D,
                 "fx_bilinear_bwd: row stride %lld < column offset %lld + P*D", (long long)dout_ld,
                 (long long)dout_col);
    FX_CHECK_ARG(dx_ld >= (int64_t)F * D, "fx_bilinear_bwd: dX sample stride %lld < F*D", (long long)dx_ld);
    const bool vec4 = D % 4 == 0 && dout_col % 4 == 0 && fx_vec_ok(X, x_ld) && fx_al16(W) &&
                      fx_vec_ok(dOut, dout_ld) && fx_vec_ok(dX, dx_ld) && fx_al16(workspace);
    const BlPlan q = bl_plan(B, F, D, vec4);
    FX_CHECK_ARG(q.lds_pg <= BL_LDS_STATIC && q.lds_dx <= BL_LDS_STATIC, "fx_bilinear_bwd: %zu / %zu bytes of LDS",
                 q.lds_pg, q.lds_dx);
    BlArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B; p.F = F; p.D = D; p.P = P; p.type = type; p.W = W; p.A = A;
    p.dOut = dOut + dout_col; p.dout_ld = dout_ld;
    p.dX = dX; p.dx_ld = dx_ld; p.dx_acc = dx_accumulate ? 1 : 0; p.dA = dA;
    p.partial = workspace;
    hipStream_t s = fx_hip_stream(stream);
    // dX (and dA): sample tiles
    BlArgs pa = p;
    pa.PG = q.PGa; pa.TB = q.TBa; pa.WS = q.WS;
    const int64_t ntiles = fx_ceil_div(B, q.TBa);
    const unsigned gx = (unsigned)(ntiles < 4096 ? ntiles : 4096);
    if (vec4) hipLaunchKernelGGL(k_bl_dx<4>, dim3(gx), dim3(BL_T), q.lds_dx, s, pa);
    else hipLaunchKernelGGL(k_bl_dx<1>, dim3(gx), dim3(BL_T), q.lds_dx, s, pa);
    FX_CHECK_LAUNCH();
    // dW: per (slab, pair) partials, then the slabs, then (field_all / field_each) the pairs of a matrix
    p.PG = q.PG; p.TB = q.TB; p.WS = q.WS;
    const dim3 grid((unsigned)q.ngroups, (unsigned)q.nslab);
    if (vec4) hipLaunchKernelGGL(k_bl_dw<4>, grid, dim3(BL_T), q.lds_pg, s, p);
    else hipLaunchKernelGGL(k_bl_dw<1>, grid, dim3(BL_T), q.lds_pg, s, p);
    FX_CHECK_LAUNCH();
    const int64_t n = (int64_t)P * DD;
    float* per_pair = type == 2 ? dW : workspace;        // (in place: entry o of slab 0 is read and written by one thread)
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, q.nslab, n, fx_rowsum_out(per_pair, n))) return st;
    if (type != 2) {
        const dim3 rg((unsigned)fx_ceil_div(DD, 16), (unsigned)(type == 0 ? 1 : F));
        hipLaunchKernelGGL(k_bl_reduce_pairs, rg, dim3(BL_T), 0, s, workspace, F, P, DD, type, dW);
        FX_CHECK_LAUNCH();
    }
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// squeeze-excitation: a wave per sample, four samples per workgroup and round; lane f / r = field / hidden unit
struct SeArgs {
    const float* X; int64_t x_ld;
    int64_t B;
    int F, D, R, act;           // act: 0 ReLU, 1 Sigmoid
    const float* W1;            // [R, F]
    const float* W2;            // [F, R]
    float* A;                   // fwd: out [B, F]; bwd: the forward's A
    float* V;                   // [B, F, D] contiguous or null
    const float* dA;
    const float* dV;
    float* dX; int64_t dx_ld; int dx_acc;
    float* partial;             // [grid, 2, F * R]: dW1 | dW2
};

#define SE_WAVES 4

__device__ __forceinline__ void se_stage_w(const SeArgs& p, float* sW1, float* sW2) {
    const int F = p.F, R = p.R, FS = F | 1, RS = R | 1;
    for (int idx = threadIdx.x; idx < F * R; idx += BL_T) {
        sW1[(idx / F) * FS + idx % F] = p.W1[idx];
        sW2[(idx / R) * RS + idx % R] = p.W2[idx];
    }
}

// Z, H = relu(W1 Z) and the pre-activation of A of this wave's sample: one instruction sequence for both directions
__device__ __forceinline__ float se_forward(const SeArgs& p, const float* sW1, const float* sW2, const float* x,
                                            bool valid, float* sZ, float* sH) {
    const int lane = threadIdx.x & 63, F = p.F, D = p.D, R = p.R, FS = F | 1, RS = R | 1;
    if (lane < F) {
        float s = 0.f;
        if (valid)
            for (int d = 0; d < D; ++d) s += x[lane * D + d];
        sZ[lane] = s / (float)D;
    }
    __syncthreads();
    if (lane < R) {
        float h = 0.f;
        for (int f = 0; f < F; ++f) h = fmaf(sW1[lane * FS + f], sZ[f], h);
        sH[lane] = fmaxf(h, 0.f);
    }
    __syncthreads();
    float a = 0.f;
    if (lane < F)
        for (int r = 0; r < R; ++r) a = fmaf(sW2[lane * RS + r], sH[r], a);
    return a;
}

__global__ __launch_bounds__(BL_T) void k_senet_fwd(SeArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = p.F, D = p.D, R = p.R, FS = F | 1, RS = R | 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* sW1 = smem;
    float* sW2 = sW1 + R * FS;
    float* sZ = sW2 + F * RS + wave * 3 * 64;
    float* sH = sZ + 64;
    float* sA = sH + 64;
    se_stage_w(p, sW1, sW2);
    const int64_t rounds = (p.B + SE_WAVES - 1) / SE_WAVES;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t b = rd * SE_WAVES + wave;
        const bool valid = b < p.B;
        const float* x = p.X + (valid ? b : 0) * p.x_ld;
        __syncthreads();
        float a = se_forward(p, sW1, sW2, x, valid, sZ, sH);
        a = p.act == 0 ? fmaxf(a, 0.f) : 1.f / (1.f + expf(-a));
        if (lane < F) {
            sA[lane] = a;
            if (valid) p.A[b * F + lane] = a;
        }
        if (p.V != nullptr) {
            __syncthreads();
            if (valid)
                for (int idx = lane; idx < F * D; idx += 64) p.V[b * F * D + idx] = x[idx] * sA[idx / D];
        }
    }
}

__global__ __launch_bounds__(BL_T) void k_senet_bwd(SeArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = p.F, D = p.D, R = p.R, FS = F | 1, RS = R | 1, FR = F * R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* sW1 = smem;
    float* sW2 = sW1 + R * FS;
    float* sAcc = sW2 + F * RS;                 // dW1 [R][F] | dW2 [F][R] of this workgroup's samples
    float* sAll = sAcc + 2 * FR;                // per wave: Z, H, GA, GH, GZ, A
    float* sZ = sAll + wave * 6 * 64;
    float* sH = sZ + 64;
    float* sGA = sH + 64;
    float* sGH = sGA + 64;
    float* sGZ = sGH + 64;
    float* sA = sGZ + 64;
    se_stage_w(p, sW1, sW2);
    for (int idx = threadIdx.x; idx < 2 * FR; idx += BL_T) sAcc[idx] = 0.f;
    const int64_t rounds = (p.B + SE_WAVES - 1) / SE_WAVES;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t b = rd * SE_WAVES + wave;
        const bool valid = b < p.B;
        const float* x = p.X + (valid ? b : 0) * p.x_ld;
        __syncthreads();
        se_forward(p, sW1, sW2, x, valid, sZ, sH);      // (A itself is the forward's: the mask and the sigmoid's slope)
        if (lane < F) {
            float ga = 0.f, a = 0.f;
            if (valid) {
                a = p.A[b * F + lane];
                if (p.dA != nullptr) ga = p.dA[b * F + lane];
                if (p.dV != nullptr) {
                    const float* dv = p.dV + b * F * D + lane * D;
                    float s = 0.f;
                    for (int d = 0; d < D; ++d) s = fmaf(dv[d], x[lane * D + d], s);
                    ga += s;
                }
                ga = p.act == 0 ? (a > 0.f ? ga : 0.f) : ga * a * (1.f - a);
            }
            sGA[lane] = ga;
            sA[lane] = a;
        }
        __syncthreads();
        if (lane < R) {
            float gh = 0.f;
            for (int f = 0; f < F; ++f) gh = fmaf(sW2[f * RS + lane], sGA[f], gh);
            sGH[lane] = (valid && sH[lane] > 0.f) ? gh : 0.f;
        }
        __syncthreads();
        if (lane < F) {
            float gz = 0.f;
            for (int r = 0; r < R; ++r) gz = fmaf(sW1[r * FS + lane], sGH[r], gz);
            sGZ[lane] = gz / (float)D;
        }
        __syncthreads();
        if (valid) {
            for (int idx = lane; idx < F * D; idx += 64) {
                const int f = idx / D;
                float g = sGZ[f];
                if (p.dV != nullptr) g = fmaf(p.dV[b * F * D + idx], sA[f], g);
                float* dx = p.dX + b * p.dx_ld + idx;
                *dx = p.dx_acc ? *dx + g : g;
            }
        }
        // the weight gradients of the round's four samples, wave 0 .. 3 in order (an absent sample adds zeros)
        for (int idx = threadIdx.x; idx < FR; idx += BL_T) {
            const int r1 = idx / F, f1 = idx - r1 * F;      // dW1[r][f] += gh[r] z[f]
            const int f2 = idx / R, r2 = idx - f2 * R;      // dW2[f][r] += ga[f] h[r]
            float t1 = 0.f, t2 = 0.f;
            for (int w = 0; w < SE_WAVES; ++w) {
                const float* q = sAll + w * 6 * 64;
                t1 = fmaf(q[3 * 64 + r1], q[f1], t1);
                t2 = fmaf(q[2 * 64 + f2], q[64 + r2], t2);
            }
            sAcc[idx] += t1;
            sAcc[FR + idx] += t2;
        }
    }
    __syncthreads();
    float* part = p.partial + (int64_t)blockIdx.x * 2 * FR;
    for (int idx = threadIdx.x; idx < 2 * FR; idx += BL_T) part[idx] = sAcc[idx];
}

static size_t se_lds_bytes(int F, int R, bool bwd) {
    size_t n = (size_t)R * (F | 1) + (size_t)F * (R | 1);
    n += bwd ? 2 * (size_t)F * R + SE_WAVES * 6 * 64 : SE_WAVES * 3 * 64;
    return 4 * n;
}

static int se_check(const char* who, const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W1,
                    const float* W2, int32_t R, int32_t act) {
    FX_CHECK_ARG(F >= 1 && F <= BL_MAX, "%s: F=%d, limit 1 <= F <= 64", who, F);
    FX_CHECK_ARG(D >= 1 && D <= BL_MAX, "%s: D=%d, limit 1 <= D <= 64", who, D);
    FX_CHECK_ARG(R >= 1 && R <= BL_MAX, "%s: R=%d, limit 1 <= R <= 64", who, R);
    FX_CHECK_ARG(act == 0 || act == 1, "%s: activation %d (0 ReLU, 1 Sigmoid)", who, act);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(B == 0 || (X && W1 && W2), "%s: null X / W1 / W2", who);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: sample stride %lld < F*D", who, (long long)x_ld);
    return FX_OK;
}

static unsigned se_bwd_grid(int64_t B) {
    const int64_t rounds = fx_ceil_div(B > 0 ? B : 1, SE_WAVES);
    return (unsigned)(rounds < SE_BWD_GRID ? rounds : SE_BWD_GRID);
}

extern "C" int64_t fx_senet_workspace_floats(int64_t B, int32_t F, int32_t R) {
    return (int64_t)se_bwd_grid(B) * 2 * F * R;
}

extern "C" int fx_senet_fwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W1,
                            const float* W2, int32_t R, int32_t act, float* A, float* V, fx_stream_t stream) {
    if (int st = se_check("fx_senet_fwd", X, x_ld, B, F, D, W1, W2, R, act)) return st;
    FX_CHECK_ARG(B == 0 || A, "fx_senet_fwd: null A");
    if (B == 0) return FX_OK;
    SeArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B; p.F = F; p.D = D; p.R = R; p.act = act; p.W1 = W1; p.W2 = W2;
    p.A = A; p.V = V;
    const size_t lds = se_lds_bytes(F, R, false);
    FX_CHECK_ARG(lds <= BL_LDS_STATIC, "fx_senet_fwd: %zu bytes of LDS", lds);
    const int64_t rounds = fx_ceil_div(B, SE_WAVES);
    const unsigned grid = (unsigned)(rounds < 1024 ? rounds : 1024);
    hipLaunchKernelGGL(k_senet_fwd, dim3(grid), dim3(BL_T), lds, fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_senet_bwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* W1,
                            const float* W2, int32_t R, int32_t act, const float* A, const float* dA,
                            const float* dV, float* dX, int64_t dx_ld, int32_t dx_accumulate, float* dW1,
                            float* dW2, float* workspace, fx_stream_t stream) {
    if (int st = se_check("fx_senet_bwd", X, x_ld, B, F, D, W1, W2, R, act)) return st;
    FX_CHECK_ARG(B > 0, "fx_senet_bwd: B=%lld", (long long)B);
    FX_CHECK_ARG(A && dX && dW1 && dW2 && workspace, "fx_senet_bwd: null A / dX / dW1 / dW2 / workspace");
    FX_CHECK_ARG(dA || dV, "fx_senet_bwd: neither dA nor dV");
    FX_CHECK_ARG(dx_ld >= (int64_t)F * D, "fx_senet_bwd: dX sample stride %lld < F*D", (long long)dx_ld);
    SeArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B; p.F = F; p.D = D; p.R = R; p.act = act; p.W1 = W1; p.W2 = W2;
    p.A = const_cast<float*>(A); p.dA = dA; p.dV = dV;
    p.dX = dX; p.dx_ld = dx_ld; p.dx_acc = dx_accumulate ? 1 : 0;
    p.partial = workspace;
    const size_t lds = se_lds_bytes(F, R, true);
    FX_CHECK_ARG(lds <= SE_LDS_MAX, "fx_senet_bwd: %zu bytes of LDS", lds);
    // (dynamic LDS above 64 KiB has to be allowed per kernel: asked for once)
    static const hipError_t lds_ok = fx_allow_lds(k_senet_bwd, SE_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    const unsigned grid = se_bwd_grid(B);
    hipStream_t s = fx_hip_stream(stream);
    hipLaunchKernelGGL(k_senet_bwd, dim3(grid), dim3(BL_T), lds, s, p);
    FX_CHECK_LAUNCH();
    const int FR = F * R;
    // partial[g] = [dW1 | dW2], rows 2 FR floats apart: one sum over the workgroups for each half
    if (int st = fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)grid, 2 * FR, fx_rowsum_out(dW1, FR))) return st;
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace + FR, (int)grid, 2 * FR, fx_rowsum_out(dW2, FR));
}
