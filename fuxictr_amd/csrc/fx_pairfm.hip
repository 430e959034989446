// fx_pairfm.hip — the field-pair interaction of FwFM (model_zoo/FwFM/src/FwFM.py:78-88) and FmFM
// (model_zoo/FmFM/src/FmFM.py:84-91) fused over the gather record.  For a sample with fields x_0..x_{F-1} (D floats
// each) and every pair p = (i, j), i < j, in the row-major upper-triangle order of torch.triu_indices:
//     out = sum_p u_p(x_i) . x_j  (+ wlin . x)  (+ bias)  (+ addend)
//     SCALAR: u_p(x) = r_p x      W = r [P]          FwFM's interaction_weight over the inner products
//     VECTOR: u_p(x) = w_p * x    W = w [P, D]       FmFM "vectorized"
//     MATRIX: u_p(x) = x^T M_p    W = M [P, D, D]    FmFM "matrixed"
// No per-pair value is written to memory.  fp32, no atomics, every sum in a fixed order.
//
//   k_pairfm_tile<T, VEC, false> (forward) and <T, VEC, true> (the record's gradient): a workgroup owns a tile of T
//       samples (16; 8 where F * D > 2304 would not fit the LDS) and every pair for them, so out and dX are plain
//       stores.  The tile sits in LDS TRANSPOSED, xsT[c][T] (c = f * D + d): the T samples of one column are
//       contiguous, a thread reads them as 16-byte words, and all lanes that work on the same left field read the
//       same address (a broadcast).  A thread holds acc[T][VEC] in registers, i.e. VEC columns for ALL T samples of
//       the tile, so every element of W that it reads (once, from global memory: M streams past the tile through
//       L2; in SCALAR / VECTOR mode W is copied to LDS once per workgroup when it fits) is used T times.
//         forward : item = (pair p, column group e0): acc[t][k] = sum_d x_i[t][d] M_p[d][e0 + k] (MATRIX; the other
//                   modes: w x_i[t][e0 + k]), then o[t] += acc[t][k] x_j[t][e0 + k].  o[t] is summed over the wave by
//                   the butterfly, over the waves in wave order.
//         backward: ORDERED pairs, so dx_i has one owner: item = (field i, column group d0, share js of the other
//                   fields j = js, js + NS, ..): acc[t][k] = sum_{j > i} sum_e M_ij[d0 + k][e] x_j[t][e] +
//                   sum_{j < i} sum_d M_ji[d][d0 + k] x_j[t][d].  The NS shares of one element are added in the
//                   order js = 0, 1, ..: share 0 stores g (acc + wlin), share s adds to what is there, a barrier
//                   between the shares.
//   k_pairfm_dw<VEC>: the weight gradient is a reduction over the batch per pair, so here a workgroup owns a chunk
//       of 1024 gradient items (a VEC x VEC block of one dM_p; VEC elements of dw_p or dwlin; one dr_p; dbias) and a
//       slab of samples, which it stages 16 at a time (sample-major) in LDS.  Slab s writes row s of `partial`;
//       fx_colsum sums the rows in a fixed order (one slab: straight into grads, no reduce).
//   VEC = 4 (16-byte accesses of X, dX and W, 4 columns per thread) when D % 4 == 0 and every base pointer and row
//   stride is 16-byte aligned; VEC = 1 otherwise (the reference's default D = 10).
#include "fx_common.h"

#define PF_SCALAR 0
#define PF_VECTOR 1
#define PF_MATRIX 2
#define PF_NT 512                  // threads of a tile workgroup
#define PF_DW_NT 1024              // threads (= items) of a weight-gradient workgroup
#define PF_DW_ROWS 16              // samples staged at a time by k_pairfm_dw
#define PF_MAX_FD 4096
#define PF_MAX_D 64
#define PF_MAX_WG 1024
#define PF_MAX_SLABS 16
#define PF_MAX_SHARES 8
#define PF_LDS_MAX (160 * 1024)
#define PF_TILE16_FD 2304          // F * D up to which 16 samples fit: 16 * 2304 * 4 = 144 KB

struct PfArgs {
    const float* X; int64_t ldx;        // [B, F*D]
    const float* W;                     // [P] / [P, D] / [P, D, D]
    const float* wlin;                  // [F*D] or null
    const float* bias;                  // [1] or null
    const float* addend;                // [B] or null
    float* out;                         // [B]                      forward
    const float* g;                     // [B]                      backward
    float* dX; int64_t lddx;            // [B, F*D]
    float* partial; int64_t ldp;        // [slabs, ldp]
    int64_t B, nW, n;                   // floats of W; floats of grads
    int F, D, P, mode;
    int wlds;                           // floats of W copied to LDS (0: read from global memory)
    int ns;                             // shares per element of dX
    int slab_rows, has_bias;
};

// pair p -> (i, j)
__device__ __forceinline__ void pf_pair(int p, int F, int& i, int& j) {
    const float b = 2.f * (float)F - 1.f;
    int ii = (int)((b - sqrtf(fmaxf(b * b - 8.f * (float)p, 0.f))) * 0.5f);
    ii = ii < 0 ? 0 : (ii > F - 2 ? F - 2 : ii);
    while (ii > 0 && fx_pair_off(ii, F) > p) --ii;
    while (ii < F - 2 && fx_pair_off(ii + 1, F) <= p) ++ii;
    i = ii;
    j = p - fx_pair_off(ii, F) + ii + 1;
}

static inline int pf_tile(int F, int D) { return F * D <= PF_TILE16_FD ? 16 : 8; }

static inline int64_t pf_w_floats(int mode, int F, int D) {
    const int64_t P = (int64_t)F * (F - 1) / 2;
    return mode == PF_MATRIX ? P * D * D : (mode == PF_VECTOR ? P * D : P);
}

// LDS of a tile workgroup, floats: xsT [FD][T] | red [NT / 64][T] | gs [T] | W (SCALAR / VECTOR, when it fits)
static inline int64_t pf_tile_fixed(int F, int D, int T) { return (int64_t)F * D * T + (PF_NT / 64) * T + T; }
static inline int pf_wlds(int mode, int F, int D, int T) {
    if (mode == PF_MATRIX) return 0;
    const int64_t nW = pf_w_floats(mode, F, D), room = PF_LDS_MAX / 4 - pf_tile_fixed(F, D, T) - 4;
    return nW <= room ? (int)nW : 0;
}

// grid: min(tiles, PF_MAX_WG) workgroups of PF_NT threads; dynamic LDS 4 * (pf_tile_fixed + wlds rounded up to 4)
template <int T, int VEC, bool BWD>
__global__ __launch_bounds__(PF_NT) void k_pairfm_tile(PfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F, D = a.D, FD = F * D, P = a.P, mode = a.mode;
    const int NC = D / VEC;                     // column groups of a field
    float* xsT = smem;
    float* red = xsT + (int64_t)FD * T;
    float* gs = red + (PF_NT / 64) * T;
    float* wl = gs + T;
    const float* Wp = a.W;
    if (a.wlds > 0) {
        for (int e = tid; e < a.wlds; e += PF_NT) wl[e] = a.W[e];
        Wp = wl;
    }
    const int64_t tiles = (a.B + T - 1) / T;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * T;
        const int rows = a.B - b0 < T ? (int)(a.B - b0) : T;
        __syncthreads();                        // W is staged; the last tile's readers are done
        // the tile, transposed; lanes run over the samples first: conflict-free LDS stores.  Rows past B: zeros.
        for (int idx = tid; idx < NC * F * T; idx += PF_NT) {
            const int t = idx % T, c = (idx / T) * VEC;
            float v[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = 0.f;
            if (t < rows) fx_load<VEC>(a.X + (b0 + t) * a.ldx + c, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) xsT[(c + k) * T + t] = v[k];
        }
        if (BWD && tid < T) gs[tid] = tid < rows ? a.g[b0 + tid] : 0.f;
        __syncthreads();
        if (!BWD) {
            float o[T];
#pragma unroll
            for (int t = 0; t < T; ++t) o[t] = 0.f;
            const int items = P * NC;
            for (int item = tid; item < items; item += PF_NT) {
                const int p = item / NC, e0 = (item - p * NC) * VEC;
                int i, j;
                pf_pair(p, F, i, j);
                const float* xi = xsT + i * D * T;
                const float* xj = xsT + (j * D + e0) * T;
                float acc[T][VEC];
                if (mode == PF_MATRIX) {
#pragma unroll
                    for (int t = 0; t < T; ++t)
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[t][k] = 0.f;
                    const float* Mp = a.W + (int64_t)p * D * D + e0;
#pragma unroll 4
                    for (int d = 0; d < D; ++d) {
                        float m[VEC];
                        fx_load<VEC>(Mp + d * D, m);
#pragma unroll
                        for (int t4 = 0; t4 < T / 4; ++t4) {
                            const float4 x = *reinterpret_cast<const float4*>(xi + d * T + t4 * 4);
#pragma unroll
                            for (int k = 0; k < VEC; ++k) {
                                acc[t4 * 4 + 0][k] = fmaf(x.x, m[k], acc[t4 * 4 + 0][k]);
                                acc[t4 * 4 + 1][k] = fmaf(x.y, m[k], acc[t4 * 4 + 1][k]);
                                acc[t4 * 4 + 2][k] = fmaf(x.z, m[k], acc[t4 * 4 + 2][k]);
                                acc[t4 * 4 + 3][k] = fmaf(x.w, m[k], acc[t4 * 4 + 3][k]);
                            }
                        }
                    }
                } else {
                    float w[VEC];
                    if (mode == PF_VECTOR) {
                        fx_load<VEC>(Wp + (int64_t)p * D + e0, w);
                    } else {
                        const float r = Wp[p];
#pragma unroll
                        for (int k = 0; k < VEC; ++k) w[k] = r;
                    }
#pragma unroll
                    for (int k = 0; k < VEC; ++k)
#pragma unroll
                        for (int t4 = 0; t4 < T / 4; ++t4) {
                            const float4 x = *reinterpret_cast<const float4*>(xi + (e0 + k) * T + t4 * 4);
                            acc[t4 * 4 + 0][k] = w[k] * x.x;
                            acc[t4 * 4 + 1][k] = w[k] * x.y;
                            acc[t4 * 4 + 2][k] = w[k] * x.z;
                            acc[t4 * 4 + 3][k] = w[k] * x.w;
                        }
                }
#pragma unroll
                for (int k = 0; k < VEC; ++k)
#pragma unroll
                    for (int t4 = 0; t4 < T / 4; ++t4) {
                        const float4 x = *reinterpret_cast<const float4*>(xj + k * T + t4 * 4);
                        o[t4 * 4 + 0] = fmaf(acc[t4 * 4 + 0][k], x.x, o[t4 * 4 + 0]);
                        o[t4 * 4 + 1] = fmaf(acc[t4 * 4 + 1][k], x.y, o[t4 * 4 + 1]);
                        o[t4 * 4 + 2] = fmaf(acc[t4 * 4 + 2][k], x.z, o[t4 * 4 + 2]);
                        o[t4 * 4 + 3] = fmaf(acc[t4 * 4 + 3][k], x.w, o[t4 * 4 + 3]);
                    }
            }
            if (a.wlin)
                for (int c = tid; c < FD; c += PF_NT) {
                    const float w = a.wlin[c];
#pragma unroll
                    for (int t = 0; t < T; ++t) o[t] = fmaf(w, xsT[c * T + t], o[t]);
                }
            // the wave's sum by the butterfly, the waves in wave order
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float s = fx_wave_sum(o[t]);
                if (lane == t) red[wave * T + t] = s;
            }
            __syncthreads();
            if (tid < rows) {
                float s = 0.f;
                for (int w = 0; w < PF_NT / 64; ++w) s += red[w * T + tid];
                if (a.bias) s += a.bias[0];
                if (a.addend) s += a.addend[b0 + tid];
                a.out[b0 + tid] = s;
            }
        } else {
            const int NCF = F * NC, NS = a.ns;
            const int items = NS * NCF;
            for (int r0 = 0; r0 < items; r0 += PF_NT) {
                const int item = r0 + tid;
                const bool valid = item < items;
                const int js = valid ? item / NCF : 0;
                const int cg = valid ? item - js * NCF : 0;
                const int i = cg / NC, d0 = (cg - i * NC) * VEC;
                float acc[T][VEC];
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[t][k] = 0.f;
                if (valid) {
                    for (int j = js; j < F; j += NS) {
                        if (j == i) continue;
                        const int lo = j < i ? j : i, hi = j < i ? i : j;
                        const int p = fx_pair_off(lo, F) + hi - lo - 1;
                        const float* xj = xsT + j * D * T;
                        if (mode == PF_MATRIX) {
                            const float* Mp = a.W + (int64_t)p * D * D;
                            if (j > i) {
                                // sum_e M_p[d0 + k][e] x_j[t][e]
                                for (int e = 0; e < D; e += VEC) {
                                    float m[VEC][VEC];
#pragma unroll
                                    for (int k = 0; k < VEC; ++k) fx_load<VEC>(Mp + (d0 + k) * D + e, m[k]);
#pragma unroll
                                    for (int ee = 0; ee < VEC; ++ee)
#pragma unroll
                                        for (int t4 = 0; t4 < T / 4; ++t4) {
                                            const float4 x =
                                                *reinterpret_cast<const float4*>(xj + (e + ee) * T + t4 * 4);
#pragma unroll
                                            for (int k = 0; k < VEC; ++k) {
                                                acc[t4 * 4 + 0][k] = fmaf(x.x, m[k][ee], acc[t4 * 4 + 0][k]);
                                                acc[t4 * 4 + 1][k] = fmaf(x.y, m[k][ee], acc[t4 * 4 + 1][k]);
                                                acc[t4 * 4 + 2][k] = fmaf(x.z, m[k][ee], acc[t4 * 4 + 2][k]);
                                                acc[t4 * 4 + 3][k] = fmaf(x.w, m[k][ee], acc[t4 * 4 + 3][k]);
                                            }
                                        }
                                }
                            } else {
                                // sum_d M_p[d][d0 + k] x_j[t][d]
#pragma unroll 4
                                for (int d = 0; d < D; ++d) {
                                    float m[VEC];
                                    fx_load<VEC>(Mp + d * D + d0, m);
#pragma unroll
                                    for (int t4 = 0; t4 < T / 4; ++t4) {
                                        const float4 x = *reinterpret_cast<const float4*>(xj + d * T + t4 * 4);
#pragma unroll
                                        for (int k = 0; k < VEC; ++k) {
                                            acc[t4 * 4 + 0][k] = fmaf(x.x, m[k], acc[t4 * 4 + 0][k]);
                                            acc[t4 * 4 + 1][k] = fmaf(x.y, m[k], acc[t4 * 4 + 1][k]);
                                            acc[t4 * 4 + 2][k] = fmaf(x.z, m[k], acc[t4 * 4 + 2][k]);
                                            acc[t4 * 4 + 3][k] = fmaf(x.w, m[k], acc[t4 * 4 + 3][k]);
                                        }
                                    }
                                }
                            }
                        } else {
                            float w[VEC];
                            if (mode == PF_VECTOR) {
                                fx_load<VEC>(Wp + (int64_t)p * D + d0, w);
                            } else {
                                const float r = Wp[p];
#pragma unroll
                                for (int k = 0; k < VEC; ++k) w[k] = r;
                            }
#pragma unroll
                            for (int k = 0; k < VEC; ++k)
#pragma unroll
                                for (int t4 = 0; t4 < T / 4; ++t4) {
                                    const float4 x = *reinterpret_cast<const float4*>(xj + (d0 + k) * T + t4 * 4);
                                    acc[t4 * 4 + 0][k] = fmaf(w[k], x.x, acc[t4 * 4 + 0][k]);
                                    acc[t4 * 4 + 1][k] = fmaf(w[k], x.y, acc[t4 * 4 + 1][k]);
                                    acc[t4 * 4 + 2][k] = fmaf(w[k], x.z, acc[t4 * 4 + 2][k]);
                                    acc[t4 * 4 + 3][k] = fmaf(w[k], x.w, acc[t4 * 4 + 3][k]);
                                }
                        }
                    }
                }
                // the shares of an element in the order 0, 1, ..: share 0 stores, the others add to what is there
                const int c = i * D + d0;
                for (int s = 0; s < NS; ++s) {
                    if (valid && js == s) {
                        float wl4[VEC];
#pragma unroll
                        for (int k = 0; k < VEC; ++k) wl4[k] = (s == 0 && a.wlin) ? a.wlin[c + k] : 0.f;
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            if (t < rows) {
                                float* dst = a.dX + (b0 + t) * a.lddx + c;
                                float v[VEC], old[VEC];
#pragma unroll
                                for (int k = 0; k < VEC; ++k) v[k] = gs[t] * (acc[t][k] + wl4[k]);
                                if (s > 0) {
                                    fx_load<VEC>(dst, old);
#pragma unroll
                                    for (int k = 0; k < VEC; ++k) v[k] = old[k] + v[k];
                                }
                                fx_store<VEC>(dst, v);
                            }
                        }
                    }
                    if (NS > 1) __syncthreads();        // (NS, items: the same for every thread)
                }
            }
        }
    }
}

// grid: (chunks of PF_DW_NT items, slabs); dynamic LDS 4 * (PF_DW_ROWS * FDp + PF_DW_ROWS), FDp = F*D up to 4
template <int VEC>
__global__ __launch_bounds__(PF_DW_NT) void k_pairfm_dw(PfArgs a, int ts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int F = a.F, D = a.D, FD = F * D, P = a.P, mode = a.mode;
    const int FDp = (FD + 3) / 4 * 4;
    const int NC = D / VEC;
    float* xs = smem;                           // [ts][FDp]
    float* gs = smem + (int64_t)ts * FDp;       // [ts]
    // the thread's item
    const int64_t nWi = mode == PF_MATRIX ? (int64_t)P * NC * NC : (mode == PF_VECTOR ? (int64_t)P * NC : P);
    const int64_t nLi = a.wlin ? F * NC : 0;
    const int64_t item = (int64_t)blockIdx.x * PF_DW_NT + tid;
    int kind = -1;                              // 0 matrix, 1 vector, 2 scalar, 3 wlin, 4 bias
    int ci = 0, cj = 0;                         // columns of the record
    int64_t dst = 0;                            // first element in grads
    if (item < nWi) {
        int p;
        if (mode == PF_MATRIX) {
            p = (int)(item / (NC * NC));
            const int r = (int)(item - (int64_t)p * NC * NC);
            const int d0 = (r / NC) * VEC, e0 = (r % NC) * VEC;
            int i, j;
            pf_pair(p, F, i, j);
            kind = 0; ci = i * D + d0; cj = j * D + e0; dst = (int64_t)p * D * D + d0 * D + e0;
        } else if (mode == PF_VECTOR) {
            p = (int)(item / NC);
            const int d0 = (int)(item - (int64_t)p * NC) * VEC;
            int i, j;
            pf_pair(p, F, i, j);
            kind = 1; ci = i * D + d0; cj = j * D + d0; dst = (int64_t)p * D + d0;
        } else {
            p = (int)item;
            int i, j;
            pf_pair(p, F, i, j);
            kind = 2; ci = i * D; cj = j * D; dst = p;
        }
    } else if (item < nWi + nLi) {
        kind = 3; ci = (int)(item - nWi) * VEC; dst = a.nW + ci;
    } else if (item == nWi + nLi && a.has_bias) {
        kind = 4; dst = a.nW + (a.wlin ? FD : 0);
    }
    float acc[VEC][VEC];
#pragma unroll
    for (int kd = 0; kd < VEC; ++kd)
#pragma unroll
        for (int ke = 0; ke < VEC; ++ke) acc[kd][ke] = 0.f;
    const int64_t r0 = (int64_t)blockIdx.y * a.slab_rows;
    const int64_t r1 = r0 + a.slab_rows < a.B ? r0 + a.slab_rows : a.B;
    for (int64_t b0 = r0; b0 < r1; b0 += ts) {
        const int rows = r1 - b0 < ts ? (int)(r1 - b0) : ts;
        __syncthreads();
        for (int idx = tid; idx < rows * (FD / VEC); idx += PF_DW_NT) {
            const int t = idx / (FD / VEC), c = (idx - t * (FD / VEC)) * VEC;
            float v[VEC];
            fx_load<VEC>(a.X + (b0 + t) * a.ldx + c, v);
            fx_store<VEC>(xs + t * FDp + c, v);
        }
        if (tid < rows) gs[tid] = a.g[b0 + tid];
        __syncthreads();
        if (kind == 0) {
            for (int t = 0; t < rows; ++t) {
                const float gt = gs[t];
                float xi[VEC], xj[VEC];
                fx_load<VEC>(xs + t * FDp + ci, xi);
                fx_load<VEC>(xs + t * FDp + cj, xj);
#pragma unroll
                for (int kd = 0; kd < VEC; ++kd) {
                    const float gx = gt * xi[kd];
#pragma unroll
                    for (int ke = 0; ke < VEC; ++ke) acc[kd][ke] = fmaf(gx, xj[ke], acc[kd][ke]);
                }
            }
        } else if (kind == 1) {
            for (int t = 0; t < rows; ++t) {
                const float gt = gs[t];
                float xi[VEC], xj[VEC];
                fx_load<VEC>(xs + t * FDp + ci, xi);
                fx_load<VEC>(xs + t * FDp + cj, xj);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[0][k] = fmaf(gt * xi[k], xj[k], acc[0][k]);
            }
        } else if (kind == 2) {
            for (int t = 0; t < rows; ++t) {
                const float* xi = xs + t * FDp + ci;
                const float* xj = xs + t * FDp + cj;
                float dot = 0.f;
                for (int d = 0; d < D; ++d) dot = fmaf(xi[d], xj[d], dot);
                acc[0][0] = fmaf(gs[t], dot, acc[0][0]);
            }
        } else if (kind == 3) {
            for (int t = 0; t < rows; ++t) {
                float xi[VEC];
                fx_load<VEC>(xs + t * FDp + ci, xi);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[0][k] = fmaf(gs[t], xi[k], acc[0][k]);
            }
        } else if (kind == 4) {
            for (int t = 0; t < rows; ++t) acc[0][0] += gs[t];
        }
    }
    float* row = a.partial + (int64_t)blockIdx.y * a.ldp + dst;
    if (kind == 0) {
#pragma unroll
        for (int kd = 0; kd < VEC; ++kd)
#pragma unroll
            for (int ke = 0; ke < VEC; ++ke) row[kd * D + ke] = acc[kd][ke];
    } else if (kind == 1 || kind == 3) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) row[k] = acc[0][k];
    } else if (kind == 2 || kind == 4) {
        row[0] = acc[0][0];
    }
}

static int pf_check(const char* who, int32_t mode, int64_t B, int32_t F, int32_t D) {
    FX_CHECK_ARG(mode >= PF_SCALAR && mode <= PF_MATRIX, "%s: mode=%d, not 0 (scalar), 1 (vector) or 2 (matrix)", who,
                 mode);
    FX_CHECK_ARG(F >= 2, "%s: F=%d, limit F >= 2", who, F);
    FX_CHECK_ARG(D >= 1 && D <= PF_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, PF_MAX_D);
    FX_CHECK_ARG((int64_t)F * D <= PF_MAX_FD, "%s: F*D=%lld, limit %d", who, (long long)F * D, PF_MAX_FD);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    return FX_OK;
}

static inline int64_t pf_slab_rows(int64_t B) {
    const int64_t r = fx_ceil_div(fx_ceil_div(B > 0 ? B : 1, PF_MAX_SLABS), PF_DW_ROWS) * PF_DW_ROWS;
    return r;
}

static inline int pf_dw_rows(int F, int D) {
    const int FDp = (F * D + 3) / 4 * 4;
    const int fit = (PF_LDS_MAX / 4 - 64) / (FDp + 1);
    return fit < PF_DW_ROWS ? fit : PF_DW_ROWS;
}

template <bool BWD>
static int pf_launch_tile(const PfArgs& p, int T, bool vec4, hipStream_t s) {
    static const hipError_t lds_ok[4] = {
        fx_allow_lds(k_pairfm_tile<16, 4, BWD>, PF_LDS_MAX), fx_allow_lds(k_pairfm_tile<16, 1, BWD>, PF_LDS_MAX),
        fx_allow_lds(k_pairfm_tile<8, 4, BWD>, PF_LDS_MAX), fx_allow_lds(k_pairfm_tile<8, 1, BWD>, PF_LDS_MAX)};
    FX_CHECK_HIP(lds_ok[(T == 16 ? 0 : 2) + (vec4 ? 0 : 1)]);
    const size_t lds = 4 * (size_t)(pf_tile_fixed(p.F, p.D, T) + (p.wlds + 3) / 4 * 4);
    const int64_t tiles = fx_ceil_div(p.B, T);
    const dim3 grid((unsigned)(tiles < PF_MAX_WG ? tiles : PF_MAX_WG)), block(PF_NT);
    if (T == 16 && vec4) hipLaunchKernelGGL((k_pairfm_tile<16, 4, BWD>), grid, block, lds, s, p);
    else if (T == 16) hipLaunchKernelGGL((k_pairfm_tile<16, 1, BWD>), grid, block, lds, s, p);
    else if (vec4) hipLaunchKernelGGL((k_pairfm_tile<8, 4, BWD>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((k_pairfm_tile<8, 1, BWD>), grid, block, lds, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" void fx_pairfm_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = 2;                  // F at least
    limits[1] = PF_MAX_FD;          // F * D at most
    limits[2] = PF_MAX_D;
}

extern "C" int32_t fx_pairfm_tile_rows(int32_t mode, int32_t F, int32_t D) {
    (void)mode;
    if (F < 2 || D < 1) return 16;
    return pf_tile(F, D);
}

extern "C" int64_t fx_pairfm_workspace_floats(int32_t mode, int64_t B, int32_t F, int32_t D) {
    if (mode < PF_SCALAR || mode > PF_MATRIX || F < 2 || D < 1) return 0;
    const int64_t n = pf_w_floats(mode, F, D) + (int64_t)F * D + 1;
    const int64_t n4 = (n + 3) / 4 * 4;
    const int64_t slabs = fx_ceil_div(B > 0 ? B : 1, pf_slab_rows(B));
    if (slabs <= 1) return 4;
    return slabs * n4 + FX_COLSUM_CHUNKS * n4;
}

extern "C" int fx_pairfm_fwd(const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D, int32_t mode,
                             const float* W, const float* wlin, const float* bias, const float* addend, float* out,
                             fx_stream_t stream) {
    const char* who = "fx_pairfm_fwd";
    if (int st = pf_check(who, mode, B, F, D)) return st;
    FX_CHECK_ARG(ldx >= (int64_t)F * D, "%s: X row stride %lld < F*D", who, (long long)ldx);
    FX_CHECK_ARG(W, "%s: null W", who);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(X && out, "%s: null X / out", who);
    PfArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.ldx = ldx; p.W = W; p.wlin = wlin; p.bias = bias; p.addend = addend; p.out = out;
    p.B = B; p.F = F; p.D = D; p.P = F * (F - 1) / 2; p.mode = mode; p.nW = pf_w_floats(mode, F, D);
    const int T = pf_tile(F, D);
    p.wlds = pf_wlds(mode, F, D, T);
    const bool vec4 = D % 4 == 0 && fx_vec_ok(X, ldx) && fx_al16(W);
    return pf_launch_tile<false>(p, T, vec4, fx_hip_stream(stream));
}

extern "C" int fx_pairfm_bwd(const float* g, const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D,
                             int32_t mode, const float* W, const float* wlin, int32_t has_bias, float* dX,
                             int64_t lddx, float* grads, float* workspace, fx_stream_t stream) {
    const char* who = "fx_pairfm_bwd";
    if (int st = pf_check(who, mode, B, F, D)) return st;
    FX_CHECK_ARG(ldx >= (int64_t)F * D, "%s: X row stride %lld < F*D", who, (long long)ldx);
    FX_CHECK_ARG(lddx >= (int64_t)F * D, "%s: dX row stride %lld < F*D", who, (long long)lddx);
    FX_CHECK_ARG(W, "%s: null W", who);
    FX_CHECK_ARG(grads && workspace, "%s: null grads / workspace", who);
    hipStream_t s = fx_hip_stream(stream);
    const int64_t nW = pf_w_floats(mode, F, D);
    const int64_t n = nW + (wlin ? (int64_t)F * D : 0) + (has_bias ? 1 : 0);
    if (B == 0) {
        FX_CHECK_HIP(hipMemsetAsync(grads, 0, sizeof(float) * n, s));
        return FX_OK;
    }
    FX_CHECK_ARG(g && X && dX, "%s: null g / X / dX", who);
    PfArgs p;
    memset(&p, 0, sizeof(p));
    p.g = g; p.X = X; p.ldx = ldx; p.W = W; p.wlin = wlin; p.has_bias = has_bias ? 1 : 0; p.dX = dX; p.lddx = lddx;
    p.B = B; p.F = F; p.D = D; p.P = F * (F - 1) / 2; p.mode = mode; p.nW = nW; p.n = n;
    const int T = pf_tile(F, D);
    p.wlds = pf_wlds(mode, F, D, T);
    const bool vecx = D % 4 == 0 && fx_vec_ok(X, ldx) && fx_al16(W);
    const bool vec4 = vecx && fx_vec_ok(dX, lddx);
    const int NCF = F * (D / (vec4 ? 4 : 1));
    int ns = PF_NT / NCF;
    ns = ns > F - 1 ? F - 1 : ns;
    ns = ns > PF_MAX_SHARES ? PF_MAX_SHARES : ns;
    p.ns = ns < 1 ? 1 : ns;
    if (int st = pf_launch_tile<true>(p, T, vec4, s)) return st;
    // the weight gradient: chunks of items x slabs of samples
    p.slab_rows = (int)pf_slab_rows(B);
    const int64_t slabs = fx_ceil_div(B, p.slab_rows);
    const int64_t n4 = (n + 3) / 4 * 4;
    p.partial = slabs > 1 ? workspace : grads;
    p.ldp = slabs > 1 ? n4 : n;
    const int NC = D / (vecx ? 4 : 1);
    const int64_t items = (mode == PF_MATRIX ? (int64_t)p.P * NC * NC : (mode == PF_VECTOR ? (int64_t)p.P * NC : p.P)) +
                          (wlin ? F * NC : 0) + (has_bias ? 1 : 0);
    const int ts = pf_dw_rows(F, D);
    const size_t lds = 4 * ((size_t)ts * ((F * D + 3) / 4 * 4) + ts);
    static const hipError_t lds_ok[2] = {fx_allow_lds(k_pairfm_dw<4>, PF_LDS_MAX),
                                         fx_allow_lds(k_pairfm_dw<1>, PF_LDS_MAX)};
    FX_CHECK_HIP(lds_ok[vecx ? 0 : 1]);
    const dim3 grid((unsigned)fx_ceil_div(items, PF_DW_NT), (unsigned)slabs), block(PF_DW_NT);
    if (vecx) hipLaunchKernelGGL(k_pairfm_dw<4>, grid, block, lds, s, p, ts);
    else hipLaunchKernelGGL(k_pairfm_dw<1>, grid, block, lds, s, p, ts);
    FX_CHECK_LAUNCH();
    if (slabs > 1) return fx_colsum(workspace, n4, slabs, n, grads, workspace + slabs * n4, stream);
    return FX_OK;
}
