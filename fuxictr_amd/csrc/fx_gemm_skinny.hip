// fx_gemm_skinny.hip — the bandwidth-bound GEMM kernels for skinny shapes (K <= 8, N <= 4, M <= 4) and the
// fused backward of a Linear(hidden -> 1) head, with their host launchers (fx_gemm_int.h:
// fx_gemm_skinny_launch, fx_head_bwd_launch).
#include "fx_common.h"
#include "fx_gemm_int.h"

// ---------------------------------------------------------------------------------------------
// Skinny shapes.  Every CTR tower ends in Linear(hidden -> 1): its forward (N = 1), weight
// gradient (M = 1) and input gradient (K = 1) would each occupy a full 128-wide MFMA tile per
// block for one useful row/column, so they run as bandwidth-bound kernels instead.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float fx_a_at(const GemmArgs& a, int ta, int64_t m, int64_t k) {
    return ta ? a.A[k * a.lda + m] : a.A[m * a.lda + k];
}
__device__ __forceinline__ float fx_b_at(const GemmArgs& a, int tb, int64_t k, int64_t n) {
    return tb ? a.B[n * a.ldb + k] : a.B[k * a.ldb + n];
}

// K <= 8: one thread per output element
__global__ __launch_bounds__(256) void k_gemm_small_k(GemmArgs a, int ta, int tb) {
    const int64_t total = a.M * a.N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / a.N, n = i - m * a.N;
        float acc = 0.f;
        for (int64_t k = 0; k < a.K; ++k) acc = fmaf(fx_a_at(a, ta, m, k), fx_b_at(a, tb, k, n), acc);
        a.C[m * a.ldc + n] = fx_epilogue(a.epi, acc, m, n);
    }
}

// K <= 8 with 4 | N (the input gradient of a Linear(hidden -> 1) head: an outer product that writes
// M x N floats and reads the same amount of ReLU mask): one thread per 4 output columns, 16-byte stores,
// no 64-bit division per element.  Pure HBM stream.
__global__ __launch_bounds__(256) void k_gemm_small_k_v4(GemmArgs a, int ta, int tb) {
    const uint32_t n4 = (uint32_t)(a.N >> 2);
    const uint32_t total = (uint32_t)(a.M * n4);              // < 2^31 (checked by the launcher)
    const fx_gemm_epilogue& e = a.epi;
    // the tower case: nothing but the ReLU mask of the layer below -> one 16-byte mask load
    const bool mask_only = e.mask && !e.bias && !e.zout && e.act == 0 && !e.mul && !e.add &&
                           (e.ldmask & 3) == 0 && (reinterpret_cast<uintptr_t>(e.mask) & 15) == 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t mi = i / n4;
        const int64_t m = mi, n = (int64_t)(i - mi * n4) << 2;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int64_t k = 0; k < a.K; ++k) {
            const float x = fx_a_at(a, ta, m, k);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(x, fx_b_at(a, tb, k, n + c), acc[c]);
        }
        float4 o;
        if (mask_only) {
            const float4 mk = *reinterpret_cast<const float4*>(e.mask + m * e.ldmask + n);
            o.x = mk.x > 0.f ? acc[0] : 0.f;
            o.y = mk.y > 0.f ? acc[1] : 0.f;
            o.z = mk.z > 0.f ? acc[2] : 0.f;
            o.w = mk.w > 0.f ? acc[3] : 0.f;
        } else {
            o.x = fx_epilogue(e, acc[0], m, n);
            o.y = fx_epilogue(e, acc[1], m, n + 1);
            o.z = fx_epilogue(e, acc[2], m, n + 2);
            o.w = fx_epilogue(e, acc[3], m, n + 3);
        }
        *reinterpret_cast<float4*>(a.C + m * a.ldc + n) = o;
    }
}

// N <= 4, A [M,K] and B [N,K] k-contiguous, 4 | K, any K: one wave per output row, a lane takes a float4
// every 256 floats, four loads in flight per lane (the scalar kernel below issues one dependent 4-byte
// load per iteration: 1.7 TB/s on the 4096 x 1024 head of the towers)
__global__ __launch_bounds__(256) void k_gemm_small_n_wide(GemmArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); m < a.M; m += waves) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* arow = a.A + m * a.lda;
        int64_t k = (int64_t)lane * 4;
        for (; k + 768 < a.K; k += 1024) {
            float4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const float4*>(arow + k + 256 * u);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    if (n < a.N) {
                        const float4 w = *reinterpret_cast<const float4*>(a.B + n * a.ldb + k + 256 * u);
                        acc[n] = fmaf(x[u].x, w.x, acc[n]);
                        acc[n] = fmaf(x[u].y, w.y, acc[n]);
                        acc[n] = fmaf(x[u].z, w.z, acc[n]);
                        acc[n] = fmaf(x[u].w, w.w, acc[n]);
                    }
        }
        for (; k < a.K; k += 256) {
            const float4 x = *reinterpret_cast<const float4*>(arow + k);
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (n < a.N) {
                    const float4 w = *reinterpret_cast<const float4*>(a.B + n * a.ldb + k);
                    acc[n] = fmaf(x.x, w.x, acc[n]);
                    acc[n] = fmaf(x.y, w.y, acc[n]);
                    acc[n] = fmaf(x.z, w.z, acc[n]);
                    acc[n] = fmaf(x.w, w.w, acc[n]);
                }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = fx_wave_sum(acc[n]);
        if (lane == 0)
            for (int n = 0; n < a.N; ++n) a.C[m * a.ldc + n] = fx_epilogue(a.epi, acc[n], m, n);
    }
}

// N <= 4, A stored [M,K]: one wave per output row, lanes stride k (coalesced), xor reduction
__global__ __launch_bounds__(256) void k_gemm_small_n(GemmArgs a, int tb) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); m < a.M; m += waves) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* arow = a.A + m * a.lda;
        for (int64_t k = lane; k < a.K; k += 64) {
            const float x = arow[k];
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (n < a.N) acc[n] = fmaf(x, fx_b_at(a, tb, k, n), acc[n]);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = fx_wave_sum(acc[n]);
        if (lane == 0)
            for (int n = 0; n < a.N; ++n) a.C[m * a.ldc + n] = fx_epilogue(a.epi, acc[n], m, n);
    }
}

// M <= 4, A stored [K,M], B stored [K,N]: Np = min(256, pow2 >= N) column lanes x 256/Np row lanes
// per workgroup, K split over blockIdx.y into workspace slabs (reduced, with the epilogue, by
// k_splitk_reduce).  Narrow outputs (the 64 -> 1 head of the DIN attention MLP has N = 64 and
// K = B*L = 204800) keep all 256 lanes busy through the row lanes.
// fused bias gradient of the skinny weight-gradient kernels (M <= 4): slab z's sum of column m of
// A over [kbeg, kend).  All 256 threads of the block take part (a single thread per row made the
// k_chunk loads one dependent chain: 40 us for a 400-deep chunk); fixed LDS tree.
__device__ __forceinline__ void fx_small_m_rowsum(const GemmArgs& a, int z, int64_t kbeg,
                                                  int64_t kend) {
    __shared__ float rs[256];
    for (int m = 0; m < (int)a.M; ++m) {            // block-uniform (M <= 4)
        float r = 0.f;
        for (int64_t k = kbeg + threadIdx.x; k < kend; k += 256) r += a.A[k * a.lda + m];
        rs[threadIdx.x] = r;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) rs[threadIdx.x] += rs[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0)
            a.ws[(int64_t)a.split_k * a.M * a.N + (int64_t)z * a.M + m] = rs[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_gemm_small_m(GemmArgs a, int np_log2) {
    __shared__ float red[4][256];
    const int Np = 1 << np_log2;
    const int tx = threadIdx.x & (Np - 1), ty = threadIdx.x >> np_log2;
    const int lanes = 256 >> np_log2;
    const int64_t n = (int64_t)blockIdx.x * Np + tx;
    const int z = blockIdx.y;
    const int64_t kbeg = (int64_t)z * a.k_chunk;
    const int64_t kend = (kbeg + a.k_chunk < a.K) ? kbeg + a.k_chunk : a.K;
    if (a.epi.rowsum && blockIdx.x == 0) fx_small_m_rowsum(a, z, kbeg, kend);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < a.N) {
        for (int64_t k = kbeg + ty; k < kend; k += lanes) {
            const float b = a.B[k * a.ldb + n];
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < a.M) acc[m] = fmaf(a.A[k * a.lda + m], b, acc[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) red[m][threadIdx.x] = acc[m];
    __syncthreads();
    for (int s2 = lanes >> 1; s2 > 0; s2 >>= 1) {
        if (ty < s2) {
#pragma unroll
            for (int m = 0; m < 4; ++m) red[m][threadIdx.x] += red[m][threadIdx.x + (s2 << np_log2)];
        }
        __syncthreads();
    }
    if (ty == 0 && n < a.N)
        for (int m = 0; m < a.M; ++m) a.ws[((int64_t)z * a.M + m) * a.N + n] = red[m][tx];
}

// vectorised M <= 4 variant (N % 4 == 0, 16-B aligned B rows): CG float4 column groups x 256/CG
// row lanes per workgroup (CG = 64 for N >= 256, fewer for narrow outputs such as the 64-wide DIN
// attention layer, K = B*L = 204800), two rows in flight per lane, LDS combine of the row lanes
template <int CG_LOG2>
__global__ __launch_bounds__(256) void k_gemm_small_m_v4(GemmArgs a) {
    constexpr int CG = 1 << CG_LOG2, RL = 256 / CG;
    __shared__ float4 red[4][256];
    const int tx = threadIdx.x & (CG - 1), ty = threadIdx.x >> CG_LOG2;
    const int64_t n = ((int64_t)blockIdx.x * CG + tx) * 4;
    const int z = blockIdx.y;
    const int64_t kbeg = (int64_t)z * a.k_chunk;
    const int64_t kend = (kbeg + a.k_chunk < a.K) ? kbeg + a.k_chunk : a.K;
    if (a.epi.rowsum && blockIdx.x == 0) fx_small_m_rowsum(a, z, kbeg, kend);
    float4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fma_row = [&](const float4& b, int64_t k) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (m < a.M) {
                const float w = a.A[k * a.lda + m];
                acc[m].x = fmaf(w, b.x, acc[m].x);
                acc[m].y = fmaf(w, b.y, acc[m].y);
                acc[m].z = fmaf(w, b.z, acc[m].z);
                acc[m].w = fmaf(w, b.w, acc[m].w);
            }
        }
    };
    if (n < a.N) {
        int64_t k = kbeg + ty;
        for (; k + RL < kend; k += 2 * RL) {
            const float4 b0 = *reinterpret_cast<const float4*>(a.B + k * a.ldb + n);
            const float4 b1 = *reinterpret_cast<const float4*>(a.B + (k + RL) * a.ldb + n);
            fma_row(b0, k);
            fma_row(b1, k + RL);
        }
        for (; k < kend; k += RL) {
            const float4 b0 = *reinterpret_cast<const float4*>(a.B + k * a.ldb + n);
            fma_row(b0, k);
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) red[m][threadIdx.x] = acc[m];
    __syncthreads();
    if (ty == 0 && n < a.N) {
        for (int m = 0; m < a.M; ++m) {
            float4 r = red[m][tx];
            for (int y = 1; y < RL; ++y) {          // fixed order over the row lanes
                const float4 q = red[m][tx + y * CG];
                r.x += q.x;
                r.y += q.y;
                r.z += q.z;
                r.w += q.w;
            }
            *reinterpret_cast<float4*>(a.ws + ((int64_t)z * a.M + m) * a.N + n) = r;
        }
    }
}

// Backward of a Linear(hidden -> 1) head in ONE pass over the hidden activations: the weight gradient
// dW[1, N] = sum_k dz[k] x[k, :] (k_gemm_small_m_v4 with M = 1: same loop, same slab order -> same bits)
// and the input gradient dX[k, :] = dz[k] W[:] with the ReLU mask x[k, :] > 0 — x IS the mask, so the
// row that was just loaded for dW also decides and the product leaves as one 16-byte store.  Two
// launches (k_gemm_small_m_v4 + k_gemm_small_k_v4: x streamed twice) become one.

template <int CG_LOG2>
__global__ __launch_bounds__(256) void k_head_bwd_v4(HeadBwdArgs h) {
    const GemmArgs& a = h.dw;
    constexpr int CG = 1 << CG_LOG2, RL = 256 / CG;
    __shared__ float4 red[256];
    const int tx = threadIdx.x & (CG - 1), ty = threadIdx.x >> CG_LOG2;
    const int64_t n = ((int64_t)blockIdx.x * CG + tx) * 4;
    const int z = blockIdx.y;
    const int64_t kbeg = (int64_t)z * a.k_chunk;
    const int64_t kend = (kbeg + a.k_chunk < a.K) ? kbeg + a.k_chunk : a.K;
    if (a.epi.rowsum && blockIdx.x == 0) fx_small_m_rowsum(a, z, kbeg, kend);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < a.N) {
        const float4 wv = *reinterpret_cast<const float4*>(h.w + n);
        const bool um = h.use_mask != 0;
        auto row = [&](const float4& b, int64_t k) {
            const float d = a.A[k * a.lda];
            acc.x = fmaf(d, b.x, acc.x);
            acc.y = fmaf(d, b.y, acc.y);
            acc.z = fmaf(d, b.z, acc.z);
            acc.w = fmaf(d, b.w, acc.w);
            float4 o = make_float4(d * wv.x, d * wv.y, d * wv.z, d * wv.w);
            if (um) {
                o.x = b.x > 0.f ? o.x : 0.f;
                o.y = b.y > 0.f ? o.y : 0.f;
                o.z = b.z > 0.f ? o.z : 0.f;
                o.w = b.w > 0.f ? o.w : 0.f;
            }
            *reinterpret_cast<float4*>(h.dx + k * h.ldx + n) = o;
        };
        int64_t k = kbeg + ty;
        for (; k + RL < kend; k += 2 * RL) {
            const float4 b0 = *reinterpret_cast<const float4*>(a.B + k * a.ldb + n);
            const float4 b1 = *reinterpret_cast<const float4*>(a.B + (k + RL) * a.ldb + n);
            row(b0, k);
            row(b1, k + RL);
        }
        for (; k < kend; k += RL) {
            const float4 b0 = *reinterpret_cast<const float4*>(a.B + k * a.ldb + n);
            row(b0, k);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (ty == 0 && n < a.N) {
        float4 r = red[tx];
        for (int y = 1; y < RL; ++y) {          // fixed order over the row lanes
            const float4 q = red[tx + y * CG];
            r.x += q.x;
            r.y += q.y;
            r.z += q.z;
            r.w += q.w;
        }
        *reinterpret_cast<float4*>(a.ws + (int64_t)z * a.N + n) = r;
    }
}

// N <= 4, A stored [M,K] with K <= 256, K % 4 == 0, 16-B aligned rows (the 64 -> 1 attention output
// layer over B*L rows): K/4 lanes read one row as float4s, 64/(K/4) rows per wave instruction
template <int LPR_LOG2>
__global__ __launch_bounds__(256) void k_gemm_small_n_v4(GemmArgs a, int tb) {
    constexpr int LPR = 1 << LPR_LOG2, RPW = 64 / LPR;     // lanes per row, rows per wave
    const int lane = threadIdx.x & 63;
    const int sub = lane & (LPR - 1), rw = lane >> LPR_LOG2;
    const int kq = sub * 4;
    float4 w[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        w[n] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < a.N && kq < a.K) {
            w[n].x = fx_b_at(a, tb, kq + 0, n);
            w[n].y = fx_b_at(a, tb, kq + 1, n);
            w[n].z = fx_b_at(a, tb, kq + 2, n);
            w[n].w = fx_b_at(a, tb, kq + 3, n);
        }
    }
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t m0 = wave * RPW; m0 < a.M; m0 += waves * RPW) {
        const int64_t m = m0 + rw;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < a.M && kq < a.K) x = *reinterpret_cast<const float4*>(a.A + m * a.lda + kq);
        float acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            acc[n] = fmaf(x.w, w[n].w, fmaf(x.z, w[n].z, fmaf(x.y, w[n].y, x.x * w[n].x)));
#pragma unroll
            for (int off = LPR >> 1; off > 0; off >>= 1) acc[n] += __shfl_xor(acc[n], off, 64);
        }
        if (sub == 0 && m < a.M)
            for (int n = 0; n < a.N; ++n) a.C[m * a.ldc + n] = fx_epilogue(a.epi, acc[n], m, n);
    }
}

// ---- host launchers -----------------------------------------------------------------------------------
// KERNEL<v> for v = 2 .. 6 (anything else: 6) / v = 0 .. 6
#define FX_LAUNCH_LOG2_FROM2(KERNEL, v, ...)                          \
    switch (v) {                                                      \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;    \
        case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;    \
        case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;    \
        case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;    \
        default: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;   \
    }
#define FX_LAUNCH_LOG2_FROM0(KERNEL, v, ...)                          \
    switch (v) {                                                      \
        case 0: hipLaunchKernelGGL(KERNEL<0>, __VA_ARGS__); break;    \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;    \
        default: FX_LAUNCH_LOG2_FROM2(KERNEL, v, __VA_ARGS__)         \
    }

bool fx_gemm_is_skinny(int32_t transa, int32_t transb, int64_t M, int64_t N, int64_t K, const void* workspace) {
    return K <= 8 || (N <= 4 && !transa) || (M <= 4 && transa && !transb && workspace);
}

static int fx_skinny_launch_k(int ta, int tb, GemmArgs& a, hipStream_t s) {
    a.split_k = 1;
    if (a.N % 4 == 0 && a.ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(a.C) & 15) == 0 &&
        a.M * (a.N / 4) < ((int64_t)1 << 31)) {
        int64_t blocks = fx_ceil_div(a.M * (a.N / 4), 256);
        if (blocks > 16384) blocks = 16384;
        hipLaunchKernelGGL(k_gemm_small_k_v4, dim3((unsigned)blocks), dim3(256), 0, s, a, ta, tb);
    } else {
        int64_t blocks = fx_ceil_div(a.M * a.N, 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_gemm_small_k, dim3((unsigned)blocks), dim3(256), 0, s, a, ta, tb);
    }
    FX_CHECK_LAUNCH();
    return FX_OK;
}

static int fx_skinny_launch_n(int tb, GemmArgs& a, hipStream_t s) {
    a.split_k = 1;
    const bool a_al = a.K % 4 == 0 && a.lda % 4 == 0 && (reinterpret_cast<uintptr_t>(a.A) & 15) == 0;
    if (a.K <= 256 && a_al) {
        int lpr_log2 = 0;
        while ((4 << lpr_log2) < a.K) ++lpr_log2;                 // lanes per row = pow2 >= K/4
        const int rpw = 64 >> lpr_log2;
        int64_t blocks = fx_ceil_div(a.M, 4 * rpw);
        if (blocks > 16384) blocks = 16384;
        FX_LAUNCH_LOG2_FROM0(k_gemm_small_n_v4, lpr_log2, dim3((unsigned)blocks), dim3(256), 0, s, a, tb);
    } else {
        int64_t blocks = fx_ceil_div(a.M, 4);
        if (blocks > 8192) blocks = 8192;
        if (tb && a_al && a.ldb % 4 == 0 && (reinterpret_cast<uintptr_t>(a.B) & 15) == 0)
            hipLaunchKernelGGL(k_gemm_small_n_wide, dim3((unsigned)blocks), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(k_gemm_small_n, dim3((unsigned)blocks), dim3(256), 0, s, a, tb);
    }
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// K split of the skinny weight-gradient kernels (k_gemm_small_m*, k_head_bwd_v4), from the slab count
// fx_gemm_prepare settled on: finer than the MFMA path wants — these kernels are column-parallel reductions
static void fx_skinny_m_slabs(GemmArgs& a) {
    const int64_t want = a.split_k > 1 ? a.split_k : 1;
    int64_t kc2 = fx_ceil_div(a.K, want);
    if (kc2 < 1) kc2 = 1;
    a.k_chunk = kc2;
    a.split_k = (int32_t)fx_ceil_div(a.K, kc2);
}

// float4 column groups per workgroup of k_gemm_small_m_v4 / k_head_bwd_v4: 4 .. 64, a power of two
static int fx_skinny_cg_log2(int64_t N) {
    int cg_log2 = 2;
    while ((4 << cg_log2) < N && cg_log2 < 6) ++cg_log2;
    return cg_log2;
}

static int fx_skinny_launch_m(GemmArgs& a, hipStream_t s) {
    fx_skinny_m_slabs(a);
    const bool v4 = (a.N >= 16) && (a.N % 4 == 0) && (a.ldb % 4 == 0) &&
                    ((reinterpret_cast<uintptr_t>(a.B) & 15) == 0) &&
                    ((reinterpret_cast<uintptr_t>(a.ws) & 15) == 0);
    if (v4) {
        const int cg_log2 = fx_skinny_cg_log2(a.N);
        const dim3 g((unsigned)fx_ceil_div(a.N, 4 << cg_log2), (unsigned)a.split_k);
        FX_LAUNCH_LOG2_FROM2(k_gemm_small_m_v4, cg_log2, g, dim3(256), 0, s, a);
    } else {
        int np_log2 = 0;
        while ((1 << np_log2) < a.N && np_log2 < 8) ++np_log2;
        hipLaunchKernelGGL(k_gemm_small_m, dim3((unsigned)fx_ceil_div(a.N, 1 << np_log2), (unsigned)a.split_k),
                           dim3(256), 0, s, a, np_log2);
    }
    FX_CHECK_LAUNCH();
    fx_launch_splitk_reduce(a, s);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

bool fx_gemm_skinny_launch(int32_t transa, int32_t transb, GemmArgs& a, hipStream_t s, int* rc) {
    if (!fx_gemm_is_skinny(transa, transb, a.M, a.N, a.K, a.ws)) return false;
    const int ta = (int)(transa != 0), tb = (int)(transb != 0);
    if (a.K <= 8) *rc = fx_skinny_launch_k(ta, tb, a, s);
    else if (a.N <= 4 && !transa) *rc = fx_skinny_launch_n(tb, a, s);
    else *rc = fx_skinny_launch_m(a, s);
    return true;
}

int fx_head_bwd_launch(HeadBwdArgs& h, hipStream_t s) {
    fx_skinny_m_slabs(h.dw);
    const int cg_log2 = fx_skinny_cg_log2(h.dw.N);
    const dim3 g((unsigned)fx_ceil_div(h.dw.N, 4 << cg_log2), (unsigned)h.dw.split_k);
    FX_LAUNCH_LOG2_FROM2(k_head_bwd_v4, cg_log2, g, dim3(256), 0, s, h);
    FX_CHECK_LAUNCH();
    fx_launch_splitk_reduce(h.dw, s);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
