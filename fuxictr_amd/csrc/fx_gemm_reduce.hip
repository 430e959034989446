// fx_gemm_reduce.hip — the slab reduces of the split-K GEMMs: every kernel that writes K slabs to a workspace
// (fx_gemm_tile.hip, fx_gemm_x6.hip, fx_gemm_skinny.hip) is followed by one of these, which adds the slabs in
// slab order and applies the epilogue.  Exports fx_launch_splitk_reduce / fx_launch_splitk_reduces
// (fx_gemm_int.h).  (Not fx_rowsum.h's row sum: these apply the GEMM's epilogue and serve several problems a launch.)
#include "fx_common.h"
#include "fx_gemm_int.h"

__global__ __launch_bounds__(256) void k_splitk_reduce(GemmArgs a) {
    const int64_t total = a.M * a.N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * 256) {
        float s = 0.f;
        for (int z = 0; z < a.split_k; ++z) s += a.ws[(int64_t)z * total + i];
        const int64_t m = i / a.N, n = i - m * a.N;
        a.C[m * a.ldc + n] = fx_epilogue(a.epi, s, m, n);
    }
    if (a.epi.rowsum) {
        const float* rs = a.ws + (int64_t)a.split_k * total;
        for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < a.M;
             m += (int64_t)gridDim.x * 256) {
            float s = 0.f;
            for (int z = 0; z < a.split_k; ++z) s += rs[(int64_t)z * a.M + m];
            a.epi.rowsum[m] = s;
        }
    }
}


// The same sums on 16-byte vectors (N % 4 == 0, everything 16-byte aligned: fx_gemm_tr_ok): the slab loads
// of a vector are issued together (SK <= 8 of them: the split rules' range) and added in slab order, so the
// result is bit for bit k_splitk_reduce's.  4096 x 1024 x 1024's weight gradient (8 slabs of 4 MB): 7.4 us
// -> round 4's A/B in profiles/.
template <int SK>
__device__ __forceinline__ void fx_splitk_reduce_v4_body(const GemmArgs& a, int64_t bx, int64_t gx) {
    const int64_t total = a.M * a.N, nv = total >> 2, n4 = a.N >> 2;
    const int sk = SK > 0 ? SK : a.split_k;
    for (int64_t i = bx * 256 + threadIdx.x; i < nv; i += gx * 256) {
        const float4* w = reinterpret_cast<const float4*>(a.ws) + i;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (SK > 0) {
            float4 v[SK];
#pragma unroll
            for (int z = 0; z < SK; ++z) v[z] = w[(int64_t)z * nv];
#pragma unroll
            for (int z = 0; z < SK; ++z) { s.x += v[z].x; s.y += v[z].y; s.z += v[z].z; s.w += v[z].w; }
        } else {
            int z = 0;
            for (; z + 4 <= sk; z += 4) {          // four independent loads at a time, added in slab order
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = w[(int64_t)(z + u) * nv];
#pragma unroll
                for (int u = 0; u < 4; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
            }
            for (; z < sk; ++z) {
                const float4 v = w[(int64_t)z * nv];
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        }
        const int64_t m = i / n4, n = (i - m * n4) << 2;
        FxEpiOps4 o;
        fx_epi_load4(a.epi, m, n, o);
        *reinterpret_cast<float4*>(a.C + m * a.ldc + n) = fx_epi_apply4(a.epi, s, m, n, o);
    }
    if (a.epi.rowsum) {
        const float* rs = a.ws + (int64_t)sk * total;
        for (int64_t m = bx * 256 + threadIdx.x; m < a.M;
             m += gx * 256) {
            float r = 0.f;
            int z = 0;
            for (; z + 8 <= sk; z += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = rs[(int64_t)(z + u) * a.M + m];
#pragma unroll
                for (int u = 0; u < 8; ++u) r += v[u];
            }
            for (; z < sk; ++z) r += rs[(int64_t)z * a.M + m];
            a.epi.rowsum[m] = r;
        }
    }
}

template <int SK>
__global__ __launch_bounds__(256) void k_splitk_reduce_v4(GemmArgs a) {
    fx_splitk_reduce_v4_body<SK>(a, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// (round 6) the slab reduces of every weight gradient of ONE multi-problem GEMM launch in one launch (DCNv2's
// cross + deep pairs: 7 reduce launches per step -> 4): workgroups [start[i], start[i + 1]) take problem i and
// run the single-problem body on it — same sums, same order, same bits.
struct ReduceMultiArgs {
    GemmArgs p[FX_MULTI_MAX];
    int32_t start[FX_MULTI_MAX + 1];
    int32_t n;
};
__global__ __launch_bounds__(256) void k_splitk_reduce_v4_multi(ReduceMultiArgs ma) {
    int i = 0;
#pragma unroll
    for (int q = 1; q < FX_MULTI_MAX; ++q)
        if (q < ma.n && (int)blockIdx.x >= ma.start[q]) i = q;
    const int64_t bx = (int64_t)blockIdx.x - ma.start[i], gx = (int64_t)ma.start[i + 1] - ma.start[i];
    // (indexing p[] by a runtime value would copy the 200-byte argument block to scratch: select by branches)
#define FX_RM_CASE(Q)                                                                        \
    if (i == Q) {                                                                            \
        const GemmArgs& a = ma.p[Q];                                                         \
        switch (a.split_k) {                                                                 \
            case 2: fx_splitk_reduce_v4_body<2>(a, bx, gx); break;                           \
            case 4: fx_splitk_reduce_v4_body<4>(a, bx, gx); break;                           \
            case 8: fx_splitk_reduce_v4_body<8>(a, bx, gx); break;                           \
            default: fx_splitk_reduce_v4_body<0>(a, bx, gx); break;                          \
        }                                                                                    \
        return;                                                                              \
    }
    FX_RM_CASE(0)
    FX_RM_CASE(1)
    FX_RM_CASE(2)
    FX_RM_CASE(3)
#undef FX_RM_CASE
}

// many slabs over a small output (skinny weight gradients with K = B*L): EL elements x 256/EL slab
// lanes per workgroup, fixed LDS tree over the slab lanes (deterministic)
template <int EL>
__global__ __launch_bounds__(256) void k_splitk_reduce_wide(GemmArgs a) {
    constexpr int ZL = 256 / EL;
    __shared__ float red[256];
    const int ii = threadIdx.x % EL, zi = threadIdx.x / EL;
    const int64_t total = a.M * a.N;
    const int64_t i = (int64_t)blockIdx.x * EL + ii;
    float s = 0.f;
    if (i < total) {
        int z = zi;
        for (; z + 7 * ZL < a.split_k; z += 8 * ZL) {      // 8 independent loads in flight,
            float v[8];                                     // summed in slab order
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = a.ws[(int64_t)(z + u * ZL) * total + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; z < a.split_k; z += ZL) s += a.ws[(int64_t)z * total + i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = ZL >> 1; h > 0; h >>= 1) {
        if (zi < h) red[threadIdx.x] += red[threadIdx.x + h * EL];
        __syncthreads();
    }
    if (zi == 0 && i < total) {
        const int64_t m = i / a.N, n = i - m * a.N;
        a.C[m * a.ldc + n] = fx_epilogue(a.epi, red[ii], m, n);
    }
    if (a.epi.rowsum && blockIdx.x == 0) {     // block-uniform
        // fused bias gradient: rowsum[m] = sum over the slabs' row sums.  With hundreds of slabs a
        // one-thread-per-row loop is a chain of dependent loads (64 us for 256 slabs): all 256
        // threads work, Mp (= pow2 >= M, M <= 256) rows x 256/Mp slab lanes, same fixed LDS tree
        const float* rs = a.ws + (int64_t)a.split_k * total;
        int mp_log2 = 0;
        while ((1 << mp_log2) < a.M) ++mp_log2;
        const int Mp = 1 << mp_log2, ZR = 256 >> mp_log2;
        const int m = threadIdx.x & (Mp - 1), zr = threadIdx.x >> mp_log2;
        __syncthreads();                         // red[] is reused: the output tree is fully read
        float r = 0.f;
        if (m < a.M) {
            int z = zr;
            for (; z + 7 * ZR < a.split_k; z += 8 * ZR) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = rs[(int64_t)(z + u * ZR) * a.M + m];
#pragma unroll
                for (int u = 0; u < 8; ++u) r += v[u];
            }
            for (; z < a.split_k; z += ZR) r += rs[(int64_t)z * a.M + m];
        }
        red[threadIdx.x] = r;
        __syncthreads();
        for (int h = ZR >> 1; h > 0; h >>= 1) {
            if (zr < h) red[threadIdx.x] += red[threadIdx.x + h * Mp];
            __syncthreads();
        }
        if (zr == 0 && m < a.M) a.epi.rowsum[m] = red[m];
    }
}

static int fx_splitk_v4_mode() {     // FX_SPLITK_V4=0: the 4-byte slab reduce (A/B runs)
    static const int mode = fx_env_int("FX_SPLITK_V4", 1);
    return mode;
}

void fx_launch_splitk_reduce(const GemmArgs& a, hipStream_t s) {
    const int64_t total = a.M * a.N;
    if (a.split_k >= 32 && total <= 65536 && a.M <= 256) {
        if (a.split_k >= 128 && total <= 2048)   // few outputs, very many slabs: more slab lanes
            hipLaunchKernelGGL(k_splitk_reduce_wide<8>, dim3((unsigned)fx_ceil_div(total, 8)),
                               dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(k_splitk_reduce_wide<32>, dim3((unsigned)fx_ceil_div(total, 32)),
                               dim3(256), 0, s, a);
    } else if (fx_splitk_v4_mode() && fx_gemm_tr_ok(a) && (total & 3) == 0) {
        int64_t blocks = fx_ceil_div(total >> 2, 256);      // one vector per thread up to 4096 workgroups
        if (blocks > 4096) blocks = 4096;
        const dim3 g((unsigned)blocks), b(256);
        switch (a.split_k) {
            case 2: hipLaunchKernelGGL(k_splitk_reduce_v4<2>, g, b, 0, s, a); break;
            case 4: hipLaunchKernelGGL(k_splitk_reduce_v4<4>, g, b, 0, s, a); break;
            case 8: hipLaunchKernelGGL(k_splitk_reduce_v4<8>, g, b, 0, s, a); break;
            case 16: hipLaunchKernelGGL(k_splitk_reduce_v4<16>, g, b, 0, s, a); break;   // (the DIN tower)
            default: hipLaunchKernelGGL(k_splitk_reduce_v4<0>, g, b, 0, s, a); break;
        }
    } else {
        int64_t blocks = fx_ceil_div(total, 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)blocks), dim3(256), 0, s, a);
    }
}

static bool fx_splitk_reduce_is_v4(const GemmArgs& a) {
    const int64_t total = a.M * a.N;
    return !(a.split_k >= 32 && total <= 65536 && a.M <= 256) && fx_splitk_v4_mode() && fx_gemm_tr_ok(a) &&
           (total & 3) == 0;
}

// every split-K problem of a multi-problem launch: one reduce launch when two or more of them take the vector
// kernel (FX_REDUCE_MULTI=0: one launch each, as in rounds 3 - 5)
void fx_launch_splitk_reduces(const GemmArgs* p, int n, hipStream_t s) {
    static const bool multi = fx_env_int("FX_REDUCE_MULTI", 1) != 0;
    ReduceMultiArgs ma;
    memset(&ma, 0, sizeof(ma));
    int cnt = 0;
    int64_t wgs = 0;
    for (int i = 0; i < n && multi; ++i)
        if (p[i].split_k > 1 && fx_splitk_reduce_is_v4(p[i])) {
            int64_t blocks = fx_ceil_div((p[i].M * p[i].N) >> 2, 256);
            if (blocks > 4096) blocks = 4096;
            ma.p[cnt] = p[i];
            ma.start[cnt] = (int32_t)wgs;
            wgs += blocks;
            ++cnt;
        }
    if (cnt >= 2) {
        for (int q = cnt; q <= FX_MULTI_MAX; ++q) ma.start[q] = (int32_t)wgs;
        ma.n = cnt;
        hipLaunchKernelGGL(k_splitk_reduce_v4_multi, dim3((unsigned)wgs), dim3(256), 0, s, ma);
    }
    for (int i = 0; i < n; ++i)
        if (p[i].split_k > 1 && !(cnt >= 2 && fx_splitk_reduce_is_v4(p[i]))) fx_launch_splitk_reduce(p[i], s);
}
