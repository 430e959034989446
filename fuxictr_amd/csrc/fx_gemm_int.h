// fx_gemm_int.h — definitions shared by the GEMM translation units of libfxctr (internal, not part of the
// C ABI): fx_gemm.hip (host only: validation, planning, dispatch), fx_gemm_tile.hip (the fp32-MFMA tile
// kernels), fx_gemm_x6.hip (the split-bf16 kernels), fx_gemm_skinny.hip (K <= 8 / N <= 4 / M <= 4 and the
// fused head backward) and fx_gemm_reduce.hip (the split-K slab reduces).  A kernel is launched only from
// the unit that defines it: the units export the host launchers declared at the end of this file.
#pragma once
#include "fx_common.h"

#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define FX_BK 32

struct GemmArgs {
    const float* A;
    int64_t lda;
    const float* B;
    int64_t ldb;
    float* C;
    int64_t ldc;
    int64_t M, N, K;
    int64_t k_chunk;
    fx_gemm_epilogue epi;
    float* ws;
    int32_t split_k;
    int32_t tiles_m, tiles_n;
    int32_t edge_plain;          // M / N edge tiles run the unmasked k-loop bodies (fx_gemm_pipe_tile)
#ifdef FX_GEMM_LAB
    unsigned long long* trace;   // scripts/ubench/gemm_lab.hip: 8 words per workgroup (timestamps)
#endif
};

#ifdef FX_GEMM_LAB
inline unsigned long long* fx_gemm_lab_trace = nullptr;   // set by the lab before a traced launch
#define FX_LAB_STAMP(slot)                                                                    \
    do {                                                                                      \
        if (a.trace && threadIdx.x == 0)                                                      \
            a.trace[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (slot)] = wall_clock64(); \
    } while (0)
#else
#define FX_LAB_STAMP(slot) do {} while (0)
#endif

__device__ __forceinline__ float fx_epilogue(const fx_gemm_epilogue& e, float z, int64_t m,
                                             int64_t n) {
    if (e.bias) z += e.bias[n];
    if (e.zout) e.zout[m * e.ldz + n] = z;
    if (e.act == 1) z = fmaxf(z, 0.f);
    if (e.mul) z *= e.mul[m * e.ldmul + n];
    if (e.mask) z = e.mask[m * e.ldmask + n] > 0.f ? z : 0.f;
    if (e.add) z += e.add[m * e.ldadd + n];
    return z;
}

// The same epilogue for 4 adjacent columns n .. n+3 of one row (every operand 16-byte aligned: checked
// by the launcher), in two halves: the operand LOADS of a 32x32 accumulator tile are issued together,
// one tile ahead of the arithmetic and the stores.  (Written as load -> use -> store per vector, each
// of a lane's 16 vectors paid its own memory round trip — the compiler may not move a load above a
// store to memory it cannot prove distinct: +6.7 us on a 128x128 tile with bias + ReLU.)  Element for
// element the operation order of fx_epilogue.
struct FxEpiOps4 {
    float4 bias, mul, mask, add;
};

__device__ __forceinline__ void fx_epi_load4(const fx_gemm_epilogue& e, int64_t m, int64_t n,
                                             FxEpiOps4& o) {
    if (e.bias) o.bias = *reinterpret_cast<const float4*>(e.bias + n);
    if (e.mul) o.mul = *reinterpret_cast<const float4*>(e.mul + m * e.ldmul + n);
    if (e.mask) o.mask = *reinterpret_cast<const float4*>(e.mask + m * e.ldmask + n);
    if (e.add) o.add = *reinterpret_cast<const float4*>(e.add + m * e.ldadd + n);
}

__device__ __forceinline__ float4 fx_epi_apply4(const fx_gemm_epilogue& e, float4 z, int64_t m,
                                                int64_t n, const FxEpiOps4& o) {
    if (e.bias) { z.x += o.bias.x; z.y += o.bias.y; z.z += o.bias.z; z.w += o.bias.w; }
    if (e.zout) *reinterpret_cast<float4*>(e.zout + m * e.ldz + n) = z;
    if (e.act == 1) {
        z.x = fmaxf(z.x, 0.f); z.y = fmaxf(z.y, 0.f); z.z = fmaxf(z.z, 0.f); z.w = fmaxf(z.w, 0.f);
    }
    if (e.mul) { z.x *= o.mul.x; z.y *= o.mul.y; z.z *= o.mul.z; z.w *= o.mul.w; }
    if (e.mask) {
        z.x = o.mask.x > 0.f ? z.x : 0.f; z.y = o.mask.y > 0.f ? z.y : 0.f;
        z.z = o.mask.z > 0.f ? z.z : 0.f; z.w = o.mask.w > 0.f ? z.w : 0.f;
    }
    if (e.add) { z.x += o.add.x; z.y += o.add.y; z.z += o.add.z; z.w += o.add.w; }
    return z;
}

template <int I, int N, typename F>
__device__ __forceinline__ void fx_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        fx_static_for<I + 1, N>(f);
    }
}

#define FX_MULTI_MAX 4
struct MultiArgs {
    GemmArgs p[FX_MULTI_MAX];
    int32_t start[FX_MULTI_MAX + 1];     // first workgroup of each problem
    int32_t cfg[FX_MULTI_MAX];
    int32_t n;
};

// ---- fx_gemm_tile.hip -------------------------------------------------------------------------------
// the 16-byte epilogue (TR) applies: every vector access of the epilogue / the slab stores is aligned
bool fx_gemm_tr_ok(const GemmArgs& a);
// `a` prepared by fx_gemm_prepare with tiles_m / tiles_n counted in bm x bn tiles (128x128 | 128x64 | 64x64).
// pipe: the software-pipelined kernel (operands must pass fx_gemm_pipe_ok); plain: k_gemm_f32, av / bv =
// 16-byte loads of op(A) / op(B) are possible
int fx_gemm_tile_launch_pipe(int bm, int bn, bool a_kc, bool b_kc, const GemmArgs& a, hipStream_t s);
void fx_gemm_tile_launch_plain(int bm, int bn, bool a_kc, bool b_kc, bool av, bool bv, const GemmArgs& a,
                               hipStream_t s);
// two problems on 64x64 tiles in one grid (k_gemm_f32_pair), the first one's workgroups first.  bwd: dW = dZ^T X
// (m- / n-contiguous operands) and dX = dZ W; fwd: two x W^T products (16-byte epilogue, no K split)
void fx_gemm_tile_launch_pair_bwd(const GemmArgs& dw, const GemmArgs& dx, hipStream_t s);
void fx_gemm_tile_launch_pair_fwd(const GemmArgs& first, const GemmArgs& second, hipStream_t s);
// cfg[i] bit 0: A k-contiguous, bit 1: B k-contiguous, bit 2: 128x64 tile (else 128x128)
void fx_gemm_tile_launch_multi(const MultiArgs& ma, int64_t workgroups, hipStream_t s);

// ---- fx_gemm_reduce.hip -----------------------------------------------------------------------------
// C = epilogue(sum of the a.split_k slabs of a.ws) (+ the fused row sums); the caller checks the launch
void fx_launch_splitk_reduce(const GemmArgs& a, hipStream_t s);
// the same for every split-K problem of p[0 .. n): one launch where two or more take the vector kernel
void fx_launch_splitk_reduces(const GemmArgs* p, int n, hipStream_t s);

// ---- fx_gemm_skinny.hip -----------------------------------------------------------------------------
// K <= 8, N <= 4 with op(A) = A, or M <= 4 with A^T B and a workspace: the bandwidth-bound kernels
bool fx_gemm_is_skinny(int32_t transa, int32_t transb, int64_t M, int64_t N, int64_t K, const void* workspace);
// launches a prepared problem if it is skinny (-> true, *rc = FX_OK or the error); false: not skinny
bool fx_gemm_skinny_launch(int32_t transa, int32_t transb, GemmArgs& a, hipStream_t s, int* rc);
// backward of a Linear(hidden -> 1) head in one pass (k_head_bwd_v4)
struct HeadBwdArgs {
    GemmArgs dw;          // A = dz [K, 1] (lda), B = x [K, N] (ldb), ws slabs, rowsum
    float* dx;            // [K, N] (ldx)
    int64_t ldx;
    const float* w;       // [N]
    int32_t use_mask;
};
// h.dw as fx_gemm_prepare left it: the K split of the skinny weight gradient is settled here, by the rule of
// fx_gemm_skinny_launch.  Launches the kernel and its slab reduce.
int fx_head_bwd_launch(HeadBwdArgs& h, hipStream_t s);

// ---- fx_gemm_x6.hip ---------------------------------------------------------------------------------
// fp32-accurate GEMM on the bf16 matrix cores (operands split into three exact bf16 planes inside the
// kernel, six v_mfma_f32_32x32x16_bf16 products per fp32 product, fp32 accumulate), 128x128 tiles,
// 512 threads.  `a` prepared by fx_gemm_prepare with tiles_m / tiles_n counted in 128x128 tiles.
bool fx_gemm_x6_enabled();                      // FX_GEMM_BF16X6 (default 1)
int fx_gemm_x6_launch(bool a_kc, bool b_kc, const GemmArgs& a, hipStream_t s);
// cfg[i] bit 0: A k-contiguous, bit 1: B k-contiguous (bit 2 must be clear: 128x128 tiles only)
int fx_gemm_x6_launch_multi(const MultiArgs& ma, int64_t workgroups, hipStream_t s);
