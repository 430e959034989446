// fx_rowsum.h — the second stage of the two-stage weight-gradient reduces.  Stage 1 (a layer's own backward
// kernel) writes one row of partial sums per workgroup or slab of samples into caller workspace; fx_rowsum adds
// column i of partial[rows, ld] over the rows in a fixed order: two launches on the same partials give the same
// bits.  64 columns per workgroup, four waves, no atomics.  ACC is the accumulator (float or double), ORDER how
// the waves walk the rows:
//   FX_ROWS_SLICES  wave w adds rows w, w + 4, ...; the four sums meet as (s0 + s1) + (s2 + s3)
//   FX_ROWS_RUNS    wave w adds the w-th run of ceil(rows / 4) consecutive rows; they meet as ((s0 + s1) + s2) + s3
//   FX_ROWS_SERIAL  wave 0 adds every row in turn; the other three leave at once
// A new layer takes <double, FX_ROWS_SLICES> unless it has a reason not to: a column's loads are spread over the
// four waves whatever the row count, and the fp64 sum of fp32 partials rounds once, at the end.  The other
// combinations stay because their callers' results are pinned to the bit, not because they are better:
//   <float,  SLICES>  fx_colsum (fx_dense_misc.hip; through it AFM, FwFM / FmFM, BST and the bias gradient)
//   <double, SLICES>  fx_mhsa_bwd, fx_bilinear_bwd (its slabs), fx_senet_bwd
//   <float,  RUNS>    fx_gate2_bwd, fx_biagg_bwd (fx_finalmlp.hip)
//   <float,  SERIAL>  fx_layernorm_bwd, fx_emb_numeric_grad
// Fewer rows than waves (one row included) take no arm of their own: a wave without rows adds an exact 0.
//
// The sums leave through an FxRowsumOut: up to three consecutive column segments with a pointer each (LayerNorm's
// dgamma | dbeta, the head's dw_x | dw_y | db).  A segment whose pointer is null is skipped and its columns of
// `partial` are never read (stage 1 need not have written them).  A segment may alias row 0 of partial: column i
// of it is read and written by one thread.
#pragma once
#include "fx_common.h"

enum { FX_ROWS_SLICES, FX_ROWS_RUNS, FX_ROWS_SERIAL };

struct FxRowsumOut {
    float* p[3];
    int64_t n[3];
};

static inline FxRowsumOut fx_rowsum_out(float* p0, int64_t n0, float* p1 = nullptr, int64_t n1 = 0,
                                        float* p2 = nullptr, int64_t n2 = 0) {
    return FxRowsumOut{{p0, p1, p2}, {n0, n1, n2}};
}

#ifdef __HIPCC__
// where column i goes; null: a skipped segment, or i past the last one
__device__ __forceinline__ float* fx_rowsum_dst(const FxRowsumOut& o, int64_t i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (i < o.n[k]) return o.p[k] ? o.p[k] + i : nullptr;
        i -= o.n[k];
    }
    return nullptr;
}

// Column i (its lane: threadIdx.x & 63) over the rows; the result is valid in wave 0.  Called by all 256 threads
// of the workgroup, `live` or not (one barrier inside).
template <typename ACC, int ORDER>
__device__ __forceinline__ float fx_rowsum_col(const float* partial, int rows, int64_t ld, int64_t i, bool live) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int r0 = w, r1 = rows, step = 4;
    if constexpr (ORDER != FX_ROWS_SLICES) {        // consecutive rows per wave; serial: all of them to wave 0
        const int per = ORDER == FX_ROWS_RUNS ? (rows + 3) / 4 : rows;
        r0 = w * per; r1 = r0 + per < rows ? r0 + per : rows; step = 1;
    }
    ACC t = 0;
    if (live)
        for (int r = r0; r < r1; r += step) t += (ACC)partial[(int64_t)r * ld + i];
    if constexpr (ORDER == FX_ROWS_SERIAL) {
        return (float)t;
    } else {
        __shared__ ACC red[4][64];
        red[w][lane] = t;
        __syncthreads();
        if (w != 0) return 0.f;
        const ACC s01 = red[0][lane] + red[1][lane], s2 = red[2][lane], s3 = red[3][lane];
        return (float)(ORDER == FX_ROWS_SLICES ? s01 + (s2 + s3) : (s01 + s2) + s3);
    }
}

template <typename ACC, int ORDER>
__global__ __launch_bounds__(256) void k_fx_rowsum(const float* partial, int rows, int64_t ld, FxRowsumOut o) {
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    float* dst = fx_rowsum_dst(o, i);
    const float t = fx_rowsum_col<ACC, ORDER>(partial, rows, ld, i, dst != nullptr);
    if (threadIdx.x < 64 && dst) *dst = t;
}

// o's columns = the sums over `rows` rows of partial, ld floats apart
template <typename ACC, int ORDER>
static int fx_rowsum(hipStream_t s, const float* partial, int rows, int64_t ld, const FxRowsumOut& o) {
    const int64_t C = o.n[0] + o.n[1] + o.n[2];
    hipLaunchKernelGGL((k_fx_rowsum<ACC, ORDER>), dim3((unsigned)fx_ceil_div(C, 64)), dim3(256), 0, s, partial, rows,
                       ld, o);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
#endif  // __HIPCC__
