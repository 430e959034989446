// fx_dice.hip — the Dice activation, and the finishing kernels of its statistics that the fused DIN
// attention (fx_din_attn.hip) shares through fx_dice_int.h.
//
// Reference (paths relative to the reference checkout):
//   fuxictr/pytorch/layers/activations.py:24-51                    Dice
//       p = sigmoid(BatchNorm1d(z; affine=False, eps=1e-9, momentum=0.01)); y = p z + alpha (1-p) z
//       NB inside DIN_Attention the batch statistics run over ALL B*L rows, padded positions included
//       (the mask is applied after the MLP) — reproduced as is.
// stats[0..H) = mean, stats[H..2H) = biased variance of the batch (training) or the running statistics
// (eval).  Every column reduction over the N rows is one pipeline:
//   stage 1  per-chunk partial sums of the terms              (k_dice_reduce*; the attention's stats passes)
//   stage 2  the chunks added in one fixed order              (k_chunks_sum)
//   [across ranks: the host all-reduces the sums]
//   stage 3  sums -> mean | biased variance, running update   (k_dice_stats_from_sums)
// and on one rank stages 2 + 3 are one launch (k_chunks_stats).  Fixed order everywhere: deterministic.
#include "fx_dice_int.h"

// Chunks of rows of stage 1.  The workspace holds FX_STAT_CHUNKS x 3 x H floats.  The backward passes use
// one chunk fewer: fx_dice_bwd keeps the finished 3H sums in the last chunk's slot of the same workspace,
// where k_dice_bwd reads them while the partials are still in place — and fx_dice_bwd_local_sums must add
// the same chunks in the same order to give the same bits.
#define FX_STAT_CHUNKS 1024
#define FX_STAT_CHUNKS_BWD (FX_STAT_CHUNKS - 1)

// ---------------------------------------------------------------------------------------------
// stage 1: partial[c][k][h] = sum over rows of chunk c of term k (k < NT)
// ---------------------------------------------------------------------------------------------
template <int MODE>  // 0: (z, z^2)   1: backward sums (dalpha, dzhat, dzhat*zhat)
__global__ __launch_bounds__(256) void k_dice_reduce(const float* Z, const float* dY,
                                                     const float* stats, const float* alpha,
                                                     float eps, int64_t N, int H, int64_t rows,
                                                     float* partial) {
    constexpr int NT = MODE == 0 ? 2 : 3;
    __shared__ float red[NT][256];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t h = (int64_t)blockIdx.x * 64 + tx;
    const int64_t r0 = (int64_t)blockIdx.y * rows;
    const int64_t r1 = (r0 + rows < N) ? r0 + rows : N;
    float acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = 0.f;
    if (h < H) {
        float mean = 0.f, rstd = 0.f, al = 0.f;
        if (MODE == 1) {
            mean = stats[h];
            rstd = rsqrtf(stats[H + h] + eps);
            al = alpha[h];
        }
        for (int64_t r = r0 + ty; r < r1; r += 4) {
            const float z = Z[r * H + h];
            if (MODE == 0) {
                acc[0] += z;
                acc[1] = fmaf(z, z, acc[1]);
            } else {
                const float zh = (z - mean) * rstd;
                const float p = 1.f / (1.f + expf(-zh));
                const float dy = dY[r * H + h];
                const float dzh = dy * z * (1.f - al) * p * (1.f - p);
                acc[0] = fmaf(dy * (1.f - p), z, acc[0]);   // d alpha
                acc[1] += dzh;
                acc[2] = fmaf(dzh, zh, acc[2]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    if (ty == 0 && h < H) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
            partial[((int64_t)blockIdx.y * NT + k) * H + h] =
                (red[k][tx] + red[k][tx + 64]) + (red[k][tx + 128] + red[k][tx + 192]);
    }
}

// H % 4 == 0: float4 columns, 16 threads per 64-column row segment, 16 row lanes, rows unrolled x2:
// the statistics pass is a pure HBM stream (52 MB at B*L = 204800, H = 64) and needs many loads in
// flight per CU to reach the bandwidth the one-float-per-thread version (above) cannot.
template <int MODE>
__global__ __launch_bounds__(256) void k_dice_reduce_v4(const float* Z, const float* dY,
                                                        const float* stats, const float* alpha,
                                                        float eps, int64_t N, int H, int64_t rows,
                                                        float* partial) {
    constexpr int NT = MODE == 0 ? 2 : 3;
    __shared__ float red[NT][16][64];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t h = (int64_t)blockIdx.x * 64 + tx * 4;
    const int64_t r0 = (int64_t)blockIdx.y * rows;
    const int64_t r1 = (r0 + rows < N) ? r0 + rows : N;
    float acc[NT][4];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.f;
    if (h < H) {
        float mean[4] = {0.f, 0.f, 0.f, 0.f}, rstd[4] = {0.f, 0.f, 0.f, 0.f}, al[4] = {0.f, 0.f, 0.f, 0.f};
        if (MODE == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                mean[e] = stats[h + e];
                rstd[e] = rsqrtf(stats[H + h + e] + eps);
                al[e] = alpha[h + e];
            }
        }
        auto term = [&](const float4& zq, const float4& dq) {
            const float z[4] = {zq.x, zq.y, zq.z, zq.w};
            const float d[4] = {dq.x, dq.y, dq.z, dq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (MODE == 0) {
                    acc[0][e] += z[e];
                    acc[1][e] = fmaf(z[e], z[e], acc[1][e]);
                } else {
                    const float zh = (z[e] - mean[e]) * rstd[e];
                    const float pr = 1.f / (1.f + expf(-zh));
                    const float dzh = d[e] * z[e] * (1.f - al[e]) * pr * (1.f - pr);
                    acc[0][e] = fmaf(d[e] * (1.f - pr), z[e], acc[0][e]);
                    acc[1][e] += dzh;
                    acc[2][e] = fmaf(dzh, zh, acc[2][e]);
                }
            }
        };
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        int64_t r = r0 + ty;
        for (; r + 16 < r1; r += 32) {
            const float4 z0 = *reinterpret_cast<const float4*>(Z + r * H + h);
            const float4 z1 = *reinterpret_cast<const float4*>(Z + (r + 16) * H + h);
            float4 d0 = zero, d1 = zero;
            if (MODE == 1) {
                d0 = *reinterpret_cast<const float4*>(dY + r * H + h);
                d1 = *reinterpret_cast<const float4*>(dY + (r + 16) * H + h);
            }
            term(z0, d0);
            term(z1, d1);
        }
        for (; r < r1; r += 16) {
            const float4 z0 = *reinterpret_cast<const float4*>(Z + r * H + h);
            float4 d0 = zero;
            if (MODE == 1) d0 = *reinterpret_cast<const float4*>(dY + r * H + h);
            term(z0, d0);
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[k][ty][tx * 4 + e] = acc[k][e];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int64_t hh = (int64_t)blockIdx.x * 64 + threadIdx.x;
        if (hh < H) {
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                float sum = 0.f;
#pragma unroll
                for (int y = 0; y < 16; ++y) sum += red[k][y][threadIdx.x];
                partial[((int64_t)blockIdx.y * NT + k) * H + hh] = sum;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// stages 2 and 3: the finishing kernels (256 threads = 16 columns x 16 chunk lanes)
// ---------------------------------------------------------------------------------------------
// t[j] = sum over the chunks of term k0 + j of column h = 16 blockIdx.x + (threadIdx.x & 15): every chunk
// lane (threadIdx.x >> 4) adds the chunks lane, lane + 16, ... with 8 independent loads in flight, then the
// 16 lane sums are added in lane order.  Valid in the threads of chunk lane 0 with h < H.  One barrier.
// (not fx_rowsum.h's row sum: 16 chunk lanes and NT terms at once, an order the DIN attention pipeline shares)
template <int NT>
__device__ __forceinline__ void fx_chunk_sums(const float* partial, int chunks, int nt, int k0, int64_t H,
                                              int64_t h, float (*red)[16][17], float (&t)[NT]) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int k = k0 + j;
        float s = 0.f;
        if (h < H) {
            int c = ty;
            for (; c + 7 * 16 < chunks; c += 8 * 16) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = partial[((int64_t)(c + u * 16) * nt + k) * H + h];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; c < chunks; c += 16) s += partial[((int64_t)c * nt + k) * H + h];
        }
        red[j][ty][tx] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NT; ++j) t[j] = 0.f;
    if (ty == 0 && h < H) {
#pragma unroll
        for (int y = 0; y < 16; ++y)
#pragma unroll
            for (int j = 0; j < NT; ++j) t[j] += red[j][y][tx];
    }
}

// column h: [sum z | sum z^2] over n_total rows -> mean | biased variance (clamped at 0), and BatchNorm1d's
// running update with the unbiased variance
__device__ __forceinline__ void fx_dice_stats_of(float sum, float sumsq, double n_total, float momentum,
                                                 int H, int h, float* stats, float* running_mean,
                                                 float* running_var) {
    const double mean = (double)sum / n_total;
    double var = (double)sumsq / n_total - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[h] = (float)mean;
    stats[H + h] = (float)var;
    if (running_mean) {
        const double unb = n_total > 1.0 ? var * n_total / (n_total - 1.0) : var;
        running_mean[h] = (float)((1.0 - momentum) * running_mean[h] + momentum * mean);
        running_var[h] = (float)((1.0 - momentum) * running_var[h] + momentum * unb);
    }
}

// out[k * H + h] = sum over chunks c (fixed order) of partial[(c * nt + k) * H + h];  k = blockIdx.y
__global__ __launch_bounds__(256) void k_chunks_sum(const float* partial, int chunks, int nt, int64_t H,
                                                    float* out) {
    __shared__ float red[1][16][17];
    const int64_t h = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
    const int k = blockIdx.y;
    float t[1];
    fx_chunk_sums<1>(partial, chunks, nt, k, H, h, red, t);
    if ((threadIdx.x >> 4) == 0 && h < H) out[(int64_t)k * H + h] = t[0];
}

__global__ __launch_bounds__(256) void k_dice_stats_from_sums(const float* sums, int H, double n_total,
                                                              float momentum, float* stats,
                                                              float* running_mean, float* running_var,
                                                              int64_t* num_batches_tracked) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h == 0 && num_batches_tracked) *num_batches_tracked += 1;   // nn.BatchNorm1d's step counter
    if (h >= H) return;
    fx_dice_stats_of(sums[h], sums[H + h], n_total, momentum, H, h, stats, running_mean, running_var);
}

// k_chunks_sum of the two terms [sum z | sum z^2] and k_dice_stats_from_sums in one launch
__global__ __launch_bounds__(256) void k_chunks_stats(const float* partial, int chunks, int H,
                                                      double n_total, float momentum, float* sums,
                                                      float* stats, float* running_mean,
                                                      float* running_var, int64_t* num_batches_tracked) {
    __shared__ float red[2][16][17];
    const int h = blockIdx.x * 16 + (threadIdx.x & 15);
    if (blockIdx.x == 0 && threadIdx.x == 0 && num_batches_tracked) *num_batches_tracked += 1;
    float t[2];
    fx_chunk_sums<2>(partial, chunks, 2, 0, H, h, red, t);
    if ((threadIdx.x >> 4) != 0 || h >= H) return;
    if (sums) {
        sums[h] = t[0];
        sums[H + h] = t[1];
    }
    fx_dice_stats_of(t[0], t[1], n_total, momentum, H, h, stats, running_mean, running_var);
}

void fx_chunks_sum_launch(const float* partial, int chunks, int nt, int64_t H, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_chunks_sum, dim3((unsigned)fx_ceil_div(H, 16), nt), dim3(256), 0, s, partial,
                       chunks, nt, H, out);
}

void fx_chunks_stats_launch(const float* partial, int chunks, int H, int64_t n_total, float momentum,
                            float* sums, float* stats, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, hipStream_t s) {
    hipLaunchKernelGGL(k_chunks_stats, dim3((unsigned)fx_ceil_div(H, 16)), dim3(256), 0, s, partial, chunks,
                       H, (double)n_total, momentum, sums, stats, running_mean, running_var,
                       num_batches_tracked);
}

// ---------------------------------------------------------------------------------------------
// the gate and its backward
// ---------------------------------------------------------------------------------------------
// forward apply: y = z (p + alpha (1 - p)),  p = sigmoid((z - mean) rstd)
__global__ __launch_bounds__(256) void k_dice_fwd(const float* Z, const float* stats,
                                                  const float* alpha, float eps, int64_t n, int H,
                                                  float* Y) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256) {
        const int h = (int)(i % H);
        const float z = Z[i];
        const float zh = (z - stats[h]) * rsqrtf(stats[H + h] + eps);
        const float p = 1.f / (1.f + expf(-zh));
        Y[i] = p * z + alpha[h] * (1.f - p) * z;
    }
}

// backward apply: dz = dy (p + alpha(1-p)) + rstd (dzhat - [mean(dzhat) + zhat mean(dzhat zhat)])
// (the bracket only in training mode, where the statistics depend on z)
__global__ __launch_bounds__(256) void k_dice_bwd(const float* Z, const float* dY,
                                                  const float* stats, const float* alpha,
                                                  const float* sums, float eps, int64_t n, int H,
                                                  int64_t N, int training, float* dZ) {
    const float invN = 1.f / (float)N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256) {
        const int h = (int)(i % H);
        const float z = Z[i], dy = dY[i], al = alpha[h];
        const float rstd = rsqrtf(stats[H + h] + eps);
        const float zh = (z - stats[h]) * rstd;
        const float p = 1.f / (1.f + expf(-zh));
        float dzh = dy * z * (1.f - al) * p * (1.f - p);
        if (training) dzh -= sums[H + h] * invN + zh * (sums[2 * H + h] * invN);
        dZ[i] = dy * (p + al * (1.f - p)) + dzh * rstd;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// stage 1 over all N rows; dY, stats, alpha, eps: MODE 1 only
template <int MODE>
static void dice_reduce_launch(const float* Z, const float* dY, const float* stats, const float* alpha,
                               float eps, int64_t N, int32_t H, float* partial, hipStream_t s) {
    const int chunks = MODE == 0 ? FX_STAT_CHUNKS : FX_STAT_CHUNKS_BWD;
    const int64_t rows = fx_ceil_div(N, chunks);
    const dim3 grid((unsigned)fx_ceil_div(H, 64), chunks);
    if (H % 4 == 0 && ((reinterpret_cast<uintptr_t>(Z) | reinterpret_cast<uintptr_t>(dY)) & 15) == 0)
        hipLaunchKernelGGL(k_dice_reduce_v4<MODE>, grid, dim3(256), 0, s, Z, dY, stats, alpha, eps, N,
                           (int)H, rows, partial);
    else
        hipLaunchKernelGGL(k_dice_reduce<MODE>, grid, dim3(256), 0, s, Z, dY, stats, alpha, eps, N, (int)H,
                           rows, partial);
}

// eval: normalise with the running statistics (BatchNorm1d.eval())
static int dice_stats_from_running(const float* running_mean, const float* running_var, int32_t H,
                                   float* stats, hipStream_t s) {
    FX_CHECK_HIP(hipMemcpyAsync(stats, running_mean, sizeof(float) * H, hipMemcpyDeviceToDevice, s));
    FX_CHECK_HIP(hipMemcpyAsync(stats + H, running_var, sizeof(float) * H, hipMemcpyDeviceToDevice, s));
    return FX_OK;
}

static void dice_fwd_apply(const float* Z, int64_t N, int32_t H, const float* alpha, float eps,
                           const float* stats, float* Y, hipStream_t s) {
    const int64_t n = N * H;
    int64_t blocks = fx_ceil_div(n, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_dice_fwd, dim3((unsigned)blocks), dim3(256), 0, s, Z, stats, alpha, eps, n,
                       (int)H, Y);
}

static void dice_bwd_apply(const float* Z, const float* dY, int64_t N, int32_t H, const float* alpha,
                           float eps, int32_t training, const float* stats, const float* sums3,
                           int64_t n_total, float* dZ, hipStream_t s) {
    const int64_t n = N * H;
    int64_t blocks = fx_ceil_div(n, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_dice_bwd, dim3((unsigned)blocks), dim3(256), 0, s, Z, dY, stats, alpha, sums3,
                       eps, n, (int)H, n_total, (int)training, dZ);
}

extern "C" int64_t fx_dice_workspace_floats(int32_t H) { return (int64_t)FX_STAT_CHUNKS * 3 * H; }

// ---------------------------------------------------------------------------------------------
// Dice across ranks (row-sharded training: every rank holds B/N samples of the global batch).  The
// reference normalises with the statistics of the WHOLE batch (activations.py:40-51), so the two
// column reductions are split from their consumers: local sums -> (the host all-reduces them) ->
// apply with the global row count.
// ---------------------------------------------------------------------------------------------
extern "C" int fx_dice_local_sums(const float* Z, int64_t N, int32_t H, float* sums,
                                  float* workspace, fx_stream_t stream) {
    FX_CHECK_ARG(N >= 1 && H >= 1, "fx_dice_local_sums: bad sizes");
    FX_CHECK_ARG(Z && sums && workspace, "fx_dice_local_sums: null pointer");
    hipStream_t s = fx_hip_stream(stream);
    dice_reduce_launch<0>(Z, nullptr, nullptr, nullptr, 0.f, N, H, workspace, s);
    fx_chunks_sum_launch(workspace, FX_STAT_CHUNKS, 2, H, sums, s);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_dice_stats_from_sums(const float* sums, int32_t H, int64_t n_total, float momentum,
                                       int32_t training, float* running_mean, float* running_var,
                                       int64_t* num_batches_tracked, float* stats, fx_stream_t stream) {
    FX_CHECK_ARG(H >= 1 && stats, "fx_dice_stats_from_sums: bad arguments");
    hipStream_t s = fx_hip_stream(stream);
    if (!training) {
        FX_CHECK_ARG(running_mean && running_var, "fx_dice_stats_from_sums: null running statistics");
        return dice_stats_from_running(running_mean, running_var, H, stats, s);
    }
    FX_CHECK_ARG(sums && n_total >= 1, "fx_dice_stats_from_sums: training mode needs the sums");
    hipLaunchKernelGGL(k_dice_stats_from_sums, dim3((unsigned)fx_ceil_div(H, 256)), dim3(256), 0, s, sums,
                       (int)H, (double)n_total, momentum, stats, running_mean, running_var,
                       num_batches_tracked);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_dice_fwd_from_sums(const float* Z, int64_t N, int32_t H, const float* alpha,
                                     float eps, float momentum, const float* sums, int64_t n_total,
                                     float* running_mean, float* running_var, float* stats,
                                     float* Y, fx_stream_t stream) {
    FX_CHECK_ARG(N >= 1 && H >= 1 && n_total >= N, "fx_dice_fwd_from_sums: bad sizes");
    FX_CHECK_ARG(Z && alpha && sums && stats && Y, "fx_dice_fwd_from_sums: null pointer");
    hipStream_t s = fx_hip_stream(stream);
    hipLaunchKernelGGL(k_dice_stats_from_sums, dim3((unsigned)fx_ceil_div(H, 256)), dim3(256), 0, s, sums,
                       (int)H, (double)n_total, momentum, stats, running_mean, running_var,
                       (int64_t*)nullptr);
    dice_fwd_apply(Z, N, H, alpha, eps, stats, Y, s);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_dice_bwd_local_sums(const float* Z, const float* dY, int64_t N, int32_t H,
                                      const float* alpha, float eps, const float* stats,
                                      float* sums3, float* workspace, fx_stream_t stream) {
    FX_CHECK_ARG(N >= 1 && H >= 1, "fx_dice_bwd_local_sums: bad sizes");
    FX_CHECK_ARG(Z && dY && alpha && stats && sums3 && workspace,
                 "fx_dice_bwd_local_sums: null pointer");
    hipStream_t s = fx_hip_stream(stream);
    dice_reduce_launch<1>(Z, dY, stats, alpha, eps, N, H, workspace, s);
    fx_chunks_sum_launch(workspace, FX_STAT_CHUNKS_BWD, 3, H, sums3, s);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_dice_bwd_from_sums(const float* Z, const float* dY, int64_t N, int32_t H,
                                     const float* alpha, float eps, const float* stats,
                                     const float* sums3, int64_t n_total, float* dZ,
                                     fx_stream_t stream) {
    FX_CHECK_ARG(N >= 1 && H >= 1 && n_total >= N, "fx_dice_bwd_from_sums: bad sizes");
    FX_CHECK_ARG(Z && dY && alpha && stats && sums3 && dZ, "fx_dice_bwd_from_sums: null pointer");
    dice_bwd_apply(Z, dY, N, H, alpha, eps, 1, stats, sums3, n_total, dZ, fx_hip_stream(stream));
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------
// Dice on one rank: the same pipeline with nothing between the sums and their consumers
// ---------------------------------------------------------------------------------------------
extern "C" int fx_dice_fwd(const float* Z, int64_t N, int32_t H, const float* alpha, float eps,
                           float momentum, int32_t training, float* running_mean,
                           float* running_var, float* stats, float* Y, float* workspace,
                           fx_stream_t stream) {
    FX_CHECK_ARG(N >= 1 && H >= 1, "fx_dice_fwd: bad sizes");
    FX_CHECK_ARG(Z && alpha && stats && Y && running_mean && running_var,
                 "fx_dice_fwd: null pointer");
    hipStream_t s = fx_hip_stream(stream);
    if (training) {
        FX_CHECK_ARG(workspace, "fx_dice_fwd: training mode needs a workspace");
        dice_reduce_launch<0>(Z, nullptr, nullptr, nullptr, 0.f, N, H, workspace, s);
        fx_chunks_stats_launch(workspace, FX_STAT_CHUNKS, H, N, momentum, nullptr, stats, running_mean,
                               running_var, nullptr, s);
    } else {
        const int rc = dice_stats_from_running(running_mean, running_var, H, stats, s);
        if (rc != FX_OK) return rc;
    }
    dice_fwd_apply(Z, N, H, alpha, eps, stats, Y, s);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_dice_bwd(const float* Z, const float* dY, int64_t N, int32_t H,
                           const float* alpha, float eps, int32_t training, const float* stats,
                           float* dZ, float* dalpha, float* workspace, fx_stream_t stream) {
    FX_CHECK_ARG(N >= 1 && H >= 1, "fx_dice_bwd: bad sizes");
    FX_CHECK_ARG(Z && dY && alpha && stats && dZ && dalpha && workspace,
                 "fx_dice_bwd: null pointer");
    hipStream_t s = fx_hip_stream(stream);
    float* sums3 = workspace + (int64_t)FX_STAT_CHUNKS_BWD * 3 * H;   // the slot the backward leaves free
    const int rc = fx_dice_bwd_local_sums(Z, dY, N, H, alpha, eps, stats, sums3, workspace, stream);
    if (rc != FX_OK) return rc;
    FX_CHECK_HIP(hipMemcpyAsync(dalpha, sums3, sizeof(float) * H, hipMemcpyDeviceToDevice, s));
    dice_bwd_apply(Z, dY, N, H, alpha, eps, training, stats, sums3, N, dZ, s);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
