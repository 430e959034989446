// fx_layernorm.hip — MaskNet's normalisation over the feature axis (model_zoo/MaskNet/src/MaskNet.py:97-99,
// 116-118 the per-field `emb_norm`, :254-257 the LayerNorm + ReLU of a mask block) and the mask's gradient toward
// V_hidden (:272-273).  torch.nn.LayerNorm's formulas, grouped: a row holds G groups of N elements, every group
// with its own affine pair
//     mu = mean_n x;  var = mean_n (x - mu)^2;  rstd = 1 / sqrt(var + eps)
//     y = (x - mu) * rstd * gamma[g, n] + beta[g, n]   (then max(y, 0) when the ReLU is fused)
// The mean is refined by the mean of the residuals and the variance is a further pass over the centred values,
// which a lane keeps in registers: x is read once, never E[x^2] - mu^2.
//
// One (row, group) segment of N floats is held in registers by L lanes, CH chunks of VEC floats per lane, chunk
// c of lane l at element (c * L + l) * VEC: consecutive lanes read consecutive addresses.  VEC is 4 (16-byte
// accesses) when N % 4 == 0 and every base pointer, row stride and column offset is 16-byte aligned, else 1.
// Regimes (ln_plan):
//     N <= 64                      a sub-wave group of L = 2^k >= N / VEC lanes (1 .. 64), CH = 1: a wave handles
//                                  64 / L segments at once, sums by xor shuffles inside the group
//     64 < N <= 2048  (VEC = 4)    a wave per segment, CH = 1, 2, 4, 8 (N <= 256, 512, 1024, 2048)
//     64 < N <= 512   (VEC = 1)    a wave per segment, CH = 2, 4, 8 (N <= 128, 256, 512)
//     above, N <= 8192             a workgroup of 256 threads per segment: VEC = 4: CH = 4, 8 (N <= 4096, 8192);
//                                  VEC = 1: CH = 4, 8, 32 (N <= 1024, 2048, 8192); sums through LDS
// Backward: dX in the same geometry (x, dY, Y's sign and gamma in registers, two sums per segment);
// dgamma / dbeta in a second pass, a thread per column of the [G * N] affine pair and a slab of rows per
// workgroup row, partial sums into caller workspace and a fixed-order sum over the slabs (fx_rowsum.h's shared row
// sum, serial in fp32).  No atomics anywhere: two launches on the same inputs give the same bits.
#include "fx_common.h"
#include "fx_rowsum.h"

#define LN_T 256
#define LN_MAX_N 8192
#define LN_MAX_G 64
#define LN_MAX_WG 2048            // 8 workgroups per CU
#define LN_SLAB_WG 1024           // workgroups the dgamma / dbeta pass aims for
#define LN_MAX_SLABS 256

struct LnArgs {
    const float* X; int64_t x_ld;
    int64_t rows;
    int G, N, L, relu;
    const float* gamma; const float* beta;
    float eps;
    float* Y; int64_t y_ld;             // (column offsets are already added to the pointers)
    float* stats;                       // [rows, G, 2]: mu, rstd
    const float* dY; int64_t dy_ld;
    float* dX; int64_t dx_ld; int dx_acc;
    float* partial;                     // [nslab, 2, G * N]
    int64_t rows_per_slab;
};

struct LnPlan {
    int vec, ch, L;
    bool block;
};

static LnPlan ln_plan(int N, bool vec4) {
    LnPlan q;
    q.vec = vec4 ? 4 : 1;
    const int chunks = (N + q.vec - 1) / q.vec;
    q.block = false;
    q.ch = 1;
    if (N <= 64) {
        q.L = 1;
        while (q.L < chunks) q.L <<= 1;
    } else if (chunks <= 64 * 8) {
        q.L = 64;
        const int need = (chunks + 63) / 64;
        while (q.ch < need) q.ch <<= 1;
    } else {
        q.L = LN_T;
        q.block = true;
        const int need = (chunks + LN_T - 1) / LN_T;
        q.ch = need <= 4 ? 4 : (need <= 8 ? 8 : 32);
    }
    return q;
}

struct LnSlabs {
    int nslab;
    int64_t rows_per_slab;
};

static LnSlabs ln_slabs(int64_t rows, int64_t C) {
    LnSlabs s;
    const int64_t colblocks = fx_ceil_div(C, LN_T);
    int64_t want = fx_ceil_div(LN_SLAB_WG, colblocks);
    if (want > LN_MAX_SLABS) want = LN_MAX_SLABS;
    if (want > rows) want = rows;
    if (want < 1) want = 1;
    s.rows_per_slab = fx_ceil_div(rows > 0 ? rows : 1, want);
    s.nslab = (int)fx_ceil_div(rows > 0 ? rows : 1, s.rows_per_slab);
    return s;
}

// sum over the L lanes (threads) of a segment, the result in every one of them
template <bool BLOCK>
__device__ __forceinline__ float ln_sum(float x, int L, float* red) {
    if constexpr (BLOCK) {
        x = fx_wave_sum(x);
        __syncthreads();                        // (the previous sum's readers are done with red)
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
        __syncthreads();
        return (red[0] + red[1]) + (red[2] + red[3]);
    } else {
        for (int off = L >> 1; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
        return x;
    }
}

// which segment this thread works on in the round that starts at segment s0, and as which of its L lanes
template <bool BLOCK>
__device__ __forceinline__ void ln_place(const LnArgs& p, int64_t s0, int64_t& seg, int& sub) {
    if constexpr (BLOCK) {
        seg = s0;
        sub = threadIdx.x;
    } else {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, per_wave = 64 / p.L;
        seg = s0 + wave * per_wave + lane / p.L;
        sub = lane & (p.L - 1);
    }
}

template <int VEC, int CH, bool BLOCK>
__global__ __launch_bounds__(LN_T) void k_ln_fwd(LnArgs p) {
    __shared__ float red[4];
    const int N = p.N, G = p.G, L = BLOCK ? LN_T : p.L;
    const int64_t S = p.rows * G;
    const int per_wg = BLOCK ? 1 : (LN_T / 64) * (64 / L);
    const float inv_n = 1.f / (float)N;
    for (int64_t s0 = (int64_t)blockIdx.x * per_wg; s0 < S; s0 += (int64_t)gridDim.x * per_wg) {
        int64_t seg;
        int sub;
        ln_place<BLOCK>(p, s0, seg, sub);
        const bool active = seg < S;
        const int64_t r = active ? seg / G : 0;
        const int g = active ? (int)(seg - r * G) : 0;
        const float* x = p.X + r * p.x_ld + (int64_t)g * N;
        float v[CH][VEC];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * L + sub) * VEC;
            if (active && e < N) {
                fx_load<VEC>(x + e, v[c]);
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[c][k] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) sum += v[c][k];
        }
        // the mean in two steps: the residuals x - mu0 are exact where it matters (x close to mu0), their own mean
        // takes the rounding of the first sum out again (a row with mean 1e4 and spread 1e-2 stays normalisable)
        const float mu0 = ln_sum<BLOCK>(sum, L, red) * inv_n;
        float ds = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * L + sub) * VEC;
            if (active && e < N) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    v[c][k] -= mu0;
                    ds += v[c][k];
                }
            }
        }
        const float dm = ln_sum<BLOCK>(ds, L, red) * inv_n;
        const float mu = mu0 + dm;
        float sq = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * L + sub) * VEC;
            if (active && e < N) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    v[c][k] -= dm;
                    sq = fmaf(v[c][k], v[c][k], sq);
                }
            }
        }
        const float var = ln_sum<BLOCK>(sq, L, red) * inv_n;
        const float rstd = 1.f / sqrtf(var + p.eps);
        float* y = p.Y + r * p.y_ld + (int64_t)g * N;
        const float* ga = p.gamma + (int64_t)g * N;
        const float* be = p.beta + (int64_t)g * N;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * L + sub) * VEC;
            if (active && e < N) {
                float gv[VEC], bv[VEC], z[VEC];
                fx_load<VEC>(ga + e, gv);
                fx_load<VEC>(be + e, bv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    z[k] = fmaf(v[c][k] * rstd, gv[k], bv[k]);
                    if (p.relu) z[k] = fmaxf(z[k], 0.f);
                }
                fx_store<VEC>(y + e, z);
            }
        }
        if (active && sub == 0) {
            p.stats[seg * 2] = mu;
            p.stats[seg * 2 + 1] = rstd;
        }
    }
}

// dX (+)= rstd * (gh - mean gh - xh * mean(gh xh)),  gh = dY * [Y > 0] * gamma,  xh = (x - mu) * rstd
template <int VEC, int CH, bool BLOCK>
__global__ __launch_bounds__(LN_T) void k_ln_bwd(LnArgs p) {
    __shared__ float red[4];
    const int N = p.N, G = p.G, L = BLOCK ? LN_T : p.L;
    const int64_t S = p.rows * G;
    const int per_wg = BLOCK ? 1 : (LN_T / 64) * (64 / L);
    const float inv_n = 1.f / (float)N;
    for (int64_t s0 = (int64_t)blockIdx.x * per_wg; s0 < S; s0 += (int64_t)gridDim.x * per_wg) {
        int64_t seg;
        int sub;
        ln_place<BLOCK>(p, s0, seg, sub);
        const bool active = seg < S;
        const int64_t r = active ? seg / G : 0;
        const int g = active ? (int)(seg - r * G) : 0;
        const float* x = p.X + r * p.x_ld + (int64_t)g * N;
        const float* dy = p.dY + r * p.dy_ld + (int64_t)g * N;
        const float* ga = p.gamma + (int64_t)g * N;
        const float mu = active ? p.stats[seg * 2] : 0.f;
        const float rstd = active ? p.stats[seg * 2 + 1] : 0.f;
        float xh[CH][VEC], gh[CH][VEC];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * L + sub) * VEC;
            if (active && e < N) {
                float gv[VEC];
                fx_load<VEC>(x + e, xh[c]);
                fx_load<VEC>(dy + e, gh[c]);
                fx_load<VEC>(ga + e, gv);
                if (p.relu) {
                    float yv[VEC];
                    fx_load<VEC>(p.Y + r * p.y_ld + (int64_t)g * N + e, yv);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) gh[c][k] = yv[k] > 0.f ? gh[c][k] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    xh[c][k] = (xh[c][k] - mu) * rstd;
                    gh[c][k] *= gv[k];
                    s1 += gh[c][k];
                    s2 = fmaf(gh[c][k], xh[c][k], s2);
                }
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) xh[c][k] = gh[c][k] = 0.f;
            }
        }
        const float m1 = ln_sum<BLOCK>(s1, L, red) * inv_n;
        const float m2 = ln_sum<BLOCK>(s2, L, red) * inv_n;
        float* dx = p.dX + r * p.dx_ld + (int64_t)g * N;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * L + sub) * VEC;
            if (active && e < N) {
                float o[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) o[k] = rstd * (gh[c][k] - m1 - xh[c][k] * m2);
                if (p.dx_acc) {
                    float old[VEC];
                    fx_load<VEC>(dx + e, old);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) o[k] += old[k];
                }
                fx_store<VEC>(dx + e, o);
            }
        }
    }
}

// grid (ceil(G N / 256), nslab): column c of the affine pair over the rows of a slab
__global__ __launch_bounds__(LN_T) void k_ln_dparam(LnArgs p) {
    const int64_t C = (int64_t)p.G * p.N;
    const int64_t c = (int64_t)blockIdx.x * LN_T + threadIdx.x;
    if (c >= C) return;
    const int g = (int)(c / p.N);
    const int64_t r0 = (int64_t)blockIdx.y * p.rows_per_slab;
    const int64_t r1 = r0 + p.rows_per_slab < p.rows ? r0 + p.rows_per_slab : p.rows;
    float dg = 0.f, db = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        float d = p.dY[r * p.dy_ld + c];
        if (p.relu && !(p.Y[r * p.y_ld + c] > 0.f)) d = 0.f;
        const float mu = p.stats[(r * p.G + g) * 2], rstd = p.stats[(r * p.G + g) * 2 + 1];
        dg = fmaf(d, (p.X[r * p.x_ld + c] - mu) * rstd, dg);
        db += d;
    }
    float* part = p.partial + (int64_t)blockIdx.y * 2 * C;
    part[c] = dg;
    part[C + c] = db;
}

// out[r, h] (+)= sum_{k < nb} dM[r, k H + h] * Vmask[r, k H + h]
template <int VEC>
__global__ __launch_bounds__(LN_T) void k_mask_grad(const float* dM, int64_t dm_ld, const float* Vm, int64_t vm_ld,
                                                    int64_t rows, int H, int nb, float* out, int64_t out_ld,
                                                    int acc) {
    const int HC = H / VEC;
    const int64_t total = rows * HC;
    for (int64_t i = (int64_t)blockIdx.x * LN_T + threadIdx.x; i < total; i += (int64_t)gridDim.x * LN_T) {
        const int64_t r = i / HC;
        const int h = (int)(i - r * HC) * VEC;
        float t[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) t[k] = 0.f;
        for (int b = 0; b < nb; ++b) {
            float a[VEC], m[VEC];
            fx_load<VEC>(dM + r * dm_ld + (int64_t)b * H + h, a);
            fx_load<VEC>(Vm + r * vm_ld + (int64_t)b * H + h, m);
#pragma unroll
            for (int k = 0; k < VEC; ++k) t[k] = fmaf(a[k], m[k], t[k]);
        }
        float* o = out + r * out_ld + h;
        if (acc) {
            float old[VEC];
            fx_load<VEC>(o, old);
#pragma unroll
            for (int k = 0; k < VEC; ++k) t[k] += old[k];
        }
        fx_store<VEC>(o, t);
    }
}

// ---------------------------------------------------------------------------------------------------------
template <bool BWD, int VEC, int CH, bool BLOCK>
static void ln_launch_one(unsigned grid, hipStream_t s, const LnArgs& p) {
    if constexpr (BWD) hipLaunchKernelGGL((k_ln_bwd<VEC, CH, BLOCK>), dim3(grid), dim3(LN_T), 0, s, p);
    else hipLaunchKernelGGL((k_ln_fwd<VEC, CH, BLOCK>), dim3(grid), dim3(LN_T), 0, s, p);
}

template <bool BWD>
static int ln_launch(const LnPlan& q, hipStream_t s, LnArgs& p) {
    const int64_t S = p.rows * p.G;
    const int64_t per_wg = q.block ? 1 : (LN_T / 64) * (64 / q.L);
    int64_t grid64 = fx_ceil_div(S, per_wg);
    if (grid64 > LN_MAX_WG) grid64 = LN_MAX_WG;
    const unsigned grid = (unsigned)grid64;
    p.L = q.L;
    const int key = q.vec * 1000 + q.ch * 10 + (q.block ? 1 : 0);
    switch (key) {
    case 4010: ln_launch_one<BWD, 4, 1, false>(grid, s, p); break;
    case 4020: ln_launch_one<BWD, 4, 2, false>(grid, s, p); break;
    case 4040: ln_launch_one<BWD, 4, 4, false>(grid, s, p); break;
    case 4080: ln_launch_one<BWD, 4, 8, false>(grid, s, p); break;
    case 4041: ln_launch_one<BWD, 4, 4, true>(grid, s, p); break;
    case 4081: ln_launch_one<BWD, 4, 8, true>(grid, s, p); break;
    case 1010: ln_launch_one<BWD, 1, 1, false>(grid, s, p); break;
    case 1020: ln_launch_one<BWD, 1, 2, false>(grid, s, p); break;
    case 1040: ln_launch_one<BWD, 1, 4, false>(grid, s, p); break;
    case 1080: ln_launch_one<BWD, 1, 8, false>(grid, s, p); break;
    case 1041: ln_launch_one<BWD, 1, 4, true>(grid, s, p); break;
    case 1081: ln_launch_one<BWD, 1, 8, true>(grid, s, p); break;
    case 1321: ln_launch_one<BWD, 1, 32, true>(grid, s, p); break;
    default:
        fx_set_error("fx_layernorm: no kernel for N=%d (vec %d, chunks %d, block %d)", p.N, q.vec, q.ch, (int)q.block);
        return FX_ERR_INVALID;
    }
    FX_CHECK_LAUNCH();
    return FX_OK;
}

static int ln_check(const char* who, const float* X, int64_t x_ld, int64_t rows, int32_t G, int32_t N) {
    FX_CHECK_ARG(N >= 1 && N <= LN_MAX_N, "%s: N=%d, limit 1 <= N <= 8192", who, N);
    FX_CHECK_ARG(G >= 1 && G <= LN_MAX_G, "%s: G=%d, limit 1 <= G <= 64", who, G);
    FX_CHECK_ARG(rows >= 0, "%s: rows=%lld", who, (long long)rows);
    FX_CHECK_ARG(rows == 0 || X, "%s: null X", who);
    FX_CHECK_ARG(x_ld >= (int64_t)G * N, "%s: row stride %lld < G*N", who, (long long)x_ld);
    return FX_OK;
}

extern "C" int64_t fx_layernorm_workspace_floats(int64_t rows, int32_t G, int32_t N) {
    if (rows < 1 || G < 1 || N < 1) return 0;
    const int64_t C = (int64_t)G * N;
    return (int64_t)ln_slabs(rows, C).nslab * 2 * C;
}

extern "C" int fx_layernorm_fwd(const float* X, int64_t x_ld, int64_t rows, int32_t G, int32_t N,
                                const float* gamma, const float* beta, float eps, int32_t relu, float* Y,
                                int64_t y_ld, int64_t y_col, float* stats, fx_stream_t stream) {
    if (int st = ln_check("fx_layernorm_fwd", X, x_ld, rows, G, N)) return st;
    FX_CHECK_ARG(rows == 0 || (gamma && beta && Y && stats), "fx_layernorm_fwd: null gamma / beta / Y / stats");
    FX_CHECK_ARG(y_col >= 0 && y_ld >= y_col + (int64_t)G * N, "fx_layernorm_fwd: Y row stride %lld < y_col + G*N",
                 (long long)y_ld);
    if (rows == 0) return FX_OK;
    LnArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.rows = rows; p.G = G; p.N = N; p.relu = relu ? 1 : 0;
    p.gamma = gamma; p.beta = beta; p.eps = eps;
    p.Y = Y + y_col; p.y_ld = y_ld; p.stats = stats;
    const bool vec4 = N % 4 == 0 && fx_vec_ok(X, x_ld) && fx_vec_ok(p.Y, y_ld) && fx_al16(gamma) && fx_al16(beta);
    return ln_launch<false>(ln_plan(N, vec4), fx_hip_stream(stream), p);
}

extern "C" int fx_layernorm_bwd(const float* X, int64_t x_ld, int64_t rows, int32_t G, int32_t N,
                                const float* gamma, int32_t relu, const float* Y, int64_t y_ld, int64_t y_col,
                                const float* stats, const float* dY, int64_t dy_ld, int64_t dy_col, float* dX,
                                int64_t dx_ld, int32_t dx_accumulate, float* dgamma, float* dbeta,
                                float* workspace, fx_stream_t stream) {
    if (int st = ln_check("fx_layernorm_bwd", X, x_ld, rows, G, N)) return st;
    FX_CHECK_ARG(rows > 0, "fx_layernorm_bwd: rows=%lld", (long long)rows);
    FX_CHECK_ARG(gamma && stats && dY && dX && dgamma && dbeta && workspace,
                 "fx_layernorm_bwd: null gamma / stats / dY / dX / dgamma / dbeta / workspace");
    FX_CHECK_ARG(!relu || Y, "fx_layernorm_bwd: the fused ReLU's mask is read from Y: null Y");
    const int64_t C = (int64_t)G * N;
    FX_CHECK_ARG(!relu || (y_col >= 0 && y_ld >= y_col + C), "fx_layernorm_bwd: Y row stride %lld < y_col + G*N",
                 (long long)y_ld);
    FX_CHECK_ARG(dy_col >= 0 && dy_ld >= dy_col + C, "fx_layernorm_bwd: dY row stride %lld < dy_col + G*N",
                 (long long)dy_ld);
    FX_CHECK_ARG(dx_ld >= C, "fx_layernorm_bwd: dX row stride %lld < G*N", (long long)dx_ld);
    LnArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.rows = rows; p.G = G; p.N = N; p.relu = relu ? 1 : 0;
    p.gamma = gamma;
    p.Y = relu ? const_cast<float*>(Y) + y_col : nullptr; p.y_ld = y_ld;
    p.stats = const_cast<float*>(stats);
    p.dY = dY + dy_col; p.dy_ld = dy_ld;
    p.dX = dX; p.dx_ld = dx_ld; p.dx_acc = dx_accumulate ? 1 : 0;
    const LnSlabs sl = ln_slabs(rows, C);
    p.partial = workspace; p.rows_per_slab = sl.rows_per_slab;
    const bool vec4 = N % 4 == 0 && fx_vec_ok(X, x_ld) && fx_vec_ok(p.dY, dy_ld) && fx_vec_ok(dX, dx_ld) &&
                      fx_al16(gamma) && (!relu || fx_vec_ok(p.Y, y_ld));
    hipStream_t s = fx_hip_stream(stream);
    if (int st = ln_launch<true>(ln_plan(N, vec4), s, p)) return st;
    hipLaunchKernelGGL(k_ln_dparam, dim3((unsigned)fx_ceil_div(C, LN_T), (unsigned)sl.nslab), dim3(LN_T), 0, s, p);
    FX_CHECK_LAUNCH();
    // partial[s] = [dgamma | dbeta]: the slabs in their order
    return fx_rowsum<float, FX_ROWS_SERIAL>(s, workspace, sl.nslab, 2 * C, fx_rowsum_out(dgamma, C, dbeta, C));
}

extern "C" int fx_mask_grad(const float* dM, int64_t dm_ld, const float* Vmask, int64_t vm_ld, int64_t rows,
                            int32_t H, int32_t nb, float* out, int64_t out_ld, int32_t accumulate,
                            fx_stream_t stream) {
    FX_CHECK_ARG(H >= 1 && nb >= 1, "fx_mask_grad: H=%d nb=%d", H, nb);
    FX_CHECK_ARG(rows >= 0, "fx_mask_grad: rows=%lld", (long long)rows);
    FX_CHECK_ARG(rows == 0 || (dM && Vmask && out), "fx_mask_grad: null dM / Vmask / out");
    FX_CHECK_ARG(dm_ld >= (int64_t)nb * H && vm_ld >= (int64_t)nb * H && out_ld >= H,
                 "fx_mask_grad: a row stride is smaller than its row (%lld, %lld, %lld)", (long long)dm_ld,
                 (long long)vm_ld, (long long)out_ld);
    if (rows == 0) return FX_OK;
    const bool vec4 = H % 4 == 0 && fx_vec_ok(dM, dm_ld) && fx_vec_ok(Vmask, vm_ld) && fx_vec_ok(out, out_ld);
    const int64_t total = rows * (vec4 ? H / 4 : H);
    int64_t grid = fx_ceil_div(total, LN_T);
    if (grid > LN_MAX_WG) grid = LN_MAX_WG;
    hipStream_t s = fx_hip_stream(stream);
    if (vec4)
        hipLaunchKernelGGL(k_mask_grad<4>, dim3((unsigned)grid), dim3(LN_T), 0, s, dM, dm_ld, Vmask, vm_ld, rows,
                           (int)H, (int)nb, out, out_ld, accumulate ? 1 : 0);
    else
        hipLaunchKernelGGL(k_mask_grad<1>, dim3((unsigned)grid), dim3(LN_T), 0, s, dM, dm_ld, Vmask, vm_ld, rows,
                           (int)H, (int)nb, out, out_ld, accumulate ? 1 : 0);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
