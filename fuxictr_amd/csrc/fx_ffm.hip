// fx_ffm.hip — the field-aware interaction of FFMv2 (model_zoo/FFM/src/FFMv2.py:78-91) and ONNv2 (also NFFM / DeepFFM;
// model_zoo/ONN/ONN_torch/src/ONNv2.py:88-109) fused over the gather record.  A field keeps one D-vector per partner
// field: the record row of a sample is E[i][c][:], field i, slot c, F * C * D floats, and the pair term is
// <E[i][s_i(j)], E[j][s_j(i)]> for i < j in the row-major upper-triangle order of torch.triu_indices (fx_pair_off).
//     ONN: C = F,     s_i(j) = j; slot i of field i is the field's own ("diagonal") vector.
//          out row [F*D + P] = [E[0][0] .. E[F-1][F-1] | the P pair terms]: the first DNN layer's input, written in
//          place (the reference's two masked_select and its cat).
//     FFM: C = F - 1, s_i(j) = j - 1 for j > i, j for j < i.   out[b] = sum of the P pair terms (+ addend[b]).
// Backward: every element of dX has exactly one contributor, dX[i][s_i(j)] = g_p E[j][s_j(i)] (g_p the pair's column
// of the ONN gradient row, g[b] in FFM mode; ONN: dX[i][i] = the diagonal columns of the row): plain stores, no
// atomics, nothing recomputed, nothing kept but X.  (i, c) -> j -> p is a closed form.  fp32, every sum in a fixed order.
//
// Matrix instructions do not fit: the product is the Hadamard product of a sample's F x C block of vectors with its
// own transpose, reduced over D <= 8 or so; no operand is shared between lanes, so an MFMA would have nothing to
// broadcast.  One multiply-add per element read: the kernels are built to stream the record.
//
//   k_ffm<VEC, GW, BWD>: a workgroup of 256 threads owns a tile of T whole samples (fx_ffm_tile_rows) and walks the tiles
//       with a grid stride (at most FFM_MAX_WG workgroups).  A sample's block is contiguous in memory; it is staged in
//       LDS with coalesced loads, GW = 4: 16-byte loads (base and row stride 16-byte aligned and F*C*D % 4 == 0),
//       GW = 1: 4-byte loads (odd widths, strided record views).  In LDS the row of a field is RS = C*D rounded up to
//       VEC floats, plus VEC more where RS / VEC would be even: a pair reads [i][s(j)] and [j][s(i)], the block and its
//       transpose, and lanes that walk j at a fixed i step RS floats in the transposed read; with RS / VEC odd they
//       fall on different banks.  VEC = 4 (ds_read_b128) when D % 4 == 0, 2 (ds_read_b64) when D % 2 == 0, else 1.
//       T is what fits in HALF the 160 KB of LDS (two workgroups per CU: one stages while the other computes), at
//       most 32; a shape whose single sample needs more than half takes the whole LDS.
//         forward : an item is (sample t, pair p), lanes take consecutive p: the (i, j) of p from a table in LDS built
//                   once per workgroup, the dot in the order d = 0 .. D-1.  ONN: the store of the pair columns is
//                   coalesced; the diagonal vectors are copied by a second walk.  FFM: per sample every thread sums
//                   its pairs p = tid, tid + 256, .., the wave by the butterfly, the waves in wave order.
//         backward: the tile and the samples' g rows are staged; threads walk dX in memory order in chunks of GW (or
//                   VEC) floats, each VEC-vector of a chunk finds its (i, c), reads the partner vector from LDS
//                   transposed and g_p from the staged row; 16-byte stores when GW = 4.
// One launch per direction.  Built without packed fp32 ops, as the neighbouring files.
#include "fx_common.h"

#define FFM_ONN 0
#define FFM_FFM 1
#define FFM_NT 256
#define FFM_MAX_F 64
#define FFM_MAX_CD 256             // C * D: the row width of fx_emb_gather_fwd
#define FFM_MAX_WG 512
#define FFM_MAX_T 32
#define FFM_LDS_MAX (160 * 1024)

struct FfmArgs {
    const float* X; int64_t ldx;        // [B, F*C*D]
    const float* addend;                // [B] or null                        forward, FFM
    float* out; int64_t ldo;            // ONN [B, F*D + P], FFM [B, 1]       forward
    const float* g; int64_t ldg;        // ONN [B, F*D + P], FFM [B, 1]       backward
    float* dX; int64_t lddx;            // [B, F*C*D]
    int64_t B;
    int F, C, D, P, mode;
    int T, RS;                          // samples of a tile; floats of a field's row in LDS
};

static inline int ffm_vec(int D) { return D % 4 == 0 ? 4 : (D % 2 == 0 ? 2 : 1); }
static inline int ffm_slots(int mode, int F) { return mode == FFM_ONN ? F : F - 1; }
static inline int ffm_row_stride(int CD, int vec) {
    int rs = (CD + vec - 1) / vec * vec;
    if ((rs / vec) % 2 == 0) rs += vec;
    return rs;
}
// LDS, floats: xs [T][F * RS] | gs [T][GS] | red [NT / 64][T] | pair table [P up to 4], GS = F*D + P (ONN), 1 (FFM)
static inline int ffm_g_floats(int mode, int F, int D) { return mode == FFM_ONN ? F * D + F * (F - 1) / 2 : 1; }
static inline int ffm_sample_floats(int mode, int F, int D) {
    const int CD = ffm_slots(mode, F) * D;
    return F * ffm_row_stride(CD, ffm_vec(D)) + ffm_g_floats(mode, F, D) + FFM_NT / 64;
}
static inline int ffm_fixed_floats(int F) { return (F * (F - 1) / 2 + 3) / 4 * 4; }
static inline int ffm_tile(int mode, int F, int D) {
    const int per = ffm_sample_floats(mode, F, D), fixed = ffm_fixed_floats(F);
    // (FX_FFM_TILE_KB: the experiment switch behind DESIGN.md's half-against-whole measurement)
    static const int kb = fx_env_int("FX_FFM_TILE_KB", FFM_LDS_MAX / 2048);
    int T = ((kb < 1 ? 1 : kb > 160 ? 160 : kb) * 256 - fixed) / per;     // half the LDS unless told otherwise
    if (T < 1) T = (FFM_LDS_MAX / 4 - fixed) / per;           // one sample needs more: the whole
    return T > FFM_MAX_T ? FFM_MAX_T : T;
}
static inline bool ffm_in_envelope(int mode, int F, int D) {
    return (mode == FFM_ONN || mode == FFM_FFM) && F >= 2 && F <= FFM_MAX_F && D >= 1 &&
           (int64_t)ffm_slots(mode, F) * D <= FFM_MAX_CD;
}

// the tile's rows [b0, b0 + rows) of X into xs[t][i * RS + r], r the float within field i's C*D
template <int GW>
__device__ __forceinline__ void ffm_stage(const FfmArgs& a, float* xs, int64_t b0, int rows, int tid) {
    const int CD = a.C * a.D, N = a.F * CD, RS = a.RS, SS = a.F * RS;
    if (GW == 4) {
        const int n4 = N / 4;
        const bool rowvec = CD % 4 == 0 && RS % 4 == 0;
#pragma unroll 4
        for (int idx = tid; idx < rows * n4; idx += FFM_NT) {
            const int t = idx / n4, q = (idx - t * n4) * 4;
            const float4 v = *reinterpret_cast<const float4*>(a.X + (b0 + t) * a.ldx + q);
            int i = q / CD, r = q - i * CD;
            float* dst = xs + t * SS;
            if (rowvec) {
                *reinterpret_cast<float4*>(dst + i * RS + r) = v;
            } else {
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    dst[i * RS + r] = e[k];
                    if (++r == CD) { r = 0; ++i; }
                }
            }
        }
    } else {
#pragma unroll 4
        for (int idx = tid; idx < rows * N; idx += FFM_NT) {
            const int t = idx / N, q = idx - t * N;
            const int i = q / CD, r = q - i * CD;
            xs[t * SS + i * RS + r] = a.X[(b0 + t) * a.ldx + q];
        }
    }
}

template <int VEC>
__device__ __forceinline__ float ffm_dot(const float* u, const float* v, int D) {
    float acc = 0.f;
    for (int d = 0; d < D; d += VEC) {
        float x[VEC], y[VEC];
        fx_load<VEC>(u + d, x);
        fx_load<VEC>(v + d, y);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc = fmaf(x[k], y[k], acc);
    }
    return acc;
}

// grid: min(tiles, FFM_MAX_WG) workgroups of FFM_NT threads; dynamic LDS 4 * (T * ffm_sample_floats + ffm_fixed_floats)
template <int VEC, int GW, bool BWD>
__global__ __launch_bounds__(FFM_NT) void k_ffm(FfmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F, C = a.C, D = a.D, P = a.P, T = a.T, RS = a.RS;
    const int CD = C * D, FD = F * D, SS = F * RS;
    const bool onn = a.mode == FFM_ONN;
    const int GS = onn ? FD + P : 1;
    float* xs = smem;
    float* gs = xs + T * SS;
    float* red = gs + T * GS;
    int* tab = reinterpret_cast<int*>(red + (FFM_NT / 64) * T);
    if (!BWD) {
        // pair p -> i | j << 8; the first tile's barrier publishes it
        for (int i = tid; i < F - 1; i += FFM_NT) {
            const int p0 = fx_pair_off(i, F);
            for (int j = i + 1; j < F; ++j) tab[p0 + j - i - 1] = i | (j << 8);
        }
    }
    const int64_t tiles = (a.B + T - 1) / T;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * T;
        const int rows = a.B - b0 < T ? (int)(a.B - b0) : T;
        __syncthreads();                        // the last tile's readers are done
        ffm_stage<GW>(a, xs, b0, rows, tid);
        if (BWD) {
            if (onn) {
                for (int idx = tid; idx < rows * GS; idx += FFM_NT) {
                    const int t = idx / GS, c = idx - t * GS;
                    gs[idx] = a.g[(b0 + t) * a.ldg + c];
                }
            } else if (tid < rows) {
                gs[tid] = a.g[(b0 + tid) * a.ldg];
            }
        }
        __syncthreads();
        if (!BWD) {
            if (onn) {
                for (int idx = tid; idx < rows * P; idx += FFM_NT) {
                    const int t = idx / P, p = idx - t * P;
                    const int ij = tab[p], i = ij & 0xff, j = ij >> 8;
                    const float* x = xs + t * SS;
                    a.out[(b0 + t) * a.ldo + FD + p] = ffm_dot<VEC>(x + i * RS + j * D, x + j * RS + i * D, D);
                }
                for (int idx = tid; idx < rows * FD; idx += FFM_NT) {
                    const int t = idx / FD, r = idx - t * FD, i = r / D;
                    a.out[(b0 + t) * a.ldo + r] = xs[t * SS + i * RS + i * D + (r - i * D)];
                }
            } else {
                for (int t = 0; t < rows; ++t) {
                    const float* x = xs + t * SS;
                    float acc = 0.f;
                    for (int p = tid; p < P; p += FFM_NT) {
                        const int ij = tab[p], i = ij & 0xff, j = ij >> 8;
                        acc += ffm_dot<VEC>(x + i * RS + (j - 1) * D, x + j * RS + i * D, D);
                    }
                    const float s = fx_wave_sum(acc);
                    if (lane == 0) red[wave * T + t] = s;
                }
                __syncthreads();
                if (tid < rows) {
                    float s = 0.f;
                    for (int w = 0; w < FFM_NT / 64; ++w) s += red[w * T + tid];
                    if (a.addend) s += a.addend[b0 + tid];
                    a.out[(b0 + tid) * a.ldo] = s;
                }
            }
        } else {
            constexpr int CW = GW == 4 ? 4 : VEC;       // floats of a thread's chunk of dX
            const int nch = F * CD / CW;
            for (int idx = tid; idx < rows * nch; idx += FFM_NT) {
                const int t = idx / nch, q = (idx - t * nch) * CW;
                const float* x = xs + t * SS;
                float v[CW];
#pragma unroll
                for (int s = 0; s < CW / VEC; ++s) {
                    const int qq = q + s * VEC;
                    const int i = qq / CD, r = qq - i * CD, c = r / D, d0 = r - c * D;
                    // the partner field j, the slot that field keeps for i, and the pair's gradient
                    const int j = onn ? c : (c < i ? c : c + 1);
                    const int sl = onn ? i : (i < j ? i : i - 1);
                    float e[VEC], gp = 1.f;
                    if (j == i) {                               // (ONN) the diagonal columns pass through
#pragma unroll
                        for (int k = 0; k < VEC; ++k) e[k] = gs[t * GS + i * D + d0 + k];
                    } else {
                        const int lo = j < i ? j : i, hi = j < i ? i : j;
                        gp = onn ? gs[t * GS + FD + fx_pair_off(lo, F) + hi - lo - 1] : gs[t];
                        fx_load<VEC>(x + j * RS + sl * D + d0, e);
                    }
#pragma unroll
                    for (int k = 0; k < VEC; ++k) v[s * VEC + k] = gp * e[k];
                }
                float* dst = a.dX + (b0 + t) * a.lddx + q;
                if constexpr (GW == 4) {
                    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < CW; ++k) dst[k] = v[k];
                }
            }
        }
    }
}

static int ffm_check(const char* who, int32_t mode, int64_t B, int32_t F, int32_t D) {
    FX_CHECK_ARG(mode == FFM_ONN || mode == FFM_FFM, "%s: mode=%d, not 0 (ONN) or 1 (FFM)", who, mode);
    FX_CHECK_ARG(F >= 2 && F <= FFM_MAX_F, "%s: F=%d, limit 2 <= F <= %d", who, F, FFM_MAX_F);
    FX_CHECK_ARG(D >= 1, "%s: D=%d, limit D >= 1", who, D);
    FX_CHECK_ARG((int64_t)ffm_slots(mode, F) * D <= FFM_MAX_CD, "%s: C*D=%lld, limit %d (the gather's row width)", who,
                 (long long)ffm_slots(mode, F) * D, FFM_MAX_CD);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    return FX_OK;
}

template <bool BWD>
static int ffm_launch(FfmArgs& p, bool vec4, hipStream_t s) {
    static const hipError_t lds_ok[6] = {
        fx_allow_lds(k_ffm<4, 4, BWD>, FFM_LDS_MAX), fx_allow_lds(k_ffm<4, 1, BWD>, FFM_LDS_MAX),
        fx_allow_lds(k_ffm<2, 4, BWD>, FFM_LDS_MAX), fx_allow_lds(k_ffm<2, 1, BWD>, FFM_LDS_MAX),
        fx_allow_lds(k_ffm<1, 4, BWD>, FFM_LDS_MAX), fx_allow_lds(k_ffm<1, 1, BWD>, FFM_LDS_MAX)};
    const int vec = ffm_vec(p.D);
    p.C = ffm_slots(p.mode, p.F);
    p.P = p.F * (p.F - 1) / 2;
    p.T = ffm_tile(p.mode, p.F, p.D);
    p.RS = ffm_row_stride(p.C * p.D, vec);
    FX_CHECK_HIP(lds_ok[(vec == 4 ? 0 : vec == 2 ? 2 : 4) + (vec4 ? 0 : 1)]);
    const size_t lds = 4 * ((size_t)p.T * ffm_sample_floats(p.mode, p.F, p.D) + ffm_fixed_floats(p.F));
    const int64_t tiles = fx_ceil_div(p.B, p.T);
    const dim3 grid((unsigned)(tiles < FFM_MAX_WG ? tiles : FFM_MAX_WG)), block(FFM_NT);
    if (vec == 4 && vec4) hipLaunchKernelGGL((k_ffm<4, 4, BWD>), grid, block, lds, s, p);
    else if (vec == 4) hipLaunchKernelGGL((k_ffm<4, 1, BWD>), grid, block, lds, s, p);
    else if (vec == 2 && vec4) hipLaunchKernelGGL((k_ffm<2, 4, BWD>), grid, block, lds, s, p);
    else if (vec == 2) hipLaunchKernelGGL((k_ffm<2, 1, BWD>), grid, block, lds, s, p);
    else if (vec4) hipLaunchKernelGGL((k_ffm<1, 4, BWD>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((k_ffm<1, 1, BWD>), grid, block, lds, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" void fx_ffm_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = 2;                  // F at least
    limits[1] = FFM_MAX_F;
    limits[2] = FFM_MAX_CD;         // C * D at most
    limits[3] = FFM_MAX_WG;         // workgroups of a launch at most
    limits[4] = FFM_MAX_T;          // samples of a tile at most
}

extern "C" int32_t fx_ffm_tile_rows(int32_t mode, int32_t F, int32_t D) {
    return ffm_in_envelope(mode, F, D) ? ffm_tile(mode, F, D) : 0;
}

extern "C" int fx_ffm_fwd(const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D, int32_t mode,
                          const float* addend, float* out, int64_t ldo, fx_stream_t stream) {
    const char* who = "fx_ffm_fwd";
    if (int st = ffm_check(who, mode, B, F, D)) return st;
    const int64_t N = (int64_t)F * ffm_slots(mode, F) * D;
    const int64_t W = mode == FFM_ONN ? (int64_t)ffm_g_floats(mode, F, D) : 1;
    FX_CHECK_ARG(ldx >= N, "%s: X row stride %lld < F*C*D", who, (long long)ldx);
    FX_CHECK_ARG(ldo >= W, "%s: out row stride %lld < %lld", who, (long long)ldo, (long long)W);
    FX_CHECK_ARG(mode == FFM_FFM || !addend, "%s: an addend in ONN mode", who);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(X && out, "%s: null X / out", who);
    FfmArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.ldx = ldx; p.addend = addend; p.out = out; p.ldo = ldo;
    p.B = B; p.F = F; p.D = D; p.mode = mode;
    return ffm_launch<false>(p, N % 4 == 0 && fx_vec_ok(X, ldx), fx_hip_stream(stream));
}

extern "C" int fx_ffm_bwd(const float* g, int64_t ldg, const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D,
                          int32_t mode, float* dX, int64_t lddx, fx_stream_t stream) {
    const char* who = "fx_ffm_bwd";
    if (int st = ffm_check(who, mode, B, F, D)) return st;
    const int64_t N = (int64_t)F * ffm_slots(mode, F) * D;
    const int64_t W = mode == FFM_ONN ? (int64_t)ffm_g_floats(mode, F, D) : 1;
    FX_CHECK_ARG(ldx >= N, "%s: X row stride %lld < F*C*D", who, (long long)ldx);
    FX_CHECK_ARG(lddx >= N, "%s: dX row stride %lld < F*C*D", who, (long long)lddx);
    FX_CHECK_ARG(ldg >= W, "%s: g row stride %lld < %lld", who, (long long)ldg, (long long)W);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(g && X && dX, "%s: null g / X / dX", who);
    FfmArgs p;
    memset(&p, 0, sizeof(p));
    p.g = g; p.ldg = ldg; p.X = X; p.ldx = ldx; p.dX = dX; p.lddx = lddx;
    p.B = B; p.F = F; p.D = D; p.mode = mode;
    return ffm_launch<true>(p, N % 4 == 0 && fx_vec_ok(X, ldx) && fx_vec_ok(dX, lddx), fx_hip_stream(stream));
}
