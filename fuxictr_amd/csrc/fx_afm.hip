// fx_afm.hip — AFM's pairwise attention (model_zoo/AFM/src/AFM.py:84-93) fused over the gather record.
// For a sample with fields x_0..x_{F-1} (D floats each) and every pair p = (i, j), i < j, in the row-major
// upper-triangle order of torch.triu_indices (inner_product.py: "elementwise_product"):
//     e_p = x_i * x_j                                   (D)
//     z_p = W1 e_p + b1,  h_p = relu(z_p)               (A)     attention.0 / attention.1
//     s_p = w2 . h_p                                            attention.2
//     a   = softmax over p of s                                 attention.3
//     out = sum_p a_p t_p (+ addend),  t_p = wp . e_p           weight_p; the addend is lr_layer(X)
// Per pair only the two scalars s_p and t_p matter: no [B, P, D] or [B, P, A] tensor exists anywhere.
//
//   fx_afm_attn_fwd : out [B] and the stats row (softmax max m, denominator sum_p exp(s_p - m), y = out without
//                     the addend) per sample.  A lane owns the pairs lane, lane + 64, ...; it carries a running
//                     max / denominator / numerator (the max is subtracted before every exp: scores of +-80 stay
//                     finite) and the wave combines the 64 of them once per sample.
//   fx_afm_attn_bwd : recomputes s_p, t_p and the ReLU mask from the record; with g = dout:
//                     dt_p = g a_p, ds_p = g a_p (t_p - y), dz_p = ds_p w2 [z_p > 0], de_p = dt_p wp + W1^T dz_p,
//                     dx_i = sum_{j != i} de_(ij) x_j, dW1 = sum dz_p e_p^T, db1 = sum dz_p, dw2 = sum ds_p h_p,
//                     dwp = sum dt_p e_p.  Phases per sample: (A) lane = pair: ds_p, dt_p and the mask bits go
//                     to LDS; (B) lane = pair, chunk of 8 hidden units outermost: dw2 and db1, one wave sum per
//                     hidden unit; (C) lane = pair, tiles of 8 hidden units by 8 dimensions of dW1 (and dwp) in
//                     registers, one wave sum per element; (D) lane = element (i, d) of the record, a loop over
//                     j != i: ordered pairs, so dx_i has ONE owner.  Every sum has a fixed order (a lane's own
//                     pairs in order, then the butterfly over the lanes): no atomics anywhere, LDS included, and
//                     two launches on the same inputs give the same bits.  The weight gradients are kept per wave
//                     in LDS over the workgroup's samples, summed over its waves in wave order and written as the
//                     workgroup's row of `partial`; fx_colsum reduces the rows.
//
// One wave per sample, AF waves per workgroup (fx_afm_attn_tile_rows: 4, fewer where the LDS image of the
// backward would not fit); a workgroup strides over the tiles of AF samples.  LDS (floats): the weights once per
// workgroup — W1 transposed [D][A8 + 4] (A8 = A rounded up to 8, zero filled: a lane reads 8 hidden units of one d
// as two 16-byte words, every lane the same address in the forward = a broadcast; the + 4 keeps the 16 lanes of a
// 16-byte read on different banks where the lanes differ in d), in the backward also W1 * w2 in that layout, b1,
// w2, wp, the pair table (i << 16 | j) — and per wave the sample's fields [F][D | 1] (the odd field stride keeps
// the 4-byte reads of x_j of consecutive j on different banks), in the backward also 4 words per pair and the
// weight-gradient accumulators.  fp32 throughout.
#include "fx_common.h"

#define AF_WAVES 4
#define AF_CHUNK 8
#define AF_MAX_FD 4096
#define AF_MAX_P 4096
#define AF_MAX_D 64
#define AF_MAX_A 64
#define AF_MAX_WG 1024            // 4 workgroups per CU
#define AF_LDS_MAX (160 * 1024)
#define AF_STATS 3                // m, denominator, y

struct AfArgs {
    const float* X; int64_t ldx;        // [B, F*D]
    const float *W1, *b1, *w2, *wp;     // [A, D], [A], [A], [D]
    const float* addend;                // [B] or null
    float* out;                         // [B]                       forward
    float* stats;                       // [B, AF_STATS]             written forward, read backward
    const float* g;                     // [B]                       backward
    float* dX; int64_t lddx;            // [B, F*D]
    float* partial;                     // [grid, n]
    int64_t B;
    int F, D, A, P, nw;
};

// the LDS image, in floats
struct AfLds {
    int Dp, A8, AS;                     // field stride, padded hidden width, row stride of the transposed weights
    int wt, wwt, b1, w2, wp, tab;       // shared offsets
    int shared;                         // floats before the first wave's block
    int xs, ds, dt, mlo, mhi, wacc;     // offsets inside a wave's block
    int per_wave, n;                    // n: floats of weight gradient = A*D + 2 A + D
};

__host__ __device__ inline AfLds af_lds(int F, int D, int A, int P, bool bwd) {
    AfLds L;
    L.Dp = D | 1;
    L.A8 = (A + AF_CHUNK - 1) / AF_CHUNK * AF_CHUNK;
    L.AS = L.A8 + 4;
    L.n = A * D + 2 * A + D;
    int o = 0;
    L.wt = o; o += D * L.AS;
    L.wwt = o; o += bwd ? D * L.AS : 0;
    L.b1 = o; o += L.A8;
    L.w2 = o; o += L.A8;
    L.wp = o; o += (D + 3) / 4 * 4;
    L.tab = o; o += (P + 3) / 4 * 4;
    L.shared = o;
    o = 0;
    L.xs = o; o += (F * L.Dp + 3) / 4 * 4;
    L.ds = o; o += bwd ? P : 0;
    L.dt = o; o += bwd ? P : 0;
    L.mlo = o; o += bwd ? P : 0;
    L.mhi = o; o += bwd ? P : 0;
    L.wacc = o; o += bwd ? L.n : 0;
    L.per_wave = (o + 3) / 4 * 4;
    return L;
}

static inline size_t af_lds_bytes(int F, int D, int A, int P, bool bwd, int nw) {
    const AfLds L = af_lds(F, D, A, P, bwd);
    return 4 * ((size_t)L.shared + (size_t)nw * L.per_wave);
}

// waves (= samples) per workgroup: the most of 4, 2, 1 whose backward image fits; the forward uses the same
static inline int af_waves(int F, int D, int A, int P) {
    for (int nw = AF_WAVES; nw > 1; nw /= 2)
        if (af_lds_bytes(F, D, A, P, true, nw) <= AF_LDS_MAX) return nw;
    return 1;
}

// weights and pair table -> LDS, all threads of the workgroup; the caller synchronises
__device__ __forceinline__ void af_stage_weights(const AfArgs& p, const AfLds& L, float* smem, bool bwd) {
    const int T = blockDim.x, t = threadIdx.x;
    for (int e = t; e < p.D * L.AS; e += T) {
        const int d = e / L.AS, a = e - d * L.AS;
        const float w = a < p.A ? p.W1[(int64_t)a * p.D + d] : 0.f;
        smem[L.wt + e] = w;
        if (bwd) smem[L.wwt + e] = a < p.A ? w * p.w2[a] : 0.f;
    }
    for (int a = t; a < L.A8; a += T) {
        smem[L.b1 + a] = a < p.A ? p.b1[a] : 0.f;
        smem[L.w2 + a] = a < p.A ? p.w2[a] : 0.f;
    }
    for (int d = t; d < p.D; d += T) smem[L.wp + d] = p.wp[d];
    uint32_t* tab = reinterpret_cast<uint32_t*>(smem + L.tab);
    for (int i = t; i < p.F - 1; i += T) {
        const int off = fx_pair_off(i, p.F);
        for (int j = i + 1; j < p.F; ++j) tab[off + j - i - 1] = ((uint32_t)i << 16) | (uint32_t)j;
    }
}

// the sample's F*D floats -> xs [F][Dp], one wave
template <int VEC>
__device__ __forceinline__ void af_stage_x(const float* x, float* xs, int FD, int D, int Dp, int lane) {
    for (int c = lane * VEC; c < FD; c += 64 * VEC) {
        float v[VEC];
        fx_load<VEC>(x + c, v);
        const int f = c / D, d = c - f * D;         // (VEC = 4 only with D % 4 == 0: the 4 floats are one field's)
#pragma unroll
        for (int k = 0; k < VEC; ++k) xs[f * Dp + d + k] = v[k];
    }
}

// z[k] = b1[a0 + k] + sum_d W1[a0 + k, d] x_i[d] x_j[d] for the 8 hidden units of a chunk; with T also
// t = sum_d wp[d] x_i[d] x_j[d]
template <bool T>
__device__ __forceinline__ void af_zchunk(const float* xi, const float* xj, const float* wt, int AS, int D,
                                          const float* b1s, const float* wps, int a0, float (&z)[AF_CHUNK],
                                          float& t) {
#pragma unroll
    for (int k = 0; k < AF_CHUNK; ++k) z[k] = b1s[a0 + k];
    const float* w = wt + a0;
    for (int d = 0; d < D; ++d) {
        const float e = xi[d] * xj[d];
        const float4 w0 = *reinterpret_cast<const float4*>(w + d * AS);
        const float4 w1 = *reinterpret_cast<const float4*>(w + d * AS + 4);
        z[0] = fmaf(w0.x, e, z[0]); z[1] = fmaf(w0.y, e, z[1]); z[2] = fmaf(w0.z, e, z[2]); z[3] = fmaf(w0.w, e, z[3]);
        z[4] = fmaf(w1.x, e, z[4]); z[5] = fmaf(w1.y, e, z[5]); z[6] = fmaf(w1.z, e, z[6]); z[7] = fmaf(w1.w, e, z[7]);
        if (T) t = fmaf(wps[d], e, t);
    }
}

// s_p, t_p and the bits [z_p[a] > 0] of one pair
__device__ __forceinline__ void af_pair(const float* smem, const AfLds& L, const float* xs, uint32_t ij, int D,
                                        float& s, float& t, uint32_t& mlo, uint32_t& mhi) {
    const float* xi = xs + (ij >> 16) * L.Dp;
    const float* xj = xs + (ij & 0xffffu) * L.Dp;
    s = 0.f; t = 0.f; mlo = 0u; mhi = 0u;
    for (int a0 = 0; a0 < L.A8; a0 += AF_CHUNK) {
        float z[AF_CHUNK];
        if (a0 == 0) af_zchunk<true>(xi, xj, smem + L.wt, L.AS, D, smem + L.b1, smem + L.wp, a0, z, t);
        else af_zchunk<false>(xi, xj, smem + L.wt, L.AS, D, smem + L.b1, smem + L.wp, a0, z, t);
        uint32_t bits = 0u;
#pragma unroll
        for (int k = 0; k < AF_CHUNK; ++k) {
            s = fmaf(smem[L.w2 + a0 + k], fmaxf(z[k], 0.f), s);
            bits |= (z[k] > 0.f ? 1u : 0u) << k;
        }
        if (a0 < 32) mlo |= bits << a0;
        else mhi |= bits << (a0 - 32);
    }
}

// grid: min(tiles, AF_MAX_WG) workgroups of nw waves; dynamic LDS af_lds_bytes(.., false, nw)
template <int VEC>
__global__ __launch_bounds__(64 * AF_WAVES) void k_afm_attn_fwd(AfArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AfLds L = af_lds(p.F, p.D, p.A, p.P, false);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* xs = smem + L.shared + w * L.per_wave + L.xs;
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(smem + L.tab);
    af_stage_weights(p, L, smem, false);
    const int64_t tiles = (p.B + p.nw - 1) / p.nw;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b = tile * p.nw + w;
        const bool act = b < p.B;
        __syncthreads();                    // the weights are staged; the last sample's readers are done
        if (act) af_stage_x<VEC>(p.X + b * p.ldx, xs, p.F * p.D, p.D, L.Dp, lane);
        __syncthreads();
        if (!act) continue;
        float m = -INFINITY, den = 0.f, num = 0.f;
        for (int p0 = 0; p0 < p.P; p0 += 64) {
            const int q = p0 + lane;
            if (q < p.P) {
                float s, t;
                uint32_t mlo, mhi;
                af_pair(smem, L, xs, tab[q], p.D, s, t, mlo, mhi);
                const float mn = fmaxf(m, s);
                const float keep = expf(m - mn), mine = expf(s - mn);      // (m = -inf: keep = 0)
                den = fmaf(den, keep, mine);
                num = fmaf(num, keep, mine * t);
                m = mn;
            }
        }
        const float M = fx_wave_max(m);     // P >= 1: finite
        const float sc = expf(m - M);       // a lane without a pair: exp(-inf) = 0
        den = fx_wave_sum(den * sc);
        num = fx_wave_sum(num * sc);
        if (lane == 0) {
            const float y = num / den;
            p.stats[b * AF_STATS + 0] = M;
            p.stats[b * AF_STATS + 1] = den;
            p.stats[b * AF_STATS + 2] = y;
            p.out[b] = p.addend ? y + p.addend[b] : y;
        }
    }
}

// grid and block as the forward; dynamic LDS af_lds_bytes(.., true, nw); partial: [gridDim.x, n]
template <int VEC>
__global__ __launch_bounds__(64 * AF_WAVES) void k_afm_attn_bwd(AfArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AfLds L = af_lds(p.F, p.D, p.A, p.P, true);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* mine = smem + L.shared + w * L.per_wave;
    float* xs = mine + L.xs;
    float* dsv = mine + L.ds;
    float* dtv = mine + L.dt;
    uint32_t* mlov = reinterpret_cast<uint32_t*>(mine + L.mlo);
    uint32_t* mhiv = reinterpret_cast<uint32_t*>(mine + L.mhi);
    float* wacc = mine + L.wacc;
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(smem + L.tab);
    const float* w2s = smem + L.w2;
    const float* wps = smem + L.wp;
    const int F = p.F, D = p.D, A = p.A, P = p.P, AD = p.A * p.D;
    af_stage_weights(p, L, smem, true);
    for (int e = lane; e < L.n; e += 64) wacc[e] = 0.f;
    const int64_t tiles = (p.B + p.nw - 1) / p.nw;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b = tile * p.nw + w;
        const bool act = b < p.B;
        __syncthreads();
        if (act) af_stage_x<VEC>(p.X + b * p.ldx, xs, F * D, D, L.Dp, lane);
        __syncthreads();
        // (A) lane = pair
        if (act) {
            const float gb = p.g[b];
            const float M = p.stats[b * AF_STATS + 0], den = p.stats[b * AF_STATS + 1], y = p.stats[b * AF_STATS + 2];
            for (int q = lane; q < P; q += 64) {
                float s, t;
                uint32_t mlo, mhi;
                af_pair(smem, L, xs, tab[q], D, s, t, mlo, mhi);
                const float dt = gb * (expf(s - M) / den);
                dtv[q] = dt;
                dsv[q] = dt * (t - y);
                mlov[q] = mlo;
                mhiv[q] = mhi;
            }
        }
        __syncthreads();
        if (!act) continue;                 // (no barrier below this line inside the loop body)
        // (B) dw2[a] += sum_p ds_p h_p[a], db1[a] += w2[a] sum_p [z_p[a] > 0] ds_p: a lane sums its own pairs, the
        // wave sums the lanes, lane k of the chunk adds to the wave's accumulator
        for (int a0 = 0; a0 < L.A8; a0 += AF_CHUNK) {
            float hw[AF_CHUNK], bw[AF_CHUNK];
#pragma unroll
            for (int k = 0; k < AF_CHUNK; ++k) hw[k] = bw[k] = 0.f;
            for (int q = lane; q < P; q += 64) {
                const uint32_t ij = tab[q];
                float z[AF_CHUNK], unused = 0.f;
                af_zchunk<false>(xs + (ij >> 16) * L.Dp, xs + (ij & 0xffffu) * L.Dp, smem + L.wt, L.AS, D,
                                 smem + L.b1, wps, a0, z, unused);
                const float ds = dsv[q];
#pragma unroll
                for (int k = 0; k < AF_CHUNK; ++k) {
                    hw[k] = fmaf(ds, fmaxf(z[k], 0.f), hw[k]);
                    bw[k] += z[k] > 0.f ? ds : 0.f;
                }
            }
            float hsum = 0.f, bsum = 0.f;
#pragma unroll
            for (int k = 0; k < AF_CHUNK; ++k) {
                const float hs = fx_wave_sum(hw[k]), bs = fx_wave_sum(bw[k]);
                if (lane == k) { hsum = hs; bsum = bs; }
            }
            if (lane < AF_CHUNK && a0 + lane < A) {
                wacc[AD + a0 + lane] += w2s[a0 + lane] * bsum;          // db1
                wacc[AD + A + a0 + lane] += hsum;                       // dw2
            }
        }
        // (C) dW1[a, d] += w2[a] sum_p [z_p[a] > 0] ds_p e_p[d] and dwp[d] += sum_p dt_p e_p[d], in tiles of 8 hidden
        // units by 8 dimensions: a lane sums its own pairs into 64 registers, the wave sums the lanes, lane 8 ka + kd
        // adds the tile's element (ka, kd) to the wave's accumulator
        for (int a0 = 0; a0 < L.A8; a0 += AF_CHUNK) {
            for (int d0 = 0; d0 < D; d0 += 8) {
                float acc[AF_CHUNK][8], accp[8];
#pragma unroll
                for (int kd = 0; kd < 8; ++kd) {
                    accp[kd] = 0.f;
#pragma unroll
                    for (int ka = 0; ka < AF_CHUNK; ++ka) acc[ka][kd] = 0.f;
                }
                for (int q = lane; q < P; q += 64) {
                    const uint32_t ij = tab[q];
                    const float* xi = xs + (ij >> 16) * L.Dp;
                    const float* xj = xs + (ij & 0xffffu) * L.Dp;
                    const float ds = dsv[q], dt = dtv[q];
                    const uint32_t bits = a0 < 32 ? mlov[q] >> a0 : mhiv[q] >> (a0 - 32);
                    float dz[AF_CHUNK];
#pragma unroll
                    for (int ka = 0; ka < AF_CHUNK; ++ka) dz[ka] = ((bits >> ka) & 1u) ? ds : 0.f;
#pragma unroll
                    for (int kd = 0; kd < 8; ++kd) {
                        const int d = d0 + kd < D ? d0 + kd : D - 1;        // (beyond D: a valid address, no use)
                        const float e = d0 + kd < D ? xi[d] * xj[d] : 0.f;
#pragma unroll
                        for (int ka = 0; ka < AF_CHUNK; ++ka) acc[ka][kd] = fmaf(dz[ka], e, acc[ka][kd]);
                        if (a0 == 0) accp[kd] = fmaf(dt, e, accp[kd]);
                    }
                }
                float mine = 0.f, minep = 0.f;
#pragma unroll
                for (int ka = 0; ka < AF_CHUNK; ++ka) {
#pragma unroll
                    for (int kd = 0; kd < 8; ++kd) {
                        const float t = fx_wave_sum(acc[ka][kd]);
                        if (lane == ka * 8 + kd) mine = t;
                    }
                }
                const int ka = lane >> 3, kd = lane & 7;
                if (a0 + ka < A && d0 + kd < D) wacc[(a0 + ka) * D + d0 + kd] += w2s[a0 + ka] * mine;
                if (a0 == 0) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float t = fx_wave_sum(accp[k]);
                        if (lane == k) minep = t;
                    }
                    if (lane < 8 && d0 + lane < D) wacc[AD + 2 * A + d0 + lane] += minep;
                }
            }
        }
        // (D) lane = VEC elements (i, d..) of the record: dx_i[d] = sum_{j != i} (dt_p wp[d] + ds_p sum_a
        // [z_p[a] > 0] w2[a] W1[a, d]) x_j[d], p the pair of i and j
        const float* wwt = smem + L.wwt;
        float* dxb = p.dX + b * p.lddx;
        for (int c = lane * VEC; c < F * D; c += 64 * VEC) {
            const int i = c / D, d = c - i * D;
            float acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
            for (int j = 0; j < F; ++j) {
                if (j == i) continue;
                const int lo = j < i ? j : i, hi = j < i ? i : j;
                const int q = fx_pair_off(lo, F) + hi - lo - 1;
                const float ds = dsv[q], dt = dtv[q];
                const uint32_t mlo = mlov[q], mhi = mhiv[q];
                float v[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[k] = 0.f;
                for (int a0 = 0; a0 < L.A8; a0 += 4) {
                    const uint32_t bits = a0 < 32 ? mlo >> a0 : mhi >> (a0 - 32);
                    // the mask as 1.0 / 0.0: fmaf(1, w, v) is v + w and fmaf(0, w, v) is v, exactly
                    const float m0 = (bits & 1u) ? 1.f : 0.f, m1 = (bits & 2u) ? 1.f : 0.f;
                    const float m2 = (bits & 4u) ? 1.f : 0.f, m3 = (bits & 8u) ? 1.f : 0.f;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float4 w4 = *reinterpret_cast<const float4*>(wwt + (d + k) * L.AS + a0);
                        v[k] = fmaf(m3, w4.w, fmaf(m2, w4.z, fmaf(m1, w4.y, fmaf(m0, w4.x, v[k]))));
                    }
                }
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float de = fmaf(ds, v[k], dt * wps[d + k]);
                    acc[k] = fmaf(de, xs[j * L.Dp + d + k], acc[k]);
                }
            }
            fx_store<VEC>(dxb + c, acc);
        }
    }
    // the workgroup's row of partial: its waves in wave order
    __syncthreads();
    float* row = p.partial + (int64_t)blockIdx.x * L.n;
    for (int e = threadIdx.x; e < L.n; e += blockDim.x) {
        float sum = 0.f;
        for (int k = 0; k < p.nw; ++k) sum += smem[L.shared + k * L.per_wave + L.wacc + e];
        row[e] = sum;
    }
}

static int af_check(const char* who, int64_t B, int32_t F, int32_t D, int32_t A) {
    FX_CHECK_ARG(F >= 2, "%s: F=%d, limit F >= 2", who, F);
    FX_CHECK_ARG(D >= 1 && D <= AF_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, AF_MAX_D);
    FX_CHECK_ARG(A >= 1 && A <= AF_MAX_A, "%s: A=%d, limit 1 <= A <= %d", who, A, AF_MAX_A);
    FX_CHECK_ARG((int64_t)F * D <= AF_MAX_FD, "%s: F*D=%lld, limit %d", who, (long long)F * D, AF_MAX_FD);
    FX_CHECK_ARG((int64_t)F * (F - 1) / 2 <= AF_MAX_P, "%s: %lld pairs, limit %d", who,
                 (long long)F * (F - 1) / 2, AF_MAX_P);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    return FX_OK;
}

static unsigned af_grid(int64_t B, int nw) {
    const int64_t tiles = fx_ceil_div(B, nw);
    return (unsigned)(tiles < AF_MAX_WG ? tiles : AF_MAX_WG);
}

extern "C" void fx_afm_attn_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = 2;                  // F at least
    limits[1] = AF_MAX_FD;          // F * D at most
    limits[2] = AF_MAX_P;           // pairs at most
    limits[3] = AF_MAX_D;
    limits[4] = AF_MAX_A;
}

extern "C" int32_t fx_afm_attn_tile_rows(int32_t F, int32_t D, int32_t A) {
    if (F < 2 || D < 1 || A < 1) return AF_WAVES;
    return af_waves(F, D, A, F * (F - 1) / 2);
}

extern "C" int64_t fx_afm_attn_workspace_floats(int64_t B, int32_t F, int32_t D, int32_t A) {
    if (F < 2 || D < 1 || A < 1) return 0;
    const int64_t n = (int64_t)A * D + 2 * A + D;
    const int64_t n4 = (n + 3) / 4 * 4;
    return (int64_t)af_grid(B > 0 ? B : 1, af_waves(F, D, A, F * (F - 1) / 2)) * n + 4 + FX_COLSUM_CHUNKS * n4;
}

extern "C" int fx_afm_attn_fwd(const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D, const float* W1,
                               const float* b1, const float* w2, const float* wp, int32_t A, const float* addend,
                               float* out, float* stats, fx_stream_t stream) {
    const char* who = "fx_afm_attn_fwd";
    if (int st = af_check(who, B, F, D, A)) return st;
    FX_CHECK_ARG(ldx >= (int64_t)F * D, "%s: X row stride %lld < F*D", who, (long long)ldx);
    FX_CHECK_ARG(W1 && b1 && w2 && wp, "%s: null W1 / b1 / w2 / wp", who);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(X && out && stats, "%s: null X / out / stats", who);
    AfArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.ldx = ldx; p.W1 = W1; p.b1 = b1; p.w2 = w2; p.wp = wp; p.addend = addend; p.out = out;
    p.stats = stats; p.B = B; p.F = F; p.D = D; p.A = A; p.P = F * (F - 1) / 2;
    p.nw = af_waves(F, D, A, p.P);
    const bool vec4 = D % 4 == 0 && fx_vec_ok(X, ldx);
    static const hipError_t lds_ok[2] = {fx_allow_lds(k_afm_attn_fwd<1>, AF_LDS_MAX),
                                         fx_allow_lds(k_afm_attn_fwd<4>, AF_LDS_MAX)};
    FX_CHECK_HIP(lds_ok[vec4 ? 1 : 0]);
    const size_t lds = af_lds_bytes(F, D, A, p.P, false, p.nw);
    const dim3 grid(af_grid(B, p.nw)), block(64 * p.nw);
    if (vec4) hipLaunchKernelGGL(k_afm_attn_fwd<4>, grid, block, lds, fx_hip_stream(stream), p);
    else hipLaunchKernelGGL(k_afm_attn_fwd<1>, grid, block, lds, fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_afm_attn_bwd(const float* g, const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D,
                               const float* W1, const float* b1, const float* w2, const float* wp, int32_t A,
                               const float* stats, float* dX, int64_t lddx, float* grads, float* workspace,
                               fx_stream_t stream) {
    const char* who = "fx_afm_attn_bwd";
    if (int st = af_check(who, B, F, D, A)) return st;
    FX_CHECK_ARG(ldx >= (int64_t)F * D, "%s: X row stride %lld < F*D", who, (long long)ldx);
    FX_CHECK_ARG(lddx >= (int64_t)F * D, "%s: dX row stride %lld < F*D", who, (long long)lddx);
    FX_CHECK_ARG(W1 && b1 && w2 && wp, "%s: null W1 / b1 / w2 / wp", who);
    FX_CHECK_ARG(grads && workspace, "%s: null grads / workspace", who);
    const int64_t n = (int64_t)A * D + 2 * A + D;
    if (B == 0) {
        FX_CHECK_HIP(hipMemsetAsync(grads, 0, sizeof(float) * n, fx_hip_stream(stream)));
        return FX_OK;
    }
    FX_CHECK_ARG(g && X && stats && dX, "%s: null g / X / stats / dX", who);
    AfArgs p;
    memset(&p, 0, sizeof(p));
    p.g = g; p.X = X; p.ldx = ldx; p.W1 = W1; p.b1 = b1; p.w2 = w2; p.wp = wp; p.stats = const_cast<float*>(stats);
    p.dX = dX; p.lddx = lddx; p.B = B; p.F = F; p.D = D; p.A = A; p.P = F * (F - 1) / 2;
    p.nw = af_waves(F, D, A, p.P);
    p.partial = workspace;
    const bool vec4 = D % 4 == 0 && fx_vec_ok(X, ldx) && fx_vec_ok(dX, lddx);
    static const hipError_t lds_ok[2] = {fx_allow_lds(k_afm_attn_bwd<1>, AF_LDS_MAX),
                                         fx_allow_lds(k_afm_attn_bwd<4>, AF_LDS_MAX)};
    FX_CHECK_HIP(lds_ok[vec4 ? 1 : 0]);
    const size_t lds = af_lds_bytes(F, D, A, p.P, true, p.nw);
    const unsigned G = af_grid(B, p.nw);
    const dim3 grid(G), block(64 * p.nw);
    if (vec4) hipLaunchKernelGGL(k_afm_attn_bwd<4>, grid, block, lds, fx_hip_stream(stream), p);
    else hipLaunchKernelGGL(k_afm_attn_bwd<1>, grid, block, lds, fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    // the rows of partial -> grads, two fixed-order stages; its own workspace starts 16-byte aligned behind them
    float* cws = workspace + ((int64_t)G * n + 3) / 4 * 4;
    return fx_colsum(workspace, n, G, n, grads, cws, stream);
}
