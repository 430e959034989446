// fx_finalmlp.hip — the two stages of FinalMLP that are not towers (model_zoo/FinalMLP/src/FinalMLP.py):
//   * the feature gates of FeatureSelection.forward (FinalMLP.py:179-192)
//         F1 = E * 2 sigmoid(Z1),  F2 = E * 2 sigmoid(Z2)
//     both in one launch.  Z is the gate tower's pre-sigmoid output: [B, W], or ONE row for all samples when the
//     gate has no context features (the reference repeats the [1, D] bias B times, FinalMLP.py:180; here the tower
//     ran on that one row and z_ld == 0 says so).  The two gates choose independently; Z2 == NULL is one gate.
//   * the head InteractionAggregation.forward with output_dim 1 (FinalMLP.py:227-235)
//         out[b] = b_x + b_y + sum_j X[b, j] w_x[j] + sum_k Y[b, k] (w_y[k] + T[b, k])     (+ out_add[b])
//     where T[:, h dyh : (h + 1) dyh] = X[:, h dxh : (h + 1) dxh] W_h is the caller's per-head GEMM.
// fp32 throughout.  Every matrix has its own row stride (floats): column slices and the gather record are read in
// place.  16-byte accesses (VEC = 4) when the widths are multiples of 4 and every base pointer and row stride is
// 16-byte aligned, a scalar arm (VEC = 1) otherwise.
//
// Forward gate: an element-wise grid-stride pass.  Forward head: L = 4, 16 or 64 lanes per row (ag_lanes: the
// smallest that covers the wider of X and Y in one round, a wave looping over the chunks beyond 64), a wave handles
// 64 / L rows, sums by xor shuffles inside the group: no width limit.
// Backward of both: a thread per column chunk and a slab of rows per workgroup row (fm_slabs).  The thread walks the
// rows of its slab, writes the per-sample gradients (dE, per-sample dZ; dT, dY, g w_x^T) and keeps the sums over
// the batch (broadcast dZ; dw_x, dw_y, db) in registers: one partial per slab into caller workspace, then
// fx_rowsum.h's shared row sum adds the slabs in a fixed order (four runs of consecutive slabs, fp32).  No atomics
// anywhere: two launches on the same inputs give the same bits.  The sigmoid is recomputed from Z in the backward;
// nothing is stashed by the forward.
#include "fx_common.h"
#include "fx_rowsum.h"

#define FM_T 256
#define FM_MAX_WG 2048            // 8 workgroups per CU
#define FM_SLAB_ROWS 16           // rows of a slab, as long as that gives at most FM_MAX_SLABS of them
#define FM_MAX_SLABS 256

struct FmSlabs {
    int nslab;
    int64_t rows_per_slab;
};

static FmSlabs fm_slabs(int64_t rows) {
    FmSlabs s;
    if (rows < 1) rows = 1;
    s.rows_per_slab = fx_ceil_div(rows, FM_MAX_SLABS);
    if (s.rows_per_slab < FM_SLAB_ROWS) s.rows_per_slab = FM_SLAB_ROWS;
    s.nslab = (int)fx_ceil_div(rows, s.rows_per_slab);
    return s;
}

// s2 = 2 sigmoid(z) and d2 = 2 sigmoid(z) (1 - sigmoid(z)) from t = exp(-|z|) in (0, 1]: sigmoid(|z|) = 1 / (1 + t)
// and sigmoid(-|z|) = t / (1 + t), neither of them a difference of nearly equal numbers: finite and accurate in
// both saturated tails
__device__ __forceinline__ void fm_gate(float z, float& s2, float& d2) {
    const float t = expf(-fabsf(z));
    const float hi = 1.f / (1.f + t);
    const float lo = t * hi;
    s2 = 2.f * (z >= 0.f ? hi : lo);
    d2 = 2.f * hi * lo;
}

struct GateArgs {
    const float* E; int64_t e_ld;
    int64_t B;
    int W;
    const float* Z1; int64_t z1_ld;     // (a row stride of 0: one row for every sample)
    const float* Z2; int64_t z2_ld;     // Z2 == nullptr: one gate
    float* F1; int64_t f1_ld;
    float* F2; int64_t f2_ld;
    const float* dF1; int64_t df1_ld;
    const float* dF2; int64_t df2_ld;
    float* dE; int64_t de_ld; int de_acc;
    float* dZ1; int64_t dz1_ld;         // per-sample gates only; a broadcast gate's dZ leaves through `partial`
    float* dZ2; int64_t dz2_ld;
    float* partial;                     // [nslab, 2, W]
    int64_t rows_per_slab;
};

template <int VEC>
__global__ __launch_bounds__(FM_T) void k_gate2_fwd(GateArgs p) {
    const int64_t chunks = p.W / VEC;
    const int64_t total = p.B * chunks;
    for (int64_t i = (int64_t)blockIdx.x * FM_T + threadIdx.x; i < total; i += (int64_t)gridDim.x * FM_T) {
        const int64_t r = i / chunks;
        const int64_t c = (i - r * chunks) * VEC;
        float e[VEC], z[VEC], f[VEC];
        fx_load<VEC>(p.E + r * p.e_ld + c, e);
        fx_load<VEC>(p.Z1 + r * p.z1_ld + c, z);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float s2, d2;
            fm_gate(z[k], s2, d2);
            f[k] = e[k] * s2;
        }
        fx_store<VEC>(p.F1 + r * p.f1_ld + c, f);
        if (p.Z2) {
            fx_load<VEC>(p.Z2 + r * p.z2_ld + c, z);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float s2, d2;
                fm_gate(z[k], s2, d2);
                f[k] = e[k] * s2;
            }
            fx_store<VEC>(p.F2 + r * p.f2_ld + c, f);
        }
    }
}

// one gate's share of a row: de += dF * 2 sigma, dz = dF * e * 2 sigma (1 - sigma)
template <int VEC>
__device__ __forceinline__ void gate_bwd_row(const float* dF, const float (&e)[VEC], const float (&s2)[VEC],
                                             const float (&d2)[VEC], float (&de)[VEC], float (&dz)[VEC]) {
    float g[VEC];
    fx_load<VEC>(dF, g);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        de[k] = fmaf(g[k], s2[k], de[k]);
        dz[k] = g[k] * e[k] * d2[k];
    }
}

// grid (ceil(W / VEC / 256), nslab)
template <int VEC>
__global__ __launch_bounds__(FM_T) void k_gate2_bwd(GateArgs p) {
    const int64_t chunk = (int64_t)blockIdx.x * FM_T + threadIdx.x;
    if (chunk >= p.W / VEC) return;
    const int64_t c = chunk * VEC;
    const int64_t r0 = (int64_t)blockIdx.y * p.rows_per_slab;
    const int64_t r1 = r0 + p.rows_per_slab < p.B ? r0 + p.rows_per_slab : p.B;
    const bool two = p.Z2 != nullptr;
    const bool bc1 = p.z1_ld == 0, bc2 = two && p.z2_ld == 0;
    float s1[VEC], d1[VEC], s2[VEC], d2[VEC], a1[VEC], a2[VEC], z[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s1[k] = d1[k] = s2[k] = d2[k] = a1[k] = a2[k] = 0.f;
    if (bc1) {                              // the gate of a broadcast row is the same for every sample
        fx_load<VEC>(p.Z1 + c, z);
#pragma unroll
        for (int k = 0; k < VEC; ++k) fm_gate(z[k], s1[k], d1[k]);
    }
    if (bc2) {
        fx_load<VEC>(p.Z2 + c, z);
#pragma unroll
        for (int k = 0; k < VEC; ++k) fm_gate(z[k], s2[k], d2[k]);
    }
    for (int64_t r = r0; r < r1; ++r) {
        float e[VEC], de[VEC], dz[VEC];
        fx_load<VEC>(p.E + r * p.e_ld + c, e);
#pragma unroll
        for (int k = 0; k < VEC; ++k) de[k] = 0.f;
        if (!bc1) {
            fx_load<VEC>(p.Z1 + r * p.z1_ld + c, z);
#pragma unroll
            for (int k = 0; k < VEC; ++k) fm_gate(z[k], s1[k], d1[k]);
        }
        gate_bwd_row<VEC>(p.dF1 + r * p.df1_ld + c, e, s1, d1, de, dz);
        if (bc1) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) a1[k] += dz[k];
        } else {
            fx_store<VEC>(p.dZ1 + r * p.dz1_ld + c, dz);
        }
        if (two) {
            if (!bc2) {
                fx_load<VEC>(p.Z2 + r * p.z2_ld + c, z);
#pragma unroll
                for (int k = 0; k < VEC; ++k) fm_gate(z[k], s2[k], d2[k]);
            }
            gate_bwd_row<VEC>(p.dF2 + r * p.df2_ld + c, e, s2, d2, de, dz);
            if (bc2) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) a2[k] += dz[k];
            } else {
                fx_store<VEC>(p.dZ2 + r * p.dz2_ld + c, dz);
            }
        }
        float* out = p.dE + r * p.de_ld + c;
        if (p.de_acc) {
            float old[VEC];
            fx_load<VEC>(out, old);
#pragma unroll
            for (int k = 0; k < VEC; ++k) de[k] += old[k];
        }
        fx_store<VEC>(out, de);
    }
    float* part = p.partial + (int64_t)blockIdx.y * 2 * p.W;
    if (bc1) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) part[c + k] = a1[k];
    }
    if (bc2) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) part[p.W + c + k] = a2[k];
    }
}

// The head's k_fx_rowsum: [dw_x | dw_y | db] over the slabs, with db, the last column, written twice
// (db[0] = db[1] = sum g: one for b_x, one for b_y)
__global__ __launch_bounds__(FM_T) void k_biagg_reduce(const float* partial, int nslab, int64_t C, FxRowsumOut o) {
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    float* dst = fx_rowsum_dst(o, i);
    const float t = fx_rowsum_col<float, FX_ROWS_RUNS>(partial, nslab, C, i, dst != nullptr);
    if (threadIdx.x < 64 && dst) {
        dst[0] = t;
        if (i == C - 1) dst[1] = t;
    }
}

// ---- the aggregation head ---------------------------------------------------------------------------------
struct AggArgs {
    const float* X; int64_t x_ld;
    const float* Y; int64_t y_ld;
    const float* T; int64_t t_ld;
    int64_t B;
    int dx, dy, L;
    const float* wx; const float* wy; const float* bx; const float* by;
    const float* out_add;
    float* out;
    const float* g;
    float* dT; int64_t dt_ld;
    float* dY; int64_t dy_ld;
    float* dXr; int64_t dxr_ld;         // g w_x^T (nullptr: not wanted)
    float* partial;                     // [nslab, dx + dy + 1]
    int64_t rows_per_slab;
};

// lanes per row: the smallest of 4, 16, 64 that covers the wider operand in one round of VEC floats per lane
static int ag_lanes(int dx, int dy, int vec) {
    const int wide = dx > dy ? dx : dy;
    const int chunks = (wide + vec - 1) / vec;
    return chunks <= 4 ? 4 : (chunks <= 16 ? 16 : 64);
}

template <int VEC>
__global__ __launch_bounds__(FM_T) void k_biagg_fwd(AggArgs p) {
    const int L = p.L, per_wave = 64 / L, per_wg = (FM_T / 64) * per_wave;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (L - 1);
    const float b = (p.bx ? p.bx[0] : 0.f) + (p.by ? p.by[0] : 0.f);
    for (int64_t row0 = (int64_t)blockIdx.x * per_wg; row0 < p.B; row0 += (int64_t)gridDim.x * per_wg) {
        const int64_t r = row0 + wave * per_wave + lane / L;
        const bool active = r < p.B;
        float acc = 0.f;
        if (active) {
            const float* x = p.X + r * p.x_ld;
            for (int e = sub * VEC; e < p.dx; e += L * VEC) {
                float xv[VEC], wv[VEC];
                fx_load<VEC>(x + e, xv);
                fx_load<VEC>(p.wx + e, wv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc = fmaf(xv[k], wv[k], acc);
            }
            const float* y = p.Y + r * p.y_ld;
            const float* t = p.T + r * p.t_ld;
            for (int e = sub * VEC; e < p.dy; e += L * VEC) {
                float yv[VEC], wv[VEC], tv[VEC];
                fx_load<VEC>(y + e, yv);
                fx_load<VEC>(p.wy + e, wv);
                fx_load<VEC>(t + e, tv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc = fmaf(yv[k], wv[k] + tv[k], acc);
            }
        }
        for (int off = L >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (active && sub == 0) p.out[r] = acc + b + (p.out_add ? p.out_add[r] : 0.f);
    }
}

// grid (ceil((dx + dy) / VEC / 256), nslab): the chunks of X's columns, then those of Y's
template <int VEC>
__global__ __launch_bounds__(FM_T) void k_biagg_bwd(AggArgs p) {
    const int64_t chunk = (int64_t)blockIdx.x * FM_T + threadIdx.x;
    const int64_t nx = p.dx / VEC, ny = p.dy / VEC;
    if (chunk >= nx + ny) return;
    const int64_t r0 = (int64_t)blockIdx.y * p.rows_per_slab;
    const int64_t r1 = r0 + p.rows_per_slab < p.B ? r0 + p.rows_per_slab : p.B;
    float* part = p.partial + (int64_t)blockIdx.y * ((int64_t)p.dx + p.dy + 1);
    float acc[VEC], w[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if (chunk < nx) {
        const int64_t c = chunk * VEC;
        fx_load<VEC>(p.wx + c, w);
        float gs = 0.f;
        for (int64_t r = r0; r < r1; ++r) {
            const float g = p.g[r];
            float xv[VEC];
            fx_load<VEC>(p.X + r * p.x_ld + c, xv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = fmaf(xv[k], g, acc[k]);
            if (p.dXr) {
                float o[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) o[k] = g * w[k];
                fx_store<VEC>(p.dXr + r * p.dxr_ld + c, o);
            }
            gs += g;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) part[c + k] = acc[k];
        if (chunk == 0) part[(int64_t)p.dx + p.dy] = gs;
    } else {
        const int64_t c = (chunk - nx) * VEC;
        fx_load<VEC>(p.wy + c, w);
        for (int64_t r = r0; r < r1; ++r) {
            const float g = p.g[r];
            float yv[VEC], tv[VEC], a[VEC], b[VEC];
            fx_load<VEC>(p.Y + r * p.y_ld + c, yv);
            fx_load<VEC>(p.T + r * p.t_ld + c, tv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                acc[k] = fmaf(yv[k], g, acc[k]);
                a[k] = g * yv[k];
                b[k] = g * (w[k] + tv[k]);
            }
            fx_store<VEC>(p.dT + r * p.dt_ld + c, a);
            fx_store<VEC>(p.dY + r * p.dy_ld + c, b);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) part[p.dx + c + k] = acc[k];
    }
}

// ---------------------------------------------------------------------------------------------------------
extern "C" int64_t fx_finalmlp_slab_rows(int64_t B) { return fm_slabs(B).rows_per_slab; }

extern "C" int64_t fx_gate2_workspace_floats(int64_t B, int32_t W) {
    if (B < 1 || W < 1) return 0;
    return (int64_t)fm_slabs(B).nslab * 2 * W;
}

extern "C" int64_t fx_biagg_workspace_floats(int64_t B, int32_t dx, int32_t dy) {
    if (B < 1 || dx < 1 || dy < 1) return 0;
    return (int64_t)fm_slabs(B).nslab * ((int64_t)dx + dy + 1);
}

// a [B, W] matrix, or with ld == 0 (where `bcast` allows it) one row
static int gate_check_mat(const char* who, const char* name, const void* ptr, int64_t ld, int32_t W, bool bcast) {
    FX_CHECK_ARG(ptr, "%s: null %s", who, name);
    FX_CHECK_ARG(ld >= W || (bcast && ld == 0), "%s: %s row stride %lld < W=%d%s", who, name, (long long)ld, W,
                 bcast ? " (0: one broadcast row)" : "");
    return FX_OK;
}

extern "C" int fx_gate2_fwd(const float* E, int64_t e_ld, int64_t B, int32_t W, const float* Z1, int64_t z1_ld,
                            const float* Z2, int64_t z2_ld, float* F1, int64_t f1_ld, float* F2, int64_t f2_ld,
                            fx_stream_t stream) {
    const char* who = "fx_gate2_fwd";
    FX_CHECK_ARG(W >= 1, "%s: W=%d", who, W);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    if (int st = gate_check_mat(who, "E", E, e_ld, W, false)) return st;
    if (int st = gate_check_mat(who, "Z1", Z1, z1_ld, W, true)) return st;
    if (int st = gate_check_mat(who, "F1", F1, f1_ld, W, false)) return st;
    if (Z2) {
        if (int st = gate_check_mat(who, "Z2", Z2, z2_ld, W, true)) return st;
        if (int st = gate_check_mat(who, "F2", F2, f2_ld, W, false)) return st;
    }
    if (B == 0) return FX_OK;
    GateArgs p;
    memset(&p, 0, sizeof(p));
    p.E = E; p.e_ld = e_ld; p.B = B; p.W = W;
    p.Z1 = Z1; p.z1_ld = z1_ld; p.Z2 = Z2; p.z2_ld = z2_ld;
    p.F1 = F1; p.f1_ld = f1_ld; p.F2 = F2; p.f2_ld = f2_ld;
    const bool vec4 = W % 4 == 0 && fx_vec_ok(E, e_ld) && fx_vec_ok(Z1, z1_ld) && fx_vec_ok(F1, f1_ld) &&
                      (!Z2 || (fx_vec_ok(Z2, z2_ld) && fx_vec_ok(F2, f2_ld)));
    const int64_t total = B * (vec4 ? W / 4 : W);
    int64_t grid = fx_ceil_div(total, FM_T);
    if (grid > FM_MAX_WG) grid = FM_MAX_WG;
    hipStream_t s = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL(k_gate2_fwd<4>, dim3((unsigned)grid), dim3(FM_T), 0, s, p);
    else hipLaunchKernelGGL(k_gate2_fwd<1>, dim3((unsigned)grid), dim3(FM_T), 0, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_gate2_bwd(const float* dF1, int64_t df1_ld, const float* dF2, int64_t df2_ld, const float* E,
                            int64_t e_ld, int64_t B, int32_t W, const float* Z1, int64_t z1_ld, const float* Z2,
                            int64_t z2_ld, float* dE, int64_t de_ld, int32_t de_accumulate, float* dZ1,
                            int64_t dz1_ld, float* dZ2, int64_t dz2_ld, float* workspace, fx_stream_t stream) {
    const char* who = "fx_gate2_bwd";
    FX_CHECK_ARG(W >= 1, "%s: W=%d", who, W);
    FX_CHECK_ARG(B >= 1, "%s: B=%lld", who, (long long)B);
    if (int st = gate_check_mat(who, "E", E, e_ld, W, false)) return st;
    if (int st = gate_check_mat(who, "dE", dE, de_ld, W, false)) return st;
    if (int st = gate_check_mat(who, "Z1", Z1, z1_ld, W, true)) return st;
    if (int st = gate_check_mat(who, "dF1", dF1, df1_ld, W, false)) return st;
    // dZ has the shape of its Z: [B, W] with a row stride, or the one row that the slabs are summed into
    if (int st = gate_check_mat(who, "dZ1", dZ1, z1_ld == 0 ? 0 : dz1_ld, W, z1_ld == 0)) return st;
    if (Z2) {
        if (int st = gate_check_mat(who, "Z2", Z2, z2_ld, W, true)) return st;
        if (int st = gate_check_mat(who, "dF2", dF2, df2_ld, W, false)) return st;
        if (int st = gate_check_mat(who, "dZ2", dZ2, z2_ld == 0 ? 0 : dz2_ld, W, z2_ld == 0)) return st;
    }
    const bool bc1 = z1_ld == 0, bc2 = Z2 && z2_ld == 0;
    FX_CHECK_ARG(!(bc1 || bc2) || workspace, "%s: a broadcast gate's dZ is summed through workspace: null", who);
    GateArgs p;
    memset(&p, 0, sizeof(p));
    p.E = E; p.e_ld = e_ld; p.B = B; p.W = W;
    p.Z1 = Z1; p.z1_ld = z1_ld; p.Z2 = Z2; p.z2_ld = z2_ld;
    p.dF1 = dF1; p.df1_ld = df1_ld; p.dF2 = dF2; p.df2_ld = df2_ld;
    p.dE = dE; p.de_ld = de_ld; p.de_acc = de_accumulate ? 1 : 0;
    p.dZ1 = dZ1; p.dz1_ld = dz1_ld; p.dZ2 = dZ2; p.dz2_ld = dz2_ld;
    const FmSlabs sl = fm_slabs(B);
    p.partial = workspace; p.rows_per_slab = sl.rows_per_slab;
    const bool vec4 = W % 4 == 0 && fx_vec_ok(E, e_ld) && fx_vec_ok(dE, de_ld) && fx_vec_ok(Z1, z1_ld) &&
                      fx_vec_ok(dF1, df1_ld) && (bc1 || fx_vec_ok(dZ1, dz1_ld)) &&
                      (!Z2 || (fx_vec_ok(Z2, z2_ld) && fx_vec_ok(dF2, df2_ld) && (bc2 || fx_vec_ok(dZ2, dz2_ld))));
    const dim3 grid((unsigned)fx_ceil_div(vec4 ? W / 4 : W, FM_T), (unsigned)sl.nslab);
    hipStream_t s = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL(k_gate2_bwd<4>, grid, dim3(FM_T), 0, s, p);
    else hipLaunchKernelGGL(k_gate2_bwd<1>, grid, dim3(FM_T), 0, s, p);
    FX_CHECK_LAUNCH();
    if (bc1 || bc2)     // (a per-sample gate's half of the partials was never written: a null segment)
        return fx_rowsum<float, FX_ROWS_RUNS>(s, workspace, sl.nslab, 2 * (int64_t)W,
                                              fx_rowsum_out(bc1 ? dZ1 : nullptr, W, bc2 ? dZ2 : nullptr, W));
    return FX_OK;
}

static int agg_check(const char* who, const float* X, int64_t x_ld, const float* Y, int64_t y_ld, const float* T,
                     int64_t t_ld, int64_t B, int32_t dx, int32_t dy, const float* w_x, const float* w_y) {
    FX_CHECK_ARG(dx >= 1 && dy >= 1, "%s: dx=%d dy=%d", who, dx, dy);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(X && Y && T && w_x && w_y, "%s: null X / Y / T / w_x / w_y", who);
    FX_CHECK_ARG(x_ld >= dx && y_ld >= dy && t_ld >= dy,
                 "%s: a row stride is smaller than its row (X %lld < %d, Y %lld or T %lld < %d)", who,
                 (long long)x_ld, dx, (long long)y_ld, (long long)t_ld, dy);
    return FX_OK;
}

extern "C" int fx_biagg_fwd(const float* X, int64_t x_ld, const float* Y, int64_t y_ld, const float* T,
                            int64_t t_ld, int64_t B, int32_t dx, int32_t dy, const float* w_x, const float* w_y,
                            const float* b_x, const float* b_y, const float* out_add, float* out,
                            fx_stream_t stream) {
    if (int st = agg_check("fx_biagg_fwd", X, x_ld, Y, y_ld, T, t_ld, B, dx, dy, w_x, w_y)) return st;
    FX_CHECK_ARG(out, "fx_biagg_fwd: null out");
    if (B == 0) return FX_OK;
    AggArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.Y = Y; p.y_ld = y_ld; p.T = T; p.t_ld = t_ld;
    p.B = B; p.dx = dx; p.dy = dy;
    p.wx = w_x; p.wy = w_y; p.bx = b_x; p.by = b_y; p.out_add = out_add; p.out = out;
    const bool vec4 = dx % 4 == 0 && dy % 4 == 0 && fx_vec_ok(X, x_ld) && fx_vec_ok(Y, y_ld) && fx_vec_ok(T, t_ld) &&
                      fx_al16(w_x) && fx_al16(w_y);
    p.L = ag_lanes(dx, dy, vec4 ? 4 : 1);
    const int64_t per_wg = (FM_T / 64) * (64 / p.L);
    int64_t grid = fx_ceil_div(B, per_wg);
    if (grid > FM_MAX_WG) grid = FM_MAX_WG;
    hipStream_t s = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL(k_biagg_fwd<4>, dim3((unsigned)grid), dim3(FM_T), 0, s, p);
    else hipLaunchKernelGGL(k_biagg_fwd<1>, dim3((unsigned)grid), dim3(FM_T), 0, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_biagg_bwd(const float* g, const float* X, int64_t x_ld, const float* Y, int64_t y_ld,
                            const float* T, int64_t t_ld, int64_t B, int32_t dx, int32_t dy, const float* w_x,
                            const float* w_y, float* dT, int64_t dt_ld, float* dY, int64_t dy_ld, float* dXr,
                            int64_t dxr_ld, float* dw_x, float* dw_y, float* db, float* workspace,
                            fx_stream_t stream) {
    const char* who = "fx_biagg_bwd";
    if (int st = agg_check(who, X, x_ld, Y, y_ld, T, t_ld, B, dx, dy, w_x, w_y)) return st;
    FX_CHECK_ARG(B >= 1, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(g && dT && dY && dw_x && dw_y && db && workspace,
                 "%s: null g / dT / dY / dw_x / dw_y / db / workspace", who);
    FX_CHECK_ARG(dt_ld >= dy && dy_ld >= dy && (!dXr || dxr_ld >= dx),
                 "%s: a row stride is smaller than its row (dT %lld or dY %lld < %d, dXr %lld < %d)", who,
                 (long long)dt_ld, (long long)dy_ld, dy, (long long)dxr_ld, dx);
    AggArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.Y = Y; p.y_ld = y_ld; p.T = T; p.t_ld = t_ld;
    p.B = B; p.dx = dx; p.dy = dy;
    p.wx = w_x; p.wy = w_y; p.g = g;
    p.dT = dT; p.dt_ld = dt_ld; p.dY = dY; p.dy_ld = dy_ld; p.dXr = dXr; p.dxr_ld = dxr_ld;
    const FmSlabs sl = fm_slabs(B);
    p.partial = workspace; p.rows_per_slab = sl.rows_per_slab;
    const bool vec4 = dx % 4 == 0 && dy % 4 == 0 && fx_vec_ok(X, x_ld) && fx_vec_ok(Y, y_ld) && fx_vec_ok(T, t_ld) &&
                      fx_al16(w_x) && fx_al16(w_y) && fx_vec_ok(dT, dt_ld) && fx_vec_ok(dY, dy_ld) &&
                      (!dXr || fx_vec_ok(dXr, dxr_ld));
    const int64_t chunks = vec4 ? (int64_t)dx / 4 + dy / 4 : (int64_t)dx + dy;
    const dim3 grid((unsigned)fx_ceil_div(chunks, FM_T), (unsigned)sl.nslab);
    hipStream_t s = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL(k_biagg_bwd<4>, grid, dim3(FM_T), 0, s, p);
    else hipLaunchKernelGGL(k_biagg_bwd<1>, grid, dim3(FM_T), 0, s, p);
    FX_CHECK_LAUNCH();
    const int64_t C = (int64_t)dx + dy + 1;
    hipLaunchKernelGGL(k_biagg_reduce, dim3((unsigned)fx_ceil_div(C, 64)), dim3(FM_T), 0, s, workspace, sl.nslab, C,
                       fx_rowsum_out(dw_x, dx, dw_y, dy, db, 1));
    FX_CHECK_LAUNCH();
    return FX_OK;
}
