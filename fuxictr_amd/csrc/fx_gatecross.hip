// fx_gatecross.hip — the element-wise half of GDCN's gated cross layer (model_zoo/GDCN/src/GDCN.py:197-211)
//         x_{i+1} = x_0 * (W_i x_i + b_i) * sigmoid(Wg_i x_i) + x_i
// The two products are the caller's ONE GEMM of x_i against the packed [2 cols, cols] weight: h[:, :cols] = u0 =
// W x_i and h[:, cols:] = v = Wg x_i.  With u = u0 + b and g = sigmoid(v):
//   fx_gate_cross_fwd : xn = x0 * u * g + xi
//   fx_gate_cross_bwd : dh[:, :cols] = dxn * x0 * g,  dh[:, cols:] = dxn * x0 * u * g * (1 - g),
//                       dx0 (= | +=) dxn * u * g (+ dxn)
// u and g are recomputed from h in the backward; the forward stashes nothing.  fp32 throughout.  Every matrix has
// its own row stride (floats): xn may be a column range of a wider buffer, dxn a column slice of a wider gradient.
// 16-byte accesses (VEC = 4) when cols is a multiple of 4 and every base pointer and row stride is 16-byte aligned,
// a scalar arm (VEC = 1) otherwise.
//
// Both are streaming passes (forward 5 floats of traffic per element, backward 7 or 8) with nothing to reuse but b.
// A workgroup is GX_ROWS waves; a wave owns one row of a tile of GX_ROWS rows by 64 chunks, so a wave instruction
// touches 1 KiB (VEC = 4) of consecutive addresses of one row; there is no index division.  blockIdx.x picks the
// 64 chunks, blockIdx.y the first tile of rows, and the workgroup strides over the row tiles: its chunk of b is
// loaded once.  The grid is capped at GX_MAX_WG workgroups (8 per CU).  No atomics, no reduction: two launches on
// the same inputs give the same bits.
#include "fx_common.h"

#define GX_LANES 64               // chunks of a row per workgroup: one wave
#define GX_ROWS 4                 // rows of a tile: the waves of a workgroup
#define GX_MAX_WG 2048            // 8 workgroups per CU

// g = sigmoid(v) and d = g (1 - g) from t = exp(-|v|) in (0, 1]: sigmoid(|v|) = 1 / (1 + t) and sigmoid(-|v|) =
// t / (1 + t), neither of them a difference of nearly equal numbers, and their product is d for either sign:
// finite and accurate in both saturated tails (t underflows to 0 beyond |v| ~ 104: g = 1 or 0, d = 0)
__device__ __forceinline__ void gx_gate(float v, float& g, float& d) {
    const float t = expf(-fabsf(v));
    const float hi = 1.f / (1.f + t);
    const float lo = t * hi;
    g = v >= 0.f ? hi : lo;
    d = hi * lo;
}

struct GxArgs {
    const float* h; int64_t ldh;        // [rows, 2 cols]: u0 | v
    const float* x0; int64_t ldx0;
    const float* xi; int64_t ldxi;      // forward only
    const float* b;                     // [cols]
    float* xn; int64_t ldxn;            // forward only
    const float* dxn; int64_t lddxn;    // backward only, as dh and dx0
    float* dh; int64_t lddh;            // [rows, 2 cols]
    float* dx0; int64_t lddx0;
    int64_t rows;
    int cols;
    int init, add_dxn;
};

// grid (ceil(cols / VEC / GX_LANES), row tiles), block (GX_LANES, GX_ROWS)
template <int VEC>
__global__ __launch_bounds__(GX_LANES * GX_ROWS) void k_gate_cross_fwd(GxArgs p) {
    const int64_t chunk = (int64_t)blockIdx.x * GX_LANES + threadIdx.x;
    if (chunk >= p.cols / VEC) return;
    const int64_t c = chunk * VEC;
    float b[VEC];
    fx_load<VEC>(p.b + c, b);
    for (int64_t r = (int64_t)blockIdx.y * GX_ROWS + threadIdx.y; r < p.rows; r += (int64_t)gridDim.y * GX_ROWS) {
        float u[VEC], v[VEC], x0[VEC], xi[VEC], xn[VEC];
        const float* hr = p.h + r * p.ldh + c;
        fx_load<VEC>(hr, u);
        fx_load<VEC>(hr + p.cols, v);
        fx_load<VEC>(p.x0 + r * p.ldx0 + c, x0);
        fx_load<VEC>(p.xi + r * p.ldxi + c, xi);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float g, d;
            gx_gate(v[k], g, d);
            xn[k] = x0[k] * (u[k] + b[k]) * g + xi[k];
        }
        fx_store<VEC>(p.xn + r * p.ldxn + c, xn);
    }
}

template <int VEC>
__global__ __launch_bounds__(GX_LANES * GX_ROWS) void k_gate_cross_bwd(GxArgs p) {
    const int64_t chunk = (int64_t)blockIdx.x * GX_LANES + threadIdx.x;
    if (chunk >= p.cols / VEC) return;
    const int64_t c = chunk * VEC;
    float b[VEC];
    fx_load<VEC>(p.b + c, b);
    for (int64_t r = (int64_t)blockIdx.y * GX_ROWS + threadIdx.y; r < p.rows; r += (int64_t)gridDim.y * GX_ROWS) {
        float u[VEC], v[VEC], x0[VEC], dy[VEC], du[VEC], dv[VEC], d0[VEC];
        const float* hr = p.h + r * p.ldh + c;
        fx_load<VEC>(hr, u);
        fx_load<VEC>(hr + p.cols, v);
        fx_load<VEC>(p.x0 + r * p.ldx0 + c, x0);
        fx_load<VEC>(p.dxn + r * p.lddxn + c, dy);
        float* out0 = p.dx0 + r * p.lddx0 + c;
        if (p.init) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) d0[k] = 0.f;
        } else {
            fx_load<VEC>(out0, d0);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float g, d;
            gx_gate(v[k], g, d);
            const float uk = u[k] + b[k];
            const float t = dy[k] * x0[k];
            du[k] = t * g;
            dv[k] = t * uk * d;
            float term = dy[k] * uk * g;
            if (p.add_dxn) term += dy[k];
            d0[k] = p.init ? term : d0[k] + term;
        }
        float* dhr = p.dh + r * p.lddh + c;
        fx_store<VEC>(dhr, du);
        fx_store<VEC>(dhr + p.cols, dv);
        fx_store<VEC>(out0, d0);
    }
}

// a [rows, width] matrix with row stride ld
static int gx_check_mat(const char* who, const char* name, const void* ptr, int64_t ld, int64_t width) {
    FX_CHECK_ARG(ptr, "%s: null %s", who, name);
    FX_CHECK_ARG(ld >= width, "%s: %s row stride %lld < %lld", who, name, (long long)ld, (long long)width);
    return FX_OK;
}

static dim3 gx_grid(int64_t rows, int64_t chunks) {
    const int64_t gx = fx_ceil_div(chunks, GX_LANES);
    int64_t gy = fx_ceil_div(rows, GX_ROWS);
    const int64_t cap = GX_MAX_WG / gx > 0 ? GX_MAX_WG / gx : 1;
    if (gy > cap) gy = cap;
    return dim3((unsigned)gx, (unsigned)gy);
}

extern "C" int32_t fx_gate_cross_tile_rows(void) { return GX_ROWS; }

extern "C" int fx_gate_cross_fwd(const float* h, int64_t ldh, const float* x0, int64_t ldx0, const float* xi,
                                 int64_t ldxi, const float* b, float* xn, int64_t ldxn, int64_t rows, int32_t cols,
                                 fx_stream_t stream) {
    const char* who = "fx_gate_cross_fwd";
    FX_CHECK_ARG(cols >= 1, "%s: cols=%d", who, cols);
    FX_CHECK_ARG(rows >= 0, "%s: rows=%lld", who, (long long)rows);
    if (int st = gx_check_mat(who, "h", h, ldh, 2 * (int64_t)cols)) return st;
    if (int st = gx_check_mat(who, "x0", x0, ldx0, cols)) return st;
    if (int st = gx_check_mat(who, "xi", xi, ldxi, cols)) return st;
    if (int st = gx_check_mat(who, "xn", xn, ldxn, cols)) return st;
    FX_CHECK_ARG(b, "%s: null b", who);
    if (rows == 0) return FX_OK;
    GxArgs p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.ldh = ldh; p.x0 = x0; p.ldx0 = ldx0; p.xi = xi; p.ldxi = ldxi; p.b = b;
    p.xn = xn; p.ldxn = ldxn; p.rows = rows; p.cols = cols;
    const bool vec4 = cols % 4 == 0 && fx_vec_ok(h, ldh) && fx_vec_ok(x0, ldx0) && fx_vec_ok(xi, ldxi) &&
                      fx_vec_ok(xn, ldxn) && fx_vec_ok(b, 0);
    const dim3 grid = gx_grid(rows, vec4 ? cols / 4 : cols), block(GX_LANES, GX_ROWS);
    hipStream_t s = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL(k_gate_cross_fwd<4>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_gate_cross_fwd<1>, grid, block, 0, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_gate_cross_bwd(const float* dxn, int64_t lddxn, const float* h, int64_t ldh, const float* x0,
                                 int64_t ldx0, const float* b, float* dh, int64_t lddh, float* dx0, int64_t lddx0,
                                 int64_t rows, int32_t cols, int32_t init, int32_t add_dxn, fx_stream_t stream) {
    const char* who = "fx_gate_cross_bwd";
    FX_CHECK_ARG(cols >= 1, "%s: cols=%d", who, cols);
    FX_CHECK_ARG(rows >= 0, "%s: rows=%lld", who, (long long)rows);
    if (int st = gx_check_mat(who, "dxn", dxn, lddxn, cols)) return st;
    if (int st = gx_check_mat(who, "h", h, ldh, 2 * (int64_t)cols)) return st;
    if (int st = gx_check_mat(who, "x0", x0, ldx0, cols)) return st;
    if (int st = gx_check_mat(who, "dh", dh, lddh, 2 * (int64_t)cols)) return st;
    if (int st = gx_check_mat(who, "dx0", dx0, lddx0, cols)) return st;
    FX_CHECK_ARG(b, "%s: null b", who);
    if (rows == 0) return FX_OK;
    GxArgs p;
    memset(&p, 0, sizeof(p));
    p.dxn = dxn; p.lddxn = lddxn; p.h = h; p.ldh = ldh; p.x0 = x0; p.ldx0 = ldx0; p.b = b;
    p.dh = dh; p.lddh = lddh; p.dx0 = dx0; p.lddx0 = lddx0; p.rows = rows; p.cols = cols;
    p.init = init ? 1 : 0; p.add_dxn = add_dxn ? 1 : 0;
    const bool vec4 = cols % 4 == 0 && fx_vec_ok(dxn, lddxn) && fx_vec_ok(h, ldh) && fx_vec_ok(x0, ldx0) &&
                      fx_vec_ok(dh, lddh) && fx_vec_ok(dx0, lddx0) && fx_vec_ok(b, 0);
    const dim3 grid = gx_grid(rows, vec4 ? cols / 4 : cols), block(GX_LANES, GX_ROWS);
    hipStream_t s = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL(k_gate_cross_bwd<4>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_gate_cross_bwd<1>, grid, block, 0, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
