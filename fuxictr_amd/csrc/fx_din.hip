// fx_din.hip — DIN target attention, first native version: the attention MLP runs on
// the fp32 MFMA GEMM with Dice (fx_dice.hip) between its layers, the concatenation in front of it and
// the masked pooling behind it are here.
//
// Reference (paths relative to the reference checkout):
//   fuxictr/pytorch/layers/attentions/target_attention.py:66-92   DIN_Attention.forward
//       x_{b,l} = [q_b, k_{b,l}, q_b - k_{b,l}, q_b * k_{b,l}]  -> MLP(4E -> H Dice -> 1) -> * mask
//       -> out_b = sum_l w_{b,l} k_{b,l}
#include "fx_common.h"

// ---------------------------------------------------------------------------------------------
// attention input [B*L, 4E] and its backward
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_din_concat_fwd(const float* q, int64_t q_ld,
                                                        const float* K, int64_t k_ldb,
                                                        int64_t k_ldl, int L, int E, int64_t n,
                                                        float* out) {
    // one thread per (row = b*L + l, e)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / E;
        const int e = (int)(i - row * E);
        const int64_t b = row / L;
        const int l = (int)(row - b * L);
        const float qv = q[b * q_ld + e];
        const float kv = K[b * k_ldb + (int64_t)l * k_ldl + e];
        float* o = out + row * 4 * E;
        o[e] = qv;
        o[E + e] = kv;
        o[2 * E + e] = qv - kv;
        o[3 * E + e] = qv * kv;
    }
}

// dK[b,l,e] = dx_k - dx_d + dx_p * q ;  dq[b,e] = sum_l (dx_q + dx_d + dx_p * k)  (16 lanes? no:
// one thread per (b,e) loops over l for dq — L is a padded max_len (50), the loop is short)
__global__ __launch_bounds__(256) void k_din_concat_bwd(const float* dx, const float* q,
                                                        int64_t q_ld, const float* K,
                                                        int64_t k_ldb, int64_t k_ldl, int L, int E,
                                                        int64_t B, float* dq, float* dK,
                                                        int64_t dk_ldb, int64_t dk_ldl,
                                                        int accumulate_dk) {
    const int64_t n = B * E;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / E;
        const int e = (int)(i - b * E);
        const float qv = q[b * q_ld + e];
        float acc = 0.f;
        for (int l = 0; l < L; ++l) {
            const float* d = dx + (b * L + l) * 4 * E;
            const float kv = K[b * k_ldb + (int64_t)l * k_ldl + e];
            const float dxq = d[e], dxk = d[E + e], dxd = d[2 * E + e], dxp = d[3 * E + e];
            acc += dxq + dxd + dxp * kv;
            float* o = dK + b * dk_ldb + (int64_t)l * dk_ldl + e;
            const float g = dxk - dxd + dxp * qv;
            *o = accumulate_dk ? *o + g : g;
        }
        dq[i] = acc;
    }
}

extern "C" int fx_din_concat_fwd(const float* q, int64_t q_ld, const float* K, int64_t k_ldb,
                                 int64_t k_ldl, int64_t B, int32_t L, int32_t E, float* out,
                                 fx_stream_t stream) {
    FX_CHECK_ARG(L >= 1 && E >= 1 && B >= 0, "fx_din_concat_fwd: bad sizes");
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(q && K && out, "fx_din_concat_fwd: null pointer");
    const int64_t n = B * L * E;
    int64_t blocks = fx_ceil_div(n, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_din_concat_fwd, dim3((unsigned)blocks), dim3(256), 0,
                       fx_hip_stream(stream), q, q_ld, K, k_ldb, k_ldl, (int)L, (int)E, n, out);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_din_concat_bwd(const float* dx, const float* q, int64_t q_ld, const float* K,
                                 int64_t k_ldb, int64_t k_ldl, int64_t B, int32_t L, int32_t E,
                                 float* dq, float* dK, int64_t dk_ldb, int64_t dk_ldl,
                                 int32_t accumulate_dk, fx_stream_t stream) {
    FX_CHECK_ARG(L >= 1 && E >= 1 && B >= 0, "fx_din_concat_bwd: bad sizes");
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(dx && q && K && dq && dK, "fx_din_concat_bwd: null pointer");
    int64_t blocks = fx_ceil_div(B * E, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_din_concat_bwd, dim3((unsigned)blocks), dim3(256), 0,
                       fx_hip_stream(stream), dx, q, q_ld, K, k_ldb, k_ldl, (int)L, (int)E, B, dq,
                       dK, dk_ldb, dk_ldl, (int)accumulate_dk);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------
// masked weighted sum over the sequence and its backward
//   out[b,e] = sum_l w[b,l] * mask[b,l] * K[b,l,e]
//   dw[b,l]  = mask[b,l] * sum_e dout[b,e] K[b,l,e] ;  dK[b,l,e] (+)= w[b,l] mask[b,l] dout[b,e]
// mask is given through the raw id column (id != 0), like `X[seq_field].long() != 0` (DIN.py:125)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_din_pool_fwd(const float* w, const int32_t* ids,
                                                      int64_t ids_ld, const float* K,
                                                      int64_t k_ldb, int64_t k_ldl, int L, int E,
                                                      int64_t B, float* out) {
    const int64_t n = B * E;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / E;
        const int e = (int)(i - b * E);
        float acc = 0.f;
        for (int l = 0; l < L; ++l) {
            const float m = ids[b * ids_ld + l] != 0 ? 1.f : 0.f;
            acc += (w[b * L + l] * m) * K[b * k_ldb + (int64_t)l * k_ldl + e];
        }
        out[i] = acc;
    }
}

__global__ __launch_bounds__(256) void k_din_pool_bwd(const float* w, const int32_t* ids,
                                                      int64_t ids_ld, const float* K,
                                                      int64_t k_ldb, int64_t k_ldl,
                                                      const float* dout, int L, int E, int Ep,
                                                      int64_t B, float* dw, float* dK,
                                                      int64_t dk_ldb, int64_t dk_ldl) {
    // Ep (power of two >= E) lanes per (b,l)
    const int sub = threadIdx.x & (Ep - 1);
    const int64_t per_block = 256 / Ep;
    const int64_t n = B * L;
    const int64_t n_iter = (n + per_block * gridDim.x - 1) / (per_block * gridDim.x);
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t row = (it * gridDim.x + blockIdx.x) * per_block + threadIdx.x / Ep;
        const bool valid = row < n;
        float dot = 0.f;
        if (valid && sub < E) {
            const int64_t b = row / L;
            const int l = (int)(row - b * L);
            const float m = ids[b * ids_ld + l] != 0 ? 1.f : 0.f;
            const float kv = K[b * k_ldb + (int64_t)l * k_ldl + sub];
            const float dv = dout[b * E + sub];
            dot = m * dv * kv;
            dK[b * dk_ldb + (int64_t)l * dk_ldl + sub] = (w[row] * m) * dv;
        }
        for (int off = 1; off < Ep; off <<= 1) dot += __shfl_xor(dot, off, 64);
        if (valid && sub == 0) dw[row] = dot;
    }
}

extern "C" int fx_din_pool_fwd(const float* w, const int32_t* ids, int64_t ids_ld, const float* K,
                               int64_t k_ldb, int64_t k_ldl, int64_t B, int32_t L, int32_t E,
                               float* out, fx_stream_t stream) {
    FX_CHECK_ARG(L >= 1 && E >= 1 && B >= 0, "fx_din_pool_fwd: bad sizes");
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(w && ids && K && out, "fx_din_pool_fwd: null pointer");
    int64_t blocks = fx_ceil_div(B * E, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_din_pool_fwd, dim3((unsigned)blocks), dim3(256), 0, fx_hip_stream(stream),
                       w, ids, ids_ld, K, k_ldb, k_ldl, (int)L, (int)E, B, out);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_din_pool_bwd(const float* w, const int32_t* ids, int64_t ids_ld, const float* K,
                               int64_t k_ldb, int64_t k_ldl, const float* dout, int64_t B,
                               int32_t L, int32_t E, float* dw, float* dK, int64_t dk_ldb,
                               int64_t dk_ldl, fx_stream_t stream) {
    FX_CHECK_ARG(L >= 1 && E >= 1 && E <= 64 && B >= 0, "fx_din_pool_bwd: bad sizes (E <= 64)");
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(w && ids && K && dout && dw && dK, "fx_din_pool_bwd: null pointer");
    int Ep = 1;
    while (Ep < E) Ep <<= 1;
    int64_t blocks = fx_ceil_div(B * L, 256 / Ep);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_din_pool_bwd, dim3((unsigned)blocks), dim3(256), 0, fx_hip_stream(stream),
                       w, ids, ids_ld, K, k_ldb, k_ldl, dout, (int)L, (int)E, Ep, B, dw, dK, dk_ldb,
                       dk_ldl);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
