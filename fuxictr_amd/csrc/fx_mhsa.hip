// fx_mhsa.hip — AutoInt's multi-head self-attention over the fields of one sample, one fused layer per launch
// (model_zoo/AutoInt/src/AutoInt.py:136-191, fuxictr/pytorch/layers/attentions/dot_product_attention.py:24-58):
//     Q = X Wq^T, K = X Wk^T, V = X Wv^T;  per head: P = softmax_rows(Q_h K_h^T [/ sqrt(head_dim)]);  O_h = P V_h
//     Y = concat_h(O_h) (+ X Wres^T | + X);  Y = relu(Y)
// One workgroup of 256 threads works on one sample at a time: X, Q, K, V and the score matrices of a group of
// heads live in LDS, nothing but Y goes to HBM.  The attention itself (weight staging, scores, P V and the loops of
// its backward) is the in-LDS core of fx_attn_lds.h, which fx_bst.hip uses too; this file owns the loading of X with
// the projection, the serial soft-max, the residual / ReLU epilogue and the fused weight-gradient loop.  The backward
// recomputes Q, K, V and P with the forward's own instruction sequence, so the same bits (a log-sum-exp saved per row
// was tried first: at scores of +-80 it costs P half an ulp of 80, 4e-6 relative), keeps the weight gradients of its
// samples in registers (entry e of a matrix belongs to thread e % 256: no atomics), writes them as one partial per
// workgroup and a second launch, the shared fx_rowsum (fx_rowsum.h: four interleaved slices in fp64), sums the
// partials in a fixed order.
#include "fx_attn_lds.h"
#include "fx_rowsum.h"

#define MH_T FX_ATTN_T
#define MH_MAX FX_ATTN_MAX  // F, D_in, A
#define MH_BWD_GRID 512     // workgroups of the backward = rows of the weight-gradient partials
#define MH_FWD_GRID 2048

struct MhsaArgs {
    const float* X;
    int64_t x_ld;
    int64_t B;
    int F, D, A, H, hd, HG, nW;
    const float* W[4];      // Wq, Wk, Wv, Wres (or null), each [A, D]
    float scale;            // 1 or 1 / sqrt(head_dim)
    int residual, relu;
    float* Y;               // fwd: out; bwd: the forward's output (ReLU mask)
    const float* dY;
    float* dX;
    int64_t dx_ld;
    int dx_acc;
    float* partial;         // [grid, nW * A * D]
};

__device__ __forceinline__ FxAttnDims mh_dims(const MhsaArgs& p) { return {p.F, p.D, p.A, p.hd, p.HG, p.scale}; }

// X of sample b -> sX, then Q, K, V = X Wq^T, X Wk^T, X Wv^T.  Private: as a helper of fx_attn_lds.h next to a separate
// load it cost k_mhsa_bwd<false, 16>, which sits at 256 VGPRs, 5.4 %; in this form nothing is slower.
template <bool WLDS>
__device__ __forceinline__ void mh_project(const MhsaArgs& p, const FxAttnW<4, WLDS>& w, int64_t b, float* sX,
                                           float* sQ, float* sK, float* sV) {
    const int F = p.F, D = p.D, A = p.A, XS = D | 1, AS = A | 1;
    const float* x = p.X + b * p.x_ld;
    for (int idx = threadIdx.x; idx < F * D; idx += MH_T) {
        const int f = idx / D, d = idx - f * D;
        sX[f * XS + d] = x[idx];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < F * A; idx += MH_T) {
        const int f = idx / A, a = idx - f * A;
        float q = 0.f, k = 0.f, v = 0.f;
        for (int d = 0; d < D; ++d) {
            const float xv = sX[f * XS + d];
            q = fmaf(xv, w(0, a, d), q);
            k = fmaf(xv, w(1, a, d), k);
            v = fmaf(xv, w(2, a, d), v);
        }
        sQ[f * AS + a] = q;
        sK[f * AS + a] = k;
        sV[f * AS + a] = v;
    }
}

// stable soft-max of one score row in place (row maximum subtracted).  A thread per row, serial maximum and sum:
// fx_bst.hip's wave-per-row soft-max sums in another order, so the two are not one function.
__device__ __forceinline__ void mh_softmax_row(float* row, int F) {
    float m = row[0];
    for (int j = 1; j < F; ++j) m = fmaxf(m, row[j]);
    float sum = 0.f;
    for (int j = 0; j < F; ++j) {
        const float e = expf(row[j] - m);
        row[j] = e;
        sum += e;
    }
    for (int j = 0; j < F; ++j) row[j] = row[j] / sum;
}

// (the weights always fit into LDS next to the forward's image: at most 149 760 bytes, at F = D = A = 64 with a
// W_res, over every F, D, A <= 64 — so the forward has no instantiation that reads them from HBM)
__global__ __launch_bounds__(MH_T) void k_mhsa_fwd(MhsaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FxAttnDims g = mh_dims(p);
    const int F = p.F, D = p.D, A = p.A, XS = D | 1, AS = A | 1, FS = F | 1;
    float* sX = smem;
    float* sQ = sX + F * XS;
    float* sK = sQ + F * AS;
    float* sV = sK + F * AS;
    float* sS = sV + F * AS;
    float* sW = sS + p.HG * F * FS;
    const FxAttnW<4, true> w = fx_attn_weights<4, true>(p.W, p.nW, A, D, sW);
    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        __syncthreads();
        mh_project<true>(p, w, b, sX, sQ, sK, sV);
        for (int h0 = 0; h0 < p.H; h0 += p.HG) {
            const int hg = p.H - h0 < p.HG ? p.H - h0 : p.HG;
            __syncthreads();
            fx_attn_scores(g, h0, hg, sQ, sK, sS);
            __syncthreads();
            for (int idx = threadIdx.x; idx < hg * F; idx += MH_T) mh_softmax_row(sS + idx * FS, F);
            __syncthreads();
            // this file's epilogue: the residual and the ReLU on the way to Y
            fx_attn_pv(g, h0, hg, sS, sV, [&](int i, int a, float o) {
                if (p.residual) {
                    if (p.W[3] != nullptr) {
                        float r2 = 0.f;
                        for (int d = 0; d < D; ++d) r2 = fmaf(sX[i * XS + d], w(3, a, d), r2);
                        o += r2;
                    } else {
                        o += sX[i * XS + a];
                    }
                }
                if (p.relu) o = fmaxf(o, 0.f);
                p.Y[(b * F + i) * A + a] = o;
            });
        }
    }
}

// R: weight-gradient entries per thread and matrix (A * D <= 256 R)
template <bool WLDS, int R>
__global__ __launch_bounds__(MH_T) void k_mhsa_bwd(MhsaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FxAttnDims g = mh_dims(p);
    const int F = p.F, D = p.D, A = p.A, XS = D | 1, AS = A | 1, FS = F | 1;
    float* sX = smem;
    float* sQ = sX + F * XS;
    float* sK = sQ + F * AS;
    float* sV = sK + F * AS;          // V, then dV (head by head)
    float* sG = sV + F * AS;          // dY through the ReLU: the gradient of the pre-activation output
    float* sdQ = sG + F * AS;
    float* sdK = sdQ + F * AS;
    float* sP = sdK + F * AS;
    float* sD = sP + p.HG * F * FS;   // dP, then dS
    float* sW = sD + p.HG * F * FS;
    const FxAttnW<4, WLDS> w = fx_attn_weights<4, WLDS>(p.W, p.nW, A, D, sW);
    const bool wres = p.W[3] != nullptr;
    float acc[4][R];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;

    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < F * A; idx += MH_T) {
            const int f = idx / A, a = idx - f * A;
            float gy = p.dY[b * F * A + idx];
            if (p.relu && !(p.Y[b * F * A + idx] > 0.f)) gy = 0.f;
            sG[f * AS + a] = gy;
        }
        mh_project<WLDS>(p, w, b, sX, sQ, sK, sV);
        for (int h0 = 0; h0 < p.H; h0 += p.HG) {
            const int hg = p.H - h0 < p.HG ? p.H - h0 : p.HG;
            __syncthreads();
            fx_attn_scores(g, h0, hg, sQ, sK, sP);
            fx_attn_dp(g, h0, hg, sG, sV, sD);
            __syncthreads();
            // row by row: P = softmax(S), then dS = P (dP - sum_j P dP) * scale
            for (int idx = threadIdx.x; idx < hg * F; idx += MH_T) {
                float* pr = sP + idx * FS;
                float* dr = sD + idx * FS;
                mh_softmax_row(pr, F);
                float delta = 0.f;
                for (int j = 0; j < F; ++j) delta = fmaf(pr[j], dr[j], delta);
                for (int j = 0; j < F; ++j) dr[j] = pr[j] * (dr[j] - delta) * p.scale;
            }
            __syncthreads();
            fx_attn_dqkv(g, h0, hg, sP, sD, sG, sQ, sK, sV, sdQ, sdK);
        }
        __syncthreads();
        // dX = dQ Wq + dK Wk + dV Wv (+ dO Wres | + dO)
        fx_attn_dx(g, w, sdQ, sdK, sV, [&](int f, int d, float s) {
            if (p.residual) {
                if (wres) {
                    float r2 = 0.f;
                    for (int a = 0; a < A; ++a) r2 = fmaf(sG[f * AS + a], w(3, a, d), r2);
                    s += r2;
                } else {
                    s += sG[f * AS + d];
                }
            }
            float* dx = p.dX + b * p.dx_ld + (f * D + d);
            *dx = p.dx_acc ? *dx + s : s;
        });
        // dW*[a][d] += sum_f d*[f][a] X[f][d], all four in one loop over f.  fx_attn_acc_dw per matrix (same bits) timed
        // 13 % faster at R = 16 but 0.3 % slower at the Criteo shape (R = 4), outside its spread: the fused loop stays.
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = threadIdx.x + r * MH_T;
            if (e < A * D) {
                const int a = e / D, d = e - a * D;
                float tq = 0.f, tk = 0.f, tv = 0.f, tr = 0.f;
                for (int f = 0; f < F; ++f) {
                    const float xv = sX[f * XS + d];
                    tq = fmaf(sdQ[f * AS + a], xv, tq);
                    tk = fmaf(sdK[f * AS + a], xv, tk);
                    tv = fmaf(sV[f * AS + a], xv, tv);
                    tr = fmaf(sG[f * AS + a], xv, tr);
                }
                acc[0][r] += tq;
                acc[1][r] += tk;
                acc[2][r] += tv;
                acc[3][r] += tr;
            }
        }
    }
    float* part = p.partial + (int64_t)blockIdx.x * p.nW * A * D;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = threadIdx.x + r * MH_T;
        if (e < A * D) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < p.nW) part[m * A * D + e] = acc[m][r];
        }
    }
}

static int mh_check(const char* who, const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* Wq,
                    const float* Wk, const float* Wv, int32_t A, int32_t H) {
    FX_CHECK_ARG(F >= 1 && F <= MH_MAX, "%s: F=%d, limit 1 <= F <= 64", who, F);
    FX_CHECK_ARG(D >= 1 && D <= MH_MAX, "%s: D_in=%d, limit 1 <= D_in <= 64", who, D);
    FX_CHECK_ARG(A >= 1 && A <= MH_MAX, "%s: A=%d, limit 1 <= A <= 64", who, A);
    FX_CHECK_ARG(H >= 1 && A % H == 0, "%s: H=%d does not divide A=%d", who, H, A);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(B == 0 || (X && Wq && Wk && Wv), "%s: null X / Wq / Wk / Wv", who);
    FX_CHECK_ARG(x_ld >= (int64_t)F * D, "%s: sample stride %lld < F*D_in", who, (long long)x_ld);
    return FX_OK;
}

static MhsaArgs mh_args(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D, const float* Wq,
                        const float* Wk, const float* Wv, const float* Wres, int32_t A, int32_t H,
                        int32_t use_scale, int32_t residual, int32_t relu) {
    MhsaArgs p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.x_ld = x_ld; p.B = B;
    p.F = F; p.D = D; p.A = A; p.H = H; p.hd = A / H;
    p.HG = fx_attn_heads_per_pass(F, H);
    p.W[0] = Wq; p.W[1] = Wk; p.W[2] = Wv; p.W[3] = (residual && Wres) ? Wres : nullptr;
    p.nW = p.W[3] ? 4 : 3;
    p.scale = use_scale ? (float)(1.0 / sqrt((double)p.hd)) : 1.f;
    p.residual = residual ? 1 : 0;
    p.relu = relu ? 1 : 0;
    return p;
}

// LDS: X and n_rows [F, A] arrays, n_score score buffers (+ the weights)
static inline FxAttnLds mh_lds(const MhsaArgs& p, int n_rows, int n_score) {
    const size_t n = fx_attn_lds_floats(p.F, p.D, p.A, n_rows, n_score, fx_attn_score_floats(p.F, p.HG), 0);
    return fx_attn_lds(n, p.nW, p.A, p.D);
}

extern "C" int64_t fx_mhsa_workspace_floats(int64_t B, int32_t D_in, int32_t A, int32_t has_wres) {
    const int64_t G = B < MH_BWD_GRID ? (B > 0 ? B : 1) : MH_BWD_GRID;
    return G * (has_wres ? 4 : 3) * (int64_t)A * D_in;
}

extern "C" int fx_mhsa_fwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D_in, const float* Wq,
                           const float* Wk, const float* Wv, const float* Wres, int32_t A, int32_t H,
                           int32_t use_scale, int32_t residual, int32_t relu, float* Y,
                           fx_stream_t stream) {
    if (int st = mh_check("fx_mhsa_fwd", X, x_ld, B, F, D_in, Wq, Wk, Wv, A, H)) return st;
    FX_CHECK_ARG(!residual || Wres || D_in == A, "fx_mhsa_fwd: identity residual needs D_in == A (%d, %d)", D_in, A);
    FX_CHECK_ARG(B == 0 || Y, "fx_mhsa_fwd: null Y");
    if (B == 0) return FX_OK;
    MhsaArgs p = mh_args(X, x_ld, B, F, D_in, Wq, Wk, Wv, Wres, A, H, use_scale, residual, relu);
    p.Y = Y;
    // Q, K, V, one score buffer and the weights: see k_mhsa_fwd (the check only guards a later change of the limits)
    const FxAttnLds l = mh_lds(p, 3, 1);
    FX_CHECK_ARG(l.wlds, "fx_mhsa_fwd: %zu bytes of LDS without the weights", l.bytes);
    const unsigned grid = (unsigned)(B < MH_FWD_GRID ? B : MH_FWD_GRID);
    return fx_attn_launch<k_mhsa_fwd>(p, grid, l.bytes, fx_hip_stream(stream));
}

template <bool WLDS>
static int mh_launch_bwd(const MhsaArgs& p, unsigned grid, size_t lds, hipStream_t s) {
    const int AD = p.A * p.D;
    if (AD <= MH_T) return fx_attn_launch<k_mhsa_bwd<WLDS, 1>>(p, grid, lds, s);
    if (AD <= 4 * MH_T) return fx_attn_launch<k_mhsa_bwd<WLDS, 4>>(p, grid, lds, s);
    return fx_attn_launch<k_mhsa_bwd<WLDS, 16>>(p, grid, lds, s);
}

extern "C" int fx_mhsa_bwd(const float* X, int64_t x_ld, int64_t B, int32_t F, int32_t D_in, const float* Wq,
                           const float* Wk, const float* Wv, const float* Wres, int32_t A, int32_t H,
                           int32_t use_scale, int32_t residual, int32_t relu, const float* Y,
                           const float* dY, float* dX, int64_t dx_ld, int32_t dx_accumulate, float* dW,
                           float* workspace, fx_stream_t stream) {
    if (int st = mh_check("fx_mhsa_bwd", X, x_ld, B, F, D_in, Wq, Wk, Wv, A, H)) return st;
    FX_CHECK_ARG(!residual || Wres || D_in == A, "fx_mhsa_bwd: identity residual needs D_in == A (%d, %d)", D_in, A);
    FX_CHECK_ARG(B > 0, "fx_mhsa_bwd: B=%lld", (long long)B);
    FX_CHECK_ARG(dY && dX && dW && workspace, "fx_mhsa_bwd: null dY / dX / dW / workspace");
    FX_CHECK_ARG(!relu || Y, "fx_mhsa_bwd: the ReLU mask needs the forward's Y");
    FX_CHECK_ARG(dx_ld >= (int64_t)F * D_in, "fx_mhsa_bwd: dX sample stride %lld < F*D_in", (long long)dx_ld);
    MhsaArgs p = mh_args(X, x_ld, B, F, D_in, Wq, Wk, Wv, Wres, A, H, use_scale, residual, relu);
    p.Y = const_cast<float*>(Y);
    p.dY = dY;
    p.dX = dX;
    p.dx_ld = dx_ld;
    p.dx_acc = dx_accumulate ? 1 : 0;
    p.partial = workspace;
    // six [F, A] arrays and two score buffers (P, dP | dS); the weights join them in LDS when all of it fits
    const FxAttnLds l = mh_lds(p, 6, 2);
    const unsigned grid = (unsigned)(B < MH_BWD_GRID ? B : MH_BWD_GRID);
    hipStream_t s = fx_hip_stream(stream);
    const int st = l.wlds ? mh_launch_bwd<true>(p, grid, l.bytes, s) : mh_launch_bwd<false>(p, grid, l.bytes, s);
    if (st) return st;
    const int n = p.nW * A * D_in;
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)grid, n, fx_rowsum_out(dW, n));
}
