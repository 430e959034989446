// fx_mhsa.hip — AutoInt's multi-head self-attention over the fields of one sample, one fused layer per launch
// (model_zoo/AutoInt/src/AutoInt.py:136-191, fuxictr/pytorch/layers/attentions/dot_product_attention.py:24-58):
//     Q = X Wq^T, K = X Wk^T, V = X Wv^T;  per head: P = softmax_rows(Q_h K_h^T [/ sqrt(head_dim)]);  O_h = P V_h
//     Y = concat_h(O_h) (+ X Wres^T | + X);  Y = relu(Y)
// One workgroup of 256 threads works on one sample at a time: X, Q, K, V and the score matrices of a group of
// heads live in LDS, nothing but Y goes to HBM.  The backward recomputes Q, K, V and P with the forward's own
// instruction sequence, so the same bits (a log-sum-exp saved per row was tried first: at scores of +-80 it costs P
// half an ulp of 80, 4e-6 relative), keeps the weight gradients of its samples in registers (entry e of a matrix
// belongs to thread e % 256: no atomics), writes them as one partial per workgroup and a second launch, the shared
// fx_rowsum (fx_rowsum.h: four interleaved slices in fp64), sums the partials in a fixed order.
// fp32 FMAs out of LDS; every LDS row has an odd stride so that both the row-wise and the column-wise walks of
// a phase are free of bank conflicts.
#include "fx_common.h"
#include "fx_rowsum.h"

#define MH_T 256            // threads per workgroup
#define MH_MAX 64           // F, D_in, A
#define MH_SBUF (64 * 65)   // floats of one score buffer: the heads of a group share it
#define MH_BWD_GRID 512     // workgroups of the backward = rows of the weight-gradient partials
#define MH_FWD_GRID 2048
#define MH_LDS_MAX (160 * 1024)

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

static inline int mh_odd(int n) { return n | 1; }
static inline int mh_heads_per_pass(int F, int H) {
    const int hg = MH_SBUF / (F * mh_odd(F));
    return hg < H ? hg : H;
}
// floats of LDS: X + n_rows [F, A] arrays + n_score score buffers (+ the weights)
static inline size_t mh_lds_floats(int F, int D, int A, int HG, int nW, int n_rows, int n_score, bool wlds) {
    size_t n = (size_t)F * mh_odd(D) + (size_t)n_rows * F * mh_odd(A) + (size_t)n_score * HG * F * mh_odd(F);
    if (wlds) n += (size_t)nW * A * mh_odd(D);
    return n;
}

template <bool WLDS>
struct MhsaW {
    const float* w[4];
    int ld;
    __device__ __forceinline__ float operator()(int m, int a, int d) const { return w[m][a * ld + d]; }
};

template <bool WLDS>
__device__ __forceinline__ MhsaW<WLDS> mh_weights(const MhsaArgs& p, float* sW) {
    MhsaW<WLDS> w;
    if constexpr (WLDS) {
        const int WS = p.D | 1, AD = p.A * p.D;
        for (int idx = threadIdx.x; idx < p.nW * AD; idx += MH_T) {
            const int m = idx / AD, r = idx - m * AD, a = r / p.D, d = r - a * p.D;
            sW[(m * p.A + a) * WS + d] = p.W[m][r];
        }
        for (int m = 0; m < 4; ++m) w.w[m] = sW + m * p.A * WS;
        w.ld = WS;
    } else {
        for (int m = 0; m < 4; ++m) w.w[m] = p.W[m];
        w.ld = p.D;
    }
    return w;
}

// X of sample b -> sX, then Q, K, V
template <bool WLDS>
__device__ __forceinline__ void mh_project(const MhsaArgs& p, const MhsaW<WLDS>& w, int64_t b, float* sX,
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

// stable soft-max of one score row in place (row maximum subtracted)
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

// scores of the heads h0 .. h0+hg-1: sS[hh][i][j] = scale * Q_i . K_j
__device__ __forceinline__ void mh_scores(const MhsaArgs& p, int h0, int hg, const float* sQ, const float* sK,
                                          float* sS) {
    const int F = p.F, AS = p.A | 1, FS = F | 1, hd = p.hd, FF = F * F;
    for (int idx = threadIdx.x; idx < hg * FF; idx += MH_T) {
        const int hh = idx / FF, r = idx - hh * FF, i = r / F, j = r - i * F;
        const float* q = sQ + i * AS + (h0 + hh) * hd;
        const float* k = sK + j * AS + (h0 + hh) * hd;
        float s = 0.f;
        for (int c = 0; c < hd; ++c) s = fmaf(q[c], k[c], s);
        sS[(hh * F + i) * FS + j] = s * p.scale;
    }
}

template <bool WLDS>
__global__ __launch_bounds__(MH_T) void k_mhsa_fwd(MhsaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = p.F, D = p.D, A = p.A, XS = D | 1, AS = A | 1, FS = F | 1, hd = p.hd;
    float* sX = smem;
    float* sQ = sX + F * XS;
    float* sK = sQ + F * AS;
    float* sV = sK + F * AS;
    float* sS = sV + F * AS;
    float* sW = sS + p.HG * F * FS;
    const MhsaW<WLDS> w = mh_weights<WLDS>(p, sW);
    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        __syncthreads();
        mh_project<WLDS>(p, w, b, sX, sQ, sK, sV);
        for (int h0 = 0; h0 < p.H; h0 += p.HG) {
            const int hg = p.H - h0 < p.HG ? p.H - h0 : p.HG;
            __syncthreads();
            mh_scores(p, h0, hg, sQ, sK, sS);
            __syncthreads();
            for (int idx = threadIdx.x; idx < hg * F; idx += MH_T) mh_softmax_row(sS + idx * FS, F);   // a thread per row
            __syncthreads();
            const int GW = hg * hd;                // this group's columns of Y: a0 .. a0 + GW
            const int a0 = h0 * hd;
            for (int idx = threadIdx.x; idx < F * GW; idx += MH_T) {
                const int i = idx / GW, r = idx - i * GW, hh = r / hd, a = a0 + r;
                const float* prow = sS + (hh * F + i) * FS;
                float o = 0.f;
                for (int j = 0; j < F; ++j) o = fmaf(prow[j], sV[j * AS + a], o);
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
            }
        }
    }
}

// R: weight-gradient entries per thread and matrix (A * D <= 256 R)
template <bool WLDS, int R>
__global__ __launch_bounds__(MH_T) void k_mhsa_bwd(MhsaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = p.F, D = p.D, A = p.A, XS = D | 1, AS = A | 1, FS = F | 1, hd = p.hd, FF = F * F;
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
    const MhsaW<WLDS> w = mh_weights<WLDS>(p, sW);
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
            float g = p.dY[b * F * A + idx];
            if (p.relu && !(p.Y[b * F * A + idx] > 0.f)) g = 0.f;
            sG[f * AS + a] = g;
        }
        mh_project<WLDS>(p, w, b, sX, sQ, sK, sV);
        for (int h0 = 0; h0 < p.H; h0 += p.HG) {
            const int hg = p.H - h0 < p.HG ? p.H - h0 : p.HG;
            const int GW = hg * hd, a0 = h0 * hd;
            __syncthreads();
            mh_scores(p, h0, hg, sQ, sK, sP);
            // dP[i][j] = dO_i . V_j
            for (int idx = threadIdx.x; idx < hg * FF; idx += MH_T) {
                const int hh = idx / FF, r = idx - hh * FF, i = r / F, j = r - i * F;
                const float* g = sG + i * AS + (h0 + hh) * hd;
                const float* v = sV + j * AS + (h0 + hh) * hd;
                float s = 0.f;
                for (int c = 0; c < hd; ++c) s = fmaf(g[c], v[c], s);
                sD[(hh * F + i) * FS + j] = s;
            }
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
            // dV[j][a] = sum_i P[i][j] dO[i][a], over V in place (dP is done with it)
            for (int idx = threadIdx.x; idx < F * GW; idx += MH_T) {
                const int j = idx / GW, r = idx - j * GW, hh = r / hd, a = a0 + r;
                const float* pc = sP + hh * F * FS + j;
                float s = 0.f;
                for (int i = 0; i < F; ++i) s = fmaf(pc[i * FS], sG[i * AS + a], s);
                sV[j * AS + a] = s;
            }
            // dQ[i][a] = sum_j dS[i][j] K[j][a];  dK[i][a] = sum_j dS[j][i] Q[j][a]
            for (int idx = threadIdx.x; idx < F * GW; idx += MH_T) {
                const int i = idx / GW, r = idx - i * GW, hh = r / hd, a = a0 + r;
                const float* ds = sD + hh * F * FS;
                float dq = 0.f, dk = 0.f;
                for (int j = 0; j < F; ++j) {
                    dq = fmaf(ds[i * FS + j], sK[j * AS + a], dq);
                    dk = fmaf(ds[j * FS + i], sQ[j * AS + a], dk);
                }
                sdQ[i * AS + a] = dq;
                sdK[i * AS + a] = dk;
            }
        }
        __syncthreads();
        // dX = dQ Wq + dK Wk + dV Wv (+ dO Wres | + dO)
        for (int idx = threadIdx.x; idx < F * D; idx += MH_T) {
            const int f = idx / D, d = idx - f * D;
            float s = 0.f;
            for (int a = 0; a < A; ++a) {
                s = fmaf(sdQ[f * AS + a], w(0, a, d), s);
                s = fmaf(sdK[f * AS + a], w(1, a, d), s);
                s = fmaf(sV[f * AS + a], w(2, a, d), s);
            }
            if (p.residual) {
                if (wres) {
                    float r2 = 0.f;
                    for (int a = 0; a < A; ++a) r2 = fmaf(sG[f * AS + a], w(3, a, d), r2);
                    s += r2;
                } else {
                    s += sG[f * AS + d];
                }
            }
            float* dx = p.dX + b * p.dx_ld + idx;
            *dx = p.dx_acc ? *dx + s : s;
        }
        // dW*[a][d] += sum_f d*[f][a] X[f][d]: this sample's sum first, then onto the running one
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
    p.HG = mh_heads_per_pass(F, H);
    p.W[0] = Wq; p.W[1] = Wk; p.W[2] = Wv; p.W[3] = (residual && Wres) ? Wres : nullptr;
    p.nW = p.W[3] ? 4 : 3;
    p.scale = use_scale ? (float)(1.0 / sqrt((double)p.hd)) : 1.f;
    p.residual = residual ? 1 : 0;
    p.relu = relu ? 1 : 0;
    return p;
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
    const bool wlds = 4 * mh_lds_floats(F, D_in, A, p.HG, p.nW, 3, 1, true) <= MH_LDS_MAX;
    const size_t lds = 4 * mh_lds_floats(F, D_in, A, p.HG, p.nW, 3, 1, wlds);
    const unsigned grid = (unsigned)(B < MH_FWD_GRID ? B : MH_FWD_GRID);
    // (once per process: both instantiations may use the whole 160 KiB, the largest image any shape needs)
    static const hipError_t lds_ok[2] = {fx_allow_lds(k_mhsa_fwd<false>, MH_LDS_MAX),
                                         fx_allow_lds(k_mhsa_fwd<true>, MH_LDS_MAX)};
    FX_CHECK_HIP(lds_ok[wlds ? 1 : 0]);
    if (wlds) hipLaunchKernelGGL(k_mhsa_fwd<true>, dim3(grid), dim3(MH_T), lds, fx_hip_stream(stream), p);
    else hipLaunchKernelGGL(k_mhsa_fwd<false>, dim3(grid), dim3(MH_T), lds, fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

template <bool WLDS>
static int mh_launch_bwd(const MhsaArgs& p, unsigned grid, size_t lds, hipStream_t s) {
    const int AD = p.A * p.D;
#define FX_MHSA_BWD(RR)                                                                                  \
    do {                                                                                                 \
        static const hipError_t lds_ok = fx_allow_lds(k_mhsa_bwd<WLDS, RR>, MH_LDS_MAX);                 \
        FX_CHECK_HIP(lds_ok);                                                                            \
        hipLaunchKernelGGL((k_mhsa_bwd<WLDS, RR>), dim3(grid), dim3(MH_T), lds, s, p);                   \
    } while (0)
    if (AD <= MH_T) FX_MHSA_BWD(1);
    else if (AD <= 4 * MH_T) FX_MHSA_BWD(4);
    else FX_MHSA_BWD(16);
#undef FX_MHSA_BWD
    FX_CHECK_LAUNCH();
    return FX_OK;
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
    const bool wlds = 4 * mh_lds_floats(F, D_in, A, p.HG, p.nW, 6, 2, true) <= MH_LDS_MAX;
    const size_t lds = 4 * mh_lds_floats(F, D_in, A, p.HG, p.nW, 6, 2, wlds);
    const unsigned grid = (unsigned)(B < MH_BWD_GRID ? B : MH_BWD_GRID);
    hipStream_t s = fx_hip_stream(stream);
    if (int st = wlds ? mh_launch_bwd<true>(p, grid, lds, s) : mh_launch_bwd<false>(p, grid, lds, s)) return st;
    const int n = p.nW * A * D_in;
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)grid, n, fx_rowsum_out(dW, n));
}
