// fx_dense_misc.hip — the dense tower's kernels that are no GEMM: column sums (the bias gradient), the ReLU
// backward mask, the CrossNetV2 backward glue, sigmoid + BCE, and the fused head of the training step
// (Linear(K -> 1) forward + sigmoid + BCE + the head's backward in one pass).
#include "fx_common.h"
#include "fx_rowsum.h"

// ---------------------------------------------------------------------------------------------
// column sums (bias gradient), two deterministic stages: FX_COLSUM_CHUNKS row chunks, then fx_rowsum over them
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_colsum_stage1(const float* X, int64_t ldx, int64_t M,
                                                       int64_t N, int64_t rows_per_chunk,
                                                       float* ws) {
    __shared__ float red[256];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * 64 + tx;
    const int64_t mb = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t me = (mb + rows_per_chunk < M) ? mb + rows_per_chunk : M;
    float acc = 0.f;
    if (n < N)
        for (int64_t m = mb + ty; m < me; m += 4) acc += X[m * ldx + n];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (ty == 0 && n < N)
        ws[(int64_t)blockIdx.y * N + n] = (red[tx] + red[tx + 64]) + (red[tx + 128] + red[tx + 192]);
}

// vectorised variant: a thread owns 4 adjacent columns (N % 4 == 0, 16-B aligned rows)
__global__ __launch_bounds__(256) void k_colsum_stage1_v4(const float* X, int64_t ldx, int64_t M,
                                                          int64_t N, int64_t rows_per_chunk,
                                                          float* ws) {
    __shared__ float4 red[256];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t n = ((int64_t)blockIdx.x * 64 + tx) * 4;
    const int64_t mb = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t me = (mb + rows_per_chunk < M) ? mb + rows_per_chunk : M;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < N)
        for (int64_t m = mb + ty; m < me; m += 4) {
            const float4 v = *reinterpret_cast<const float4*>(X + m * ldx + n);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (ty == 0 && n < N) {
        const float4 a0 = red[tx], a1 = red[tx + 64], a2 = red[tx + 128], a3 = red[tx + 192];
        float4 r;
        r.x = (a0.x + a1.x) + (a2.x + a3.x);
        r.y = (a0.y + a1.y) + (a2.y + a3.y);
        r.z = (a0.z + a1.z) + (a2.z + a3.z);
        r.w = (a0.w + a1.w) + (a2.w + a3.w);
        *reinterpret_cast<float4*>(ws + (int64_t)blockIdx.y * N + n) = r;
    }
}

extern "C" int fx_colsum(const float* X, int64_t ldx, int64_t M, int64_t N, float* out,
                         float* workspace, fx_stream_t stream) {
    FX_CHECK_ARG(M >= 0 && N >= 0, "fx_colsum: negative dimension");
    if (N == 0) return FX_OK;
    FX_CHECK_ARG(X && out && workspace, "fx_colsum: null pointer");
    hipStream_t s = fx_hip_stream(stream);
    const int64_t rpc = fx_ceil_div(M > 0 ? M : 1, FX_COLSUM_CHUNKS);
    const bool vec = (N % 4 == 0) && (ldx % 4 == 0) &&
                     ((reinterpret_cast<uintptr_t>(X) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
    if (vec)
        hipLaunchKernelGGL(k_colsum_stage1_v4, dim3((unsigned)fx_ceil_div(N, 256), FX_COLSUM_CHUNKS),
                           dim3(256), 0, s, X, ldx, M, N, rpc, workspace);
    else
        hipLaunchKernelGGL(k_colsum_stage1, dim3((unsigned)fx_ceil_div(N, 64), FX_COLSUM_CHUNKS),
                           dim3(256), 0, s, X, ldx, M, N, rpc, workspace);
    FX_CHECK_LAUNCH();
    return fx_rowsum<float, FX_ROWS_SLICES>(s, workspace, (int)FX_COLSUM_CHUNKS, N, fx_rowsum_out(out, N));
}

// ---------------------------------------------------------------------------------------------
// relu backward mask (only for a tower whose last layer is activated)
// ---------------------------------------------------------------------------------------------
// (the incoming gradient may be a column slice of a wider tensor — the backward of the torch.cat that
// joins the towers' outputs hands out strided views: read in place through its row stride instead of
// a .contiguous() copy first)
__global__ __launch_bounds__(256) void k_mask_mul(const float* dy, int64_t dy_ld, const float* y,
                                                  int64_t y_ld, float* out, uint32_t n, uint32_t cols) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t r = i / cols, c = i - r * cols;
        const float d = dy[(int64_t)r * dy_ld + c];
        out[i] = y[(int64_t)r * y_ld + c] > 0.f ? d : 0.f;
    }
}

extern "C" int fx_mask_mul(const float* dy, int64_t dy_ld, const float* y, int64_t y_ld, float* out,
                           int64_t rows, int64_t cols, fx_stream_t stream) {
    const int64_t n = rows * cols;
    if (n <= 0) return FX_OK;
    FX_CHECK_ARG(dy && y && out && dy_ld >= cols && y_ld >= cols, "fx_mask_mul: bad arguments");
    // (32-bit grid-stride counter: i += gridDim.x * 256 must not wrap)
    FX_CHECK_ARG(n < ((int64_t)1 << 31), "fx_mask_mul: more than 2^31 elements");
    int64_t blocks = fx_ceil_div(n, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_mask_mul, dim3((unsigned)blocks), dim3(256), 0, fx_hip_stream(stream), dy,
                       dy_ld, y, y_ld, out, (uint32_t)n, (uint32_t)cols);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------
// CrossNetV2 backward glue
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cross_bwd_prep(const float* dxn, int64_t dxn_ld,
                                                        const float* x0, const float* z, float* t,
                                                        float* dx0, uint32_t n, uint32_t cols,
                                                        int init, int add_dxn) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t r = i / cols;
        const float d = dxn[(int64_t)r * dxn_ld + (i - r * cols)];
        t[i] = d * x0[i];
        float term = d * z[i];
        if (add_dxn) term += d;
        dx0[i] = init ? term : dx0[i] + term;
    }
}

extern "C" int fx_cross_bwd_prep(const float* dxn, int64_t dxn_ld, const float* x0, const float* z,
                                 float* t, float* dx0, int64_t rows, int64_t cols, int32_t init,
                                 int32_t add_dxn, fx_stream_t stream) {
    const int64_t n = rows * cols;
    if (n <= 0) return FX_OK;
    FX_CHECK_ARG(dxn && x0 && z && t && dx0 && dxn_ld >= cols, "fx_cross_bwd_prep: bad arguments");
    FX_CHECK_ARG(n < ((int64_t)1 << 31), "fx_cross_bwd_prep: more than 2^31 elements");
    int64_t blocks = fx_ceil_div(n, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_cross_bwd_prep, dim3((unsigned)blocks), dim3(256), 0,
                       fx_hip_stream(stream), dxn, dxn_ld, x0, z, t, dx0, (uint32_t)n,
                       (uint32_t)cols, (int)init, (int)add_dxn);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------
// sigmoid + binary cross entropy (mean) + dloss/dlogit, one workgroup, fixed-order reduction
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_sigmoid_bce(const float* logit, const float* y,
                                                      int64_t B, float* prob, float* loss,
                                                      float* dlogit) {
    __shared__ float red[1024];
    float acc = 0.f;
    const float invB = 1.f / (float)B;
    for (int64_t i = threadIdx.x; i < B; i += 1024) {
        const float x = logit[i];
        const float p = 1.f / (1.f + expf(-x));  // torch.sigmoid
        if (prob) prob[i] = p;
        if (!y) continue;  // activation only
        const float t = y[i];
        // F.binary_cross_entropy clamps each log term at -100
        const float lp = fmaxf(logf(p), -100.f);
        const float lq = fmaxf(logf(1.f - p), -100.f);
        acc += -(t * lp + (1.f - t) * lq);
        if (dlogit) {
            // binary_cross_entropy_backward: (p - t) / max((1 - p) * p, 1e-12) * grad, then
            // sigmoid_backward: * p * (1 - p)
            const float dp = (p - t) / fmaxf((1.f - p) * p, 1e-12f) * invB;
            dlogit[i] = dp * ((1.f - p) * p);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && loss) *loss = red[0] * invB;
}

extern "C" int fx_sigmoid_bce(const float* logit, const float* y, int64_t B, float* prob,
                              float* loss, float* dlogit, fx_stream_t stream) {
    FX_CHECK_ARG(B > 0, "fx_sigmoid_bce: B must be positive");
    FX_CHECK_ARG(logit, "fx_sigmoid_bce: null logit");
    FX_CHECK_ARG(y || (!loss && !dlogit), "fx_sigmoid_bce: loss/dlogit need labels");
    hipLaunchKernelGGL(k_sigmoid_bce, dim3(1), dim3(1024), 0, fx_hip_stream(stream), logit, y, B,
                       prob, loss, dlogit);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------
// The training step's last mile in one pass over the top hidden layer (round 4): the Linear(K -> 1)
// head forward (+ the term added to the logit), sigmoid + BCE, and the head's backward — dlogit, the
// input gradient dz[m, :] = dlogit[m] w[:] (with the ReLU mask of the hidden layer: h IS the mask; from a
// column on when only the tail of h went through a ReLU — DCNv2's [cross | deep] head input) and
// the slabs of dW = sum_m dlogit[m] h[m, :], db = sum_m dlogit[m], loss = mean_m bce_m.  It replaces
// k_gemm_small_n_wide + k_sigmoid_bce + k_head_bwd_v4 (h streamed twice, three launch boundaries) by
// one launch; k_head_reduce then adds the G slabs in a fixed order (deterministic) instead of
// k_splitk_reduce_wide.  One wave per row, a lane holds the row's float4s k = 4 lane + 256 u (u < NU):
// the dot product is k_gemm_small_n_wide's fmaf chain + fx_wave_sum, so the logit is bit for bit the
// unfused forward's (evaluate / predict run that one); dlogit is k_sigmoid_bce's expression.
// ---------------------------------------------------------------------------------------------
struct HeadTrainArgs {
    const float* h;       // [M, K] hidden activations (row stride ldh)
    int64_t ldh;
    const float* w;       // [K]
    const float* bias;    // [1] or null
    const float* add;     // [M] (stride ldadd) or null: added to the logit after the bias
    int64_t ldadd;
    const float* y;       // [M] labels
    float* logit;         // [M]
    float* dlogit;        // [M]
    float* dz;            // [M, K] (row stride lddz) or null
    int64_t lddz;
    float* ws;            // [G, K] dW slabs | [G] db partials | [G] loss partials
    int64_t M, K;
    float root_scale;     // the root gradient of loss.backward() (1, or 1 / world when sharded)
    int32_t mask_from;    // < 0: no mask; else dz[m, k] = 0 where h[m, k] <= 0 for k >= mask_from (4 | mask_from)
};

template <int NU>
__global__ __launch_bounds__(256) void k_head_train(HeadTrainArgs a) {
    __shared__ float red[4][NU * 256];
    __shared__ float red2[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t G = gridDim.x;
    const float invB = 1.f / (float)a.M;
    float4 wv[NU], acc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int64_t k = (int64_t)lane * 4 + 256 * u;
        wv[u] = k < a.K ? *reinterpret_cast<const float4*>(a.w + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float b0 = a.bias ? a.bias[0] : 0.f;
    float dbs = 0.f, ls = 0.f;
    for (int64_t m = (int64_t)blockIdx.x * 4 + wave; m < a.M; m += G * 4) {
        const float* row = a.h + m * a.ldh;
        float4 x[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int64_t k = (int64_t)lane * 4 + 256 * u;
            x[u] = k < a.K ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float t = a.y[m];
        const float ad = a.add ? a.add[m * a.ldadd] : 0.f;
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if ((int64_t)lane * 4 + 256 * u < a.K) {      // (k_gemm_small_n_wide adds nothing past K either)
                s = fmaf(x[u].x, wv[u].x, s);
                s = fmaf(x[u].y, wv[u].y, s);
                s = fmaf(x[u].z, wv[u].z, s);
                s = fmaf(x[u].w, wv[u].w, s);
            }
        }
        float z = fx_wave_sum(s);
        if (a.bias) z += b0;
        if (a.add) z += ad;
        const float p = 1.f / (1.f + expf(-z));
        const float lp = fmaxf(logf(p), -100.f);
        const float lq = fmaxf(logf(1.f - p), -100.f);
        ls += -(t * lp + (1.f - t) * lq);
        const float dp = (p - t) / fmaxf((1.f - p) * p, 1e-12f) * invB;
        float d = dp * ((1.f - p) * p);
        if (a.root_scale != 1.f) d *= a.root_scale;
        dbs += d;
        if (lane == 0) {
            a.logit[m] = z;
            a.dlogit[m] = d;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int64_t k = (int64_t)lane * 4 + 256 * u;
            acc[u].x = fmaf(d, x[u].x, acc[u].x);
            acc[u].y = fmaf(d, x[u].y, acc[u].y);
            acc[u].z = fmaf(d, x[u].z, acc[u].z);
            acc[u].w = fmaf(d, x[u].w, acc[u].w);
            if (a.dz && k < a.K) {
                float4 o = make_float4(d * wv[u].x, d * wv[u].y, d * wv[u].z, d * wv[u].w);
                if (a.mask_from >= 0 && k >= a.mask_from) {
                    o.x = x[u].x > 0.f ? o.x : 0.f;
                    o.y = x[u].y > 0.f ? o.y : 0.f;
                    o.z = x[u].z > 0.f ? o.z : 0.f;
                    o.w = x[u].w > 0.f ? o.w : 0.f;
                }
                *reinterpret_cast<float4*>(a.dz + m * a.lddz + k) = o;
            }
        }
    }
    // the four waves' partial sums, added in wave order
#pragma unroll
    for (int u = 0; u < NU; ++u)
        *reinterpret_cast<float4*>(&red[wave][lane * 4 + 256 * u]) = acc[u];
    if (lane == 0) {
        red2[wave] = dbs;
        red2[4 + wave] = ls;
    }
    __syncthreads();
    for (int64_t k = threadIdx.x; k < a.K; k += 256)
        a.ws[(int64_t)blockIdx.x * a.K + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    if (threadIdx.x == 0) {
        a.ws[G * a.K + blockIdx.x] = ((red2[0] + red2[1]) + red2[2]) + red2[3];
        a.ws[G * a.K + G + blockIdx.x] = ((red2[4] + red2[5]) + red2[6]) + red2[7];
    }
}

// dW[k] = sum over the G slabs (8 elements x 32 slab lanes per workgroup, 8 loads in flight, fixed LDS
// tree); workgroup 0 also adds the G db / loss partials (G <= 256: one per thread, fixed tree).
// (not fx_rowsum: 32 slab lanes per column, the 1 / B scale and the db / loss sums ride in the same launch)
__global__ __launch_bounds__(256) void k_head_reduce(const float* ws, int64_t G, int64_t K, float invB,
                                                     float* dW, float* db, float* loss) {
    __shared__ float red[256];
    const int ii = threadIdx.x & 7, zi = threadIdx.x >> 3;
    const int64_t k = (int64_t)blockIdx.x * 8 + ii;
    float s = 0.f;
    if (k < K) {
        int64_t z = zi;
        for (; z + 7 * 32 < G; z += 8 * 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ws[(z + u * 32) * K + k];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; z < G; z += 32) s += ws[z * K + k];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 16; h > 0; h >>= 1) {
        if (zi < h) red[threadIdx.x] += red[threadIdx.x + h * 8];
        __syncthreads();
    }
    if (zi == 0 && k < K) dW[k] = red[ii];
    if (blockIdx.x == 0) {                       // block-uniform
        for (int which = 0; which < 2; ++which) {
            __syncthreads();
            red[threadIdx.x] = (int64_t)threadIdx.x < G ? ws[G * K + which * G + threadIdx.x] : 0.f;
            __syncthreads();
            for (int h = 128; h > 0; h >>= 1) {
                if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                if (which == 0) { if (db) db[0] = red[0]; }
                else if (loss) loss[0] = red[0] * invB;
            }
        }
    }
}

static int64_t fx_head_train_groups(int64_t M) {
    int64_t g = fx_ceil_div(M, 4);
    return g > 256 ? 256 : (g < 1 ? 1 : g);
}

extern "C" int64_t fx_head_train_workspace(int64_t M, int64_t K) {
    return fx_head_train_groups(M) * (K + 2);
}

extern "C" int fx_head_train(const float* h, int64_t ldh, const float* w, const float* bias,
                             const float* add, int64_t ldadd, const float* y, int64_t M, int64_t K,
                             int32_t mask_from, float root_scale, float* logit, float* dlogit, float* dz,
                             int64_t lddz, float* dW, float* db, float* loss, float* workspace,
                             fx_stream_t stream) {
    FX_CHECK_ARG(M > 0 && K > 0, "fx_head_train: M and K must be positive");
    FX_CHECK_ARG(h && w && y && logit && dlogit && dW && workspace, "fx_head_train: null argument");
    // (K <= 8: fx_gemm_f32 takes its one-thread-per-output kernel there — another summation order)
    FX_CHECK_ARG(K % 4 == 0 && K > 8 && K <= 2048, "fx_head_train: K must be a multiple of 4 in (8, 2048] (K=%lld)",
                 (long long)K);
    FX_CHECK_ARG(ldh % 4 == 0 && (reinterpret_cast<uintptr_t>(h) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(w) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                 "fx_head_train: h / w / workspace must be 16-byte aligned, ldh %% 4 == 0");
    FX_CHECK_ARG(!dz || (lddz % 4 == 0 && (reinterpret_cast<uintptr_t>(dz) & 15) == 0),
                 "fx_head_train: dz must be 16-byte aligned, lddz %% 4 == 0");
    HeadTrainArgs a;
    a.h = h; a.ldh = ldh; a.w = w; a.bias = bias; a.add = add; a.ldadd = ldadd; a.y = y;
    a.logit = logit; a.dlogit = dlogit; a.dz = dz; a.lddz = lddz; a.ws = workspace;
    FX_CHECK_ARG(mask_from < 0 || mask_from % 4 == 0, "fx_head_train: mask_from must be a multiple of 4");
    a.M = M; a.K = K; a.root_scale = root_scale; a.mask_from = mask_from;
    const int64_t G = fx_head_train_groups(M);
    hipStream_t s = fx_hip_stream(stream);
    const dim3 grid((unsigned)G), block(256);
    const int64_t nu = fx_ceil_div(K, 256);
    if (nu <= 1) hipLaunchKernelGGL(k_head_train<1>, grid, block, 0, s, a);
    else if (nu <= 2) hipLaunchKernelGGL(k_head_train<2>, grid, block, 0, s, a);
    else if (nu <= 4) hipLaunchKernelGGL(k_head_train<4>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_head_train<8>, grid, block, 0, s, a);
    FX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head_reduce, dim3((unsigned)fx_ceil_div(K, 8)), block, 0, s, workspace, G, K,
                       1.f / (float)M, dW, db, loss);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
