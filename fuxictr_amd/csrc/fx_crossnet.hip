// fx_crossnet.hip — DCN's rank-1 cross network (fuxictr/pytorch/layers/interactions/cross_net.py:24-92), the whole
// L-layer stack per launch:
//         x_{l+1} = x_l + ((s_l * x_0) + b_l),   s_l = w_l . x_l   (one scalar per row and layer)
//   fx_cross_net_fwd : ONE launch for all L layers.  A wave owns a row: x_0 and the running x_l stay in registers
//                      (CN_NREG floats per lane each), the dot is a lane-local fp64 fma chain + a wave sum, the update
//                      keeps the reference's order.  Reads x_0 once, writes x_L once, optionally stashes s [rows, L].
//   fx_cross_net_bwd : TWO launches.  With a_l = 1 + sum_{k<l} s_k and B_l = sum_{k<l} b_k the stack is
//                      x_l = a_l x_0 + B_l, so with the per-row dots d = dout . x_0 and q_k = w_k . x_0:
//                          t_l = g_{l+1} . x_0 = d + sum_{k>l} t_k q_k          (scalar recurrence, l = L-1 .. 0)
//                          dx0 = a_L dout + sum_k (t_k a_k) w_k
//                          dw_l = sum_rows (t_l a_l) x_0 + B_l sum_rows t_l
//                          db_l = sum_rows dout + sum_{k>l} (sum_rows t_k) w_k
//                      k_cross_net_bwd, the row pass: a wave per row forms the dots chunk by chunk, reads dout again
//                      (out of the cache) for dx0 and leaves u_l = t_l a_l and t_l of its row in LDS; then the
//                      workgroup's threads, now one per chunk of PV columns, add u_l x_0 and dout of the tile's rows
//                      (a second read, out of L2) to column sums that they carry in registers over all tiles of the
//                      workgroup: one row of `partial` per workgroup.  k_cross_net_reduce sums the rows of `partial`
//                      in a fixed order and applies the B_l and w_k terms.  x_l is never read from memory and never
//                      formed.
// fp32 in memory.  Every sum over the columns of a row or over the rows (the dots, the scalar recurrence, dx0's L + 1
// terms, the column sums and their reduction) is accumulated in fp64 and rounded to fp32 once, when it is stored or
// enters the element-wise update: a sum of few, cancelling terms is as exact as its fp32 result can be.  These
// kernels stream; the fp64 fmas (half the fp32 rate) stay far below the time of the memory traffic.
// Every matrix has its own row stride (floats).  The aligned arm (16-byte accesses in the forward, 8-byte in the
// backward) when cols is a multiple of 4 and every base pointer and row stride is 16-byte aligned, a scalar arm
// otherwise.  No atomics; every sum has a fixed order: two launches on the same inputs give the same bits.
//
// Limits (fx_cross_net_limits): cols <= CN_MAX_COLS = 64 lanes * CN_NREG = 2048 (the production widths 624 and 1248
// are inside): the forward holds 2 * CN_NREG floats of x_0 and x_l per lane, the backward's column phase CN_MAX_L + 1
// sums per column of a thread.  L <= CN_MAX_L = 8: the backward unrolls over the layers (t_l, u_l, q_l in registers).
// A workgroup is CN_ROWS = 16 waves = 16 rows of a tile, so 128 VGPRs are the budget; the grid is capped at
// CN_MAX_WG = 256 workgroups (one per CU, 4 waves per SIMD) which stride over the row tiles with an int64 row index.
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage at these limits:
//     kernel                      VGPRs  SGPRs  scratch [bytes/lane]  LDS [bytes]  occupancy [waves/SIMD]
//     k_cross_net_fwd<4, 8>         108     58                     0            0                       4
//     k_cross_net_fwd<1, 32>        116    106                     0            0                       4
//     k_cross_net_bwd<2, 2, 1>      116    106                     0         2048                       4
//     k_cross_net_bwd<1, 1, 2>      119    106                     0         2048                       4
//     k_cross_net_reduce             34     34                     0         2304                       8
// The backward's aligned arm reads and writes 8 bytes per lane, not 16: with 16 the loads of all CN_MAX_L layers of a
// chunk, live next to the fp64 column sums, went past the 128 VGPRs (12 bytes of scratch per lane).  For the same
// reason the chunk loops of its row pass run one chunk per iteration.
#include "fx_common.h"

#define CN_NREG 32                // floats of a row per lane
#define CN_MAX_COLS (64 * CN_NREG)
#define CN_MAX_L 8
#define CN_ROWS 16                // rows of a tile: the waves of a workgroup
#define CN_THREADS (64 * CN_ROWS)
#define CN_MAX_WG 256             // one workgroup per CU
#define CN_RED_COLS 64            // k_cross_net_reduce: columns per workgroup, times CN_RED_PARTS groups of partials
#define CN_RED_PARTS 4

struct CnArgs {
    const float* x0; int64_t ldx0;
    const float* w;                     // [L, cols] packed
    const float* b;                     // [L, cols] packed
    float* out; int64_t ldout;          // forward
    float* s;                           // [rows, L] packed; forward: written (null: not wanted), backward: read
    const float* dout; int64_t lddout;  // backward
    float* dx0; int64_t lddx0;
    float* partial; int64_t pstride;    // one row per workgroup: L column sums of u_l x_0 | of dout | L sums of t_l
    float* dw; float* db;               // [L, cols] packed
    int64_t rows;
    int cols, L, init, G;
};

// grid (row tiles, capped), block (64, CN_ROWS).  NCH * VEC = CN_NREG: lane holds the chunks lane + 64 j of its row
template <int VEC, int NCH>
__global__ __launch_bounds__(CN_THREADS) void k_cross_net_fwd(CnArgs p) {
    const int lane = threadIdx.x;
    const int nch = p.cols / VEC;
    for (int64_t r = (int64_t)blockIdx.x * CN_ROWS + threadIdx.y; r < p.rows; r += (int64_t)gridDim.x * CN_ROWS) {
        float x0[NCH][VEC], x[NCH][VEC];
        const float* src = p.x0 + r * p.ldx0;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int q = lane + 64 * j;
            if (q < nch) {
                fx_load<VEC>(src + (int64_t)q * VEC, x0[j]);
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) x0[j][k] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) x[j][k] = x0[j][k];
        }
        for (int l = 0; l < p.L; ++l) {
            const float* w = p.w + (int64_t)l * p.cols;
            const float* b = p.b + (int64_t)l * p.cols;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int q = lane + 64 * j;
                if (q < nch) {
                    float wv[VEC];
                    fx_load<VEC>(w + (int64_t)q * VEC, wv);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc = fma((double)wv[k], (double)x[j][k], acc);
                }
            }
            const float s = (float)fx_wave_sum(acc);
            if (p.s != nullptr && lane == 0) p.s[r * p.L + l] = s;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int q = lane + 64 * j;
                if (q < nch) {
                    float bv[VEC];
                    fx_load<VEC>(b + (int64_t)q * VEC, bv);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) x[j][k] = x[j][k] + ((s * x0[j][k]) + bv[k]);
                }
            }
        }
        float* dst = p.out + r * p.ldout;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int q = lane + 64 * j;
            if (q < nch) fx_store<VEC>(dst + (int64_t)q * VEC, x[j]);
        }
    }
}

// The row pass of the backward.  grid (G <= CN_MAX_WG), block (64, CN_ROWS).  VEC: floats per access of the row
// phase.  PV, KCH: the column phase, thread tid owns the chunks tid + CN_THREADS m, m < KCH, of PV columns each:
// KCH * CN_THREADS * PV >= CN_MAX_COLS (PV = 2 on the 16-byte arm: every thread has a chunk at the widest rows).
template <int VEC, int PV, int KCH>
__global__ __launch_bounds__(CN_THREADS) void k_cross_net_bwd(CnArgs p) {
    __shared__ double u_sh[CN_ROWS][CN_MAX_L];      // u_l = t_l a_l of the tile's rows (0 behind the last row)
    __shared__ double t_sh[CN_ROWS][CN_MAX_L];      // t_l
    const int lane = threadIdx.x, wy = threadIdx.y;
    const int tid = wy * 64 + lane;
    const int nch = p.cols / VEC, npv = p.cols / PV;
    const int L = p.L;
    double accP[CN_MAX_L][KCH][PV], accD[KCH][PV];
    double accT = 0.0;                               // thread tid < L: sum_rows t_tid
#pragma unroll
    for (int m = 0; m < KCH; ++m) {
#pragma unroll
        for (int k = 0; k < PV; ++k) {
            accD[m][k] = 0.0;
#pragma unroll
            for (int l = 0; l < CN_MAX_L; ++l) accP[l][m][k] = 0.0;
        }
    }
    // (r0 is the same in every thread of the workgroup: all of them reach both barriers of every tile)
    for (int64_t r0 = (int64_t)blockIdx.x * CN_ROWS; r0 < p.rows; r0 += (int64_t)gridDim.x * CN_ROWS) {
        const int64_t r = r0 + wy;
        double u[CN_MAX_L], t[CN_MAX_L];
#pragma unroll
        for (int l = 0; l < CN_MAX_L; ++l) u[l] = t[l] = 0.0;
        if (r < p.rows) {
            double d = 0.0, qd[CN_MAX_L];
#pragma unroll
            for (int l = 0; l < CN_MAX_L; ++l) qd[l] = 0.0;
            const float* gsrc = p.dout + r * p.lddout;
            const float* xsrc = p.x0 + r * p.ldx0;
#pragma unroll 1
            for (int q = lane; q < nch; q += 64) {
                float gv[VEC], xv[VEC];
                fx_load<VEC>(gsrc + (int64_t)q * VEC, gv);
                fx_load<VEC>(xsrc + (int64_t)q * VEC, xv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) d = fma((double)gv[k], (double)xv[k], d);
#pragma unroll
                for (int l = 0; l < CN_MAX_L; ++l) {
                    if (l < L) {
                        float wv[VEC];
                        fx_load<VEC>(p.w + (int64_t)l * p.cols + (int64_t)q * VEC, wv);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) qd[l] = fma((double)wv[k], (double)xv[k], qd[l]);
                    }
                }
            }
            d = fx_wave_sum(d);
            double a[CN_MAX_L + 1];
            a[0] = 1.0;
#pragma unroll
            for (int l = 0; l < CN_MAX_L; ++l) {
                if (l < L) {
                    qd[l] = fx_wave_sum(qd[l]);
                    a[l + 1] = a[l] + (double)p.s[r * L + l];
                } else {
                    a[l + 1] = a[l];
                }
            }
            // t_l = d + sum_{k>l} t_k q_k, from the last layer down
#pragma unroll
            for (int l = CN_MAX_L - 1; l >= 0; --l) {
                if (l < L) {
                    double tl = d;
#pragma unroll
                    for (int k = l + 1; k < CN_MAX_L; ++k)
                        if (k < L) tl = fma(t[k], qd[k], tl);
                    t[l] = tl;
                    u[l] = tl * a[l];
                }
            }
            const double aL = a[CN_MAX_L];           // = a_L: a stops growing at L
            float* dst = p.dx0 + r * p.lddx0;
            // dout a second time, out of the cache: no row is held in registers
#pragma unroll 1
            for (int q = lane; q < nch; q += 64) {
                float gv[VEC], v[VEC];
                double acc[VEC];
                fx_load<VEC>(gsrc + (int64_t)q * VEC, gv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = aL * (double)gv[k];
#pragma unroll
                for (int l = 0; l < CN_MAX_L; ++l) {
                    if (l < L) {
                        float wv[VEC];
                        fx_load<VEC>(p.w + (int64_t)l * p.cols + (int64_t)q * VEC, wv);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[k] = fma(u[l], (double)wv[k], acc[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[k] = (float)acc[k];
                if (!p.init) {
                    float old[VEC];
                    fx_load<VEC>(dst + (int64_t)q * VEC, old);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) v[k] = old[k] + v[k];
                }
                fx_store<VEC>(dst + (int64_t)q * VEC, v);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int l = 0; l < CN_MAX_L; ++l) {
                u_sh[wy][l] = u[l];
                t_sh[wy][l] = t[l];
            }
        }
        __syncthreads();
        // the column phase: this thread's chunks of columns over the rows of the tile, in row order
        const int nr = p.rows - r0 < CN_ROWS ? (int)(p.rows - r0) : CN_ROWS;
#pragma unroll
        for (int m = 0; m < KCH; ++m) {
            const int q = tid + CN_THREADS * m;
            if (q < npv) {
                for (int rr = 0; rr < nr; ++rr) {
                    float xv[PV], gv[PV];
                    fx_load<PV>(p.x0 + (r0 + rr) * p.ldx0 + (int64_t)q * PV, xv);
                    fx_load<PV>(p.dout + (r0 + rr) * p.lddout + (int64_t)q * PV, gv);
#pragma unroll
                    for (int k = 0; k < PV; ++k) accD[m][k] += (double)gv[k];
#pragma unroll
                    for (int l = 0; l < CN_MAX_L; ++l) {
                        if (l < L) {
                            const double ul = u_sh[rr][l];
#pragma unroll
                            for (int k = 0; k < PV; ++k) accP[l][m][k] = fma(ul, (double)xv[k], accP[l][m][k]);
                        }
                    }
                }
            }
        }
        if (tid < L) {
            for (int rr = 0; rr < nr; ++rr) accT += t_sh[rr][tid];
        }
        __syncthreads();                             // u_sh / t_sh are free for the next tile
    }
    float* prow = p.partial + (int64_t)blockIdx.x * p.pstride;
#pragma unroll
    for (int m = 0; m < KCH; ++m) {
        const int q = tid + CN_THREADS * m;
        if (q < npv) {
            float v[PV];
#pragma unroll
            for (int l = 0; l < CN_MAX_L; ++l) {
                if (l < L) {
#pragma unroll
                    for (int k = 0; k < PV; ++k) v[k] = (float)accP[l][m][k];
                    fx_store<PV>(prow + (int64_t)l * p.cols + (int64_t)q * PV, v);
                }
            }
#pragma unroll
            for (int k = 0; k < PV; ++k) v[k] = (float)accD[m][k];
            fx_store<PV>(prow + (int64_t)L * p.cols + (int64_t)q * PV, v);
        }
    }
    if (tid < L) prow[(int64_t)(L + 1) * p.cols + tid] = (float)accT;
}

// The G rows of `partial` -> dw, db.  grid (ceil(cols / CN_RED_COLS), L + 1), block (CN_RED_COLS, CN_RED_PARTS):
// blockIdx.y = j < L sums the column sums of u_j x_0 and writes dw_j; blockIdx.y = L sums those of dout and writes
// every db_l.  Group y of the block adds the rows y, y + CN_RED_PARTS, ... in that order; the groups and the G sums
// of t_k meet in a fixed order.  (Not fx_rowsum.h's row sum: the sums are combined with b and T_k before they leave.)
__global__ __launch_bounds__(CN_RED_COLS * CN_RED_PARTS) void k_cross_net_reduce(CnArgs p) {
    __shared__ double red[CN_RED_PARTS][CN_RED_COLS];
    __shared__ double tred[CN_MAX_L][CN_RED_PARTS];
    const int lane = threadIdx.x, part = threadIdx.y;
    const int tid = part * CN_RED_COLS + lane;
    const int L = p.L, cols = p.cols, j = blockIdx.y;
    const int c = blockIdx.x * CN_RED_COLS + lane;
    double sum = 0.0;
    if (c < cols) {
        for (int g = part; g < p.G; g += CN_RED_PARTS)
            sum += (double)p.partial[(int64_t)g * p.pstride + (int64_t)j * cols + c];
    }
    red[part][lane] = sum;
    // T_k = sum over the workgroups of their sums of t_k: thread tid takes the rows tid, tid + 256, ...
    for (int k = 0; k < L; ++k) {
        double tk = 0.0;
        for (int g = tid; g < p.G; g += CN_RED_COLS * CN_RED_PARTS)
            tk += (double)p.partial[(int64_t)g * p.pstride + (int64_t)(L + 1) * cols + k];
        tk = fx_wave_sum(tk);                        // (CN_RED_COLS = 64: a group is a wave)
        if (lane == 0) tred[k][part] = tk;
    }
    __syncthreads();
    if (part != 0 || c >= cols) return;
    const double total = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    double T[CN_MAX_L];
#pragma unroll
    for (int k = 0; k < CN_MAX_L; ++k) T[k] = k < L ? (tred[k][0] + tred[k][1]) + (tred[k][2] + tred[k][3]) : 0.0;
    if (j < L) {
        double B = 0.0;                              // B_j = b_0 + ... + b_{j-1}
        double Tj = 0.0;
#pragma unroll
        for (int k = 0; k < CN_MAX_L; ++k) {
            if (k < j) B += (double)p.b[(int64_t)k * cols + c];
            if (k == j) Tj = T[k];
        }
        p.dw[(int64_t)j * cols + c] = (float)fma(B, Tj, total);
    } else {
        // db_l = sum_rows dout + sum_{k>l} T_k w_k, built from the last layer down
        double tail = 0.0;
#pragma unroll
        for (int l = CN_MAX_L - 1; l >= 0; --l) {
            if (l < L) {
                p.db[(int64_t)l * cols + c] = (float)(total + tail);
                tail = fma(T[l], (double)p.w[(int64_t)l * cols + c], tail);
            }
        }
    }
}

static_assert(CN_RED_COLS == 64 && CN_RED_PARTS == 4, "k_cross_net_reduce: a group is a wave, four groups");
static_assert(CN_MAX_L <= CN_THREADS && CN_MAX_L <= 64, "one thread per layer sums t_l");

// a [rows, cols] matrix with row stride ld
static int cn_check_mat(const char* who, const char* name, const void* ptr, int64_t ld, int64_t cols) {
    FX_CHECK_ARG(ptr, "%s: null %s", who, name);
    FX_CHECK_ARG(ld >= cols, "%s: %s row stride %lld < %lld", who, name, (long long)ld, (long long)cols);
    return FX_OK;
}

static int cn_check_shape(const char* who, int64_t rows, int32_t cols, int32_t L) {
    FX_CHECK_ARG(cols >= 1 && cols <= CN_MAX_COLS, "%s: cols=%d, limit 1 <= cols <= %d", who, cols, CN_MAX_COLS);
    FX_CHECK_ARG(L >= 1 && L <= CN_MAX_L, "%s: L=%d, limit 1 <= L <= %d", who, L, CN_MAX_L);
    FX_CHECK_ARG(rows >= 0, "%s: rows=%lld", who, (long long)rows);
    return FX_OK;
}

static unsigned cn_grid(int64_t rows) {
    const int64_t tiles = fx_ceil_div(rows, CN_ROWS);
    return (unsigned)(tiles < CN_MAX_WG ? tiles : CN_MAX_WG);
}

// floats of one workgroup's row of `partial`: (L + 1) column sums and L scalars, a multiple of 4
static int64_t cn_pstride(int32_t cols, int32_t L) { return ((int64_t)(L + 1) * cols + L + 3) / 4 * 4; }

extern "C" void fx_cross_net_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = CN_MAX_COLS;
    limits[1] = CN_MAX_L;
    limits[2] = CN_ROWS;
    limits[3] = CN_MAX_WG;
}

extern "C" int64_t fx_cross_net_workspace_floats(int64_t rows, int32_t cols, int32_t L) {
    if (cols < 1 || L < 1) return 0;
    return (int64_t)cn_grid(rows > 0 ? rows : 1) * cn_pstride(cols, L);
}

extern "C" int fx_cross_net_fwd(const float* x0, int64_t ldx0, const float* w, const float* b, float* out,
                                int64_t ldout, float* s, int64_t rows, int32_t cols, int32_t L,
                                fx_stream_t stream) {
    const char* who = "fx_cross_net_fwd";
    if (int st = cn_check_shape(who, rows, cols, L)) return st;
    if (int st = cn_check_mat(who, "x0", x0, ldx0, cols)) return st;
    if (int st = cn_check_mat(who, "out", out, ldout, cols)) return st;
    FX_CHECK_ARG(w && b, "%s: null w / b", who);
    if (rows == 0) return FX_OK;
    CnArgs p;
    memset(&p, 0, sizeof(p));
    p.x0 = x0; p.ldx0 = ldx0; p.w = w; p.b = b; p.out = out; p.ldout = ldout; p.s = s;
    p.rows = rows; p.cols = cols; p.L = L;
    const bool vec4 = cols % 4 == 0 && fx_vec_ok(x0, ldx0) && fx_vec_ok(out, ldout) && fx_vec_ok(w, 0) &&
                      fx_vec_ok(b, 0);
    const dim3 grid(cn_grid(rows)), block(64, CN_ROWS);
    hipStream_t st = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL((k_cross_net_fwd<4, CN_NREG / 4>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((k_cross_net_fwd<1, CN_NREG>), grid, block, 0, st, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_cross_net_bwd(const float* dout, int64_t lddout, const float* x0, int64_t ldx0, const float* w,
                                const float* b, const float* s, float* dx0, int64_t lddx0, float* dw, float* db,
                                float* workspace, int64_t rows, int32_t cols, int32_t L, int32_t init,
                                fx_stream_t stream) {
    const char* who = "fx_cross_net_bwd";
    if (int st = cn_check_shape(who, rows, cols, L)) return st;
    if (int st = cn_check_mat(who, "dout", dout, lddout, cols)) return st;
    if (int st = cn_check_mat(who, "x0", x0, ldx0, cols)) return st;
    if (int st = cn_check_mat(who, "dx0", dx0, lddx0, cols)) return st;
    FX_CHECK_ARG(w && b && s, "%s: null w / b / s", who);
    FX_CHECK_ARG(dw && db && workspace, "%s: null dw / db / workspace", who);
    hipStream_t st = fx_hip_stream(stream);
    if (rows == 0) {
        FX_CHECK_HIP(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)L * cols, st));
        FX_CHECK_HIP(hipMemsetAsync(db, 0, sizeof(float) * (size_t)L * cols, st));
        return FX_OK;
    }
    CnArgs p;
    memset(&p, 0, sizeof(p));
    p.dout = dout; p.lddout = lddout; p.x0 = x0; p.ldx0 = ldx0; p.w = w; p.b = b; p.s = const_cast<float*>(s);
    p.dx0 = dx0; p.lddx0 = lddx0; p.dw = dw; p.db = db; p.partial = workspace; p.pstride = cn_pstride(cols, L);
    p.rows = rows; p.cols = cols; p.L = L; p.init = init ? 1 : 0;
    p.G = (int)cn_grid(rows);
    const bool vec4 = cols % 4 == 0 && fx_vec_ok(dout, lddout) && fx_vec_ok(x0, ldx0) && fx_vec_ok(dx0, lddx0) &&
                      fx_vec_ok(w, 0) && fx_vec_ok(workspace, 0);
    const dim3 grid(p.G), block(64, CN_ROWS);
    if (vec4) hipLaunchKernelGGL((k_cross_net_bwd<2, 2, 1>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((k_cross_net_bwd<1, 1, 2>), grid, block, 0, st, p);
    FX_CHECK_LAUNCH();
    const dim3 rgrid((unsigned)fx_ceil_div(cols, CN_RED_COLS), (unsigned)(L + 1)), rblock(CN_RED_COLS, CN_RED_PARTS);
    hipLaunchKernelGGL(k_cross_net_reduce, rgrid, rblock, 0, st, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}
