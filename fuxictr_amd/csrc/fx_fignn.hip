// fx_fignn.hip — FiGNN's gated graph propagation over the fields of one sample (model_zoo/FiGNN/src/FiGNN.py) and its
// attentional prediction head, fused over the [B, F, D] gather record.  Per sample, x = feature_emb[b] of shape [F, D]:
//   graph (FiGNN.py:128-145), built once from x:
//       alpha[i][j] = leaky_relu_0.01(w_src . x_i + w_dst . x_j),  W_attn.weight [1, 2 D] = w_src | w_dst
//       g[i] = softmax_j(alpha[i]) with the diagonal at -inf.  2 F dot products; the [F^2, 2 D] concat is never formed.
//   layer l of L (FiGNN.py:158-171, 200-203), from h = x:
//       o_f = W_out[l][f] h_f;  aggr_i = sum_j g[i][j] o_j;  a_i = W_in[l][i] aggr_i + bias_p[l]
//       FG_GRU: h = GRUCell(a, h) (chunks r, z, n; h' = (1 - z) n + z h; one weight set for all fields and layers),
//       otherwise h = a + h;  FG_RES: h += x;  FG_REUSE: every layer reads layer 0's W_in / W_out / bias_p.
//   head (FiGNN.py:228-231): logit = sum_f sigmoid(Z[f]) (mlp1 . h_f),  Z = mlp2 . flatten(h) from the project's GEMM.
// fp32, no atomics, every sum in a fixed order.
//
//   k_fignn_fwd<VEC>: a workgroup owns a tile of T samples (fx_fignn_tile_rows: the largest power of two up to 16 that
//       the 160 KB of LDS hold) for the graph and all layers.  The planes x, h and two scratch planes (o / a and
//       aggr / h') sit in LDS TRANSPOSED as in fx_pairfm.hip, plane[c][T] (c = f * D + d), with g [F * F][T] and the
//       two score vectors [2 F][T] beside them.  A thread's item is (column c, sample t), t fastest: the T lanes of
//       one column read consecutive LDS words and the SAME element of W_out[l] / W_in[l], which streams past the tile
//       from global memory (L2) once per tile and layer and is never copied to LDS.  The GRU's four tensors are kept in
//       LDS (row stride D + 4, or D | 1 for VEC = 1) whenever that costs no tile rows, and are read from global
//       memory otherwise.  Training also writes the inputs of layers 1 .. L - 1 (`hs`); g is recomputed.
//   k_fignn_bwd<VEC>: one launch, from d_h_out back through the layers and the graph.  The same tile plan with nine
//       planes and g, dg (so a smaller T).  Per layer it recomputes o, aggr, a and the gates from the layer's input,
//       then walks the chain backwards; dX (layers + residual + graph) leaves with plain stores.  Every weight
//       gradient is a sum over the batch: a workgroup owns row blockIdx.x of `partial` and adds its tiles' sums to
//       it in tile order (the first touch stores), one owner thread per element; fx_rowsum<double, SLICES> adds the
//       rows.  One workgroup: straight into grads, no reduce.
//   k_fignn_head_fwd / _bwd: a wave per sample, lane d; score_f by the butterfly.  d mlp1 is summed per workgroup in
//       wave order, then over the workgroups by fx_rowsum.
//   VEC = 4 (16-byte accesses of X, dX, hs and the weight rows) when D % 4 == 0 and every base pointer and row stride
//   is 16-byte aligned; VEC = 1 otherwise (the reference's default D = 10).
#include "fx_common.h"
#include "fx_rowsum.h"

#define FG_GRU 1
#define FG_RES 2
#define FG_REUSE 4
#define FG_NT 512                  // threads of a tile workgroup
#define FG_MIN_F 2
#define FG_MAX_F 64
#define FG_MAX_FD 2048
#define FG_MAX_D 64
#define FG_MAX_LAYERS 8
#define FG_MAX_WG 256              // workgroups = rows of `partial`
#define FG_MAX_TILE 16
#define FG_LDS_MAX (160 * 1024)
#define FG_HEAD_NT 256
#define FG_HEAD_WG 256

struct FgArgs {
    const float* X; int64_t ldx;        // [B, F*D]
    const float* W;                     // [LW][W_in F*D*D | W_out F*D*D | bias_p D], LW = 1 (FG_REUSE) or L
    const float *w_ih, *w_hh, *b_ih, *b_hh;     // [3D, D] x 2, [3D] x 2 (FG_GRU)
    const float* w_attn;                // [2D]
    float* h_out;                       // [B, F*D]                 forward
    float* hs;                          // [L-1, B, F*D] or null    forward: written; backward: read
    const float* dH;                    // [B, F*D]                 backward
    float* dX; int64_t lddx;            // [B, F*D]
    float* partial; int64_t ldp;        // [workgroups, ldp]
    int64_t B;
    int F, D, L, flags;
    int T, tsh;                         // tile rows, log2
    int glds, ldg;                      // floats of GRU weights in LDS (0: global memory); their row stride
};

struct FgPlan { int T, tsh, glds, ldg; };

static inline int64_t fg_per_sample(int F, int D, bool bwd) {
    const int64_t FD = (int64_t)F * D;
    return bwd ? 9 * FD + 2 * F * F + 2 * F : 4 * FD + F * F + 2 * F;
}
static inline int fg_fit(int64_t room, int64_t per) {
    int T = FG_MAX_TILE;
    while (T > 1 && T * per > room) T >>= 1;
    return T;
}
static inline int fg_ldg_lds(int D) { return D % 4 == 0 ? D + 4 : (D | 1); }

static FgPlan fg_plan(int F, int D, int flags, bool bwd) {
    const int64_t room = FG_LDS_MAX / 4, per = fg_per_sample(F, D, bwd);
    FgPlan p;
    p.T = fg_fit(room, per);
    p.glds = 0;
    p.ldg = D;
    if (flags & FG_GRU) {
        const int ldg = fg_ldg_lds(D);
        const int64_t g = (6 * (int64_t)D * ldg + 6 * D + 3) / 4 * 4;
        if (g < room && fg_fit(room - g, per) == p.T && p.T * per <= room - g) {
            p.glds = (int)g;
            p.ldg = ldg;
        }
    }
    p.tsh = 0;
    while ((1 << p.tsh) < p.T) ++p.tsh;
    return p;
}

static inline int64_t fg_layer_floats(int F, int D) { return 2 * (int64_t)F * D * D + D; }
static inline int64_t fg_grad_floats(int F, int D, int L, int flags) {
    return ((flags & FG_REUSE) ? 1 : L) * fg_layer_floats(F, D) + ((flags & FG_GRU) ? 6 * (int64_t)D * D + 6 * D : 0) +
           2 * D;
}

struct FgGru {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    int ld;
};

__device__ __forceinline__ float fg_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// the GRU's tensors: copied to `gl` (row stride a.ldg) when the plan keeps them in LDS; a barrier follows at the caller
__device__ __forceinline__ FgGru fg_stage_gru(const FgArgs& a, float* gl) {
    FgGru w = {a.w_ih, a.w_hh, a.b_ih, a.b_hh, a.D};
    if (a.glds > 0) {
        const int D = a.D, ld = a.ldg, n = 3 * D * D;
        float* wi = gl;
        float* wh = gl + 3 * D * ld;
        float* bi = wh + 3 * D * ld;
        float* bh = bi + 3 * D;
        for (int e = threadIdx.x; e < n; e += FG_NT) {
            const int r = e / D, d = e - r * D;
            wi[r * ld + d] = a.w_ih[e];
            wh[r * ld + d] = a.w_hh[e];
        }
        for (int e = threadIdx.x; e < 3 * D; e += FG_NT) {
            bi[e] = a.b_ih[e];
            bh[e] = a.b_hh[e];
        }
        w.w_ih = wi; w.w_hh = wh; w.b_ih = bi; w.b_hh = bh; w.ld = ld;
    }
    return w;
}

// T samples of src ([B, ld]) from row b0 -> plane P (and P2), transposed; lanes run over the samples first.  Rows
// past `rows`: zeros.
template <int VEC>
__device__ __forceinline__ void fg_load_tile(float* P, float* P2, const float* src, int64_t ld, int64_t b0, int rows,
                                             int FD, int T, int tsh) {
    for (int idx = threadIdx.x; idx < ((FD / VEC) << tsh); idx += FG_NT) {
        const int t = idx & (T - 1), c = (idx >> tsh) * VEC;
        float v[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = 0.f;
        if (t < rows) fx_load<VEC>(src + (b0 + t) * ld + c, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            P[(c + k) * T + t] = v[k];
            if (P2) P2[(c + k) * T + t] = v[k];
        }
    }
}

template <int VEC>
__device__ __forceinline__ void fg_store_tile(const float* P, float* dst, int64_t ld, int64_t b0, int rows, int FD,
                                              int T, int tsh) {
    for (int idx = threadIdx.x; idx < ((FD / VEC) << tsh); idx += FG_NT) {
        const int t = idx & (T - 1), c = (idx >> tsh) * VEC;
        if (t >= rows) continue;
        float v[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = P[(c + k) * T + t];
        fx_store<VEC>(dst + (b0 + t) * ld + c, v);
    }
}

// acc + sum_d w[d] col[d * T]: a contiguous weight row against one sample's column of a plane
template <int VEC>
__device__ __forceinline__ float fg_dot_row(const float* w, const float* col, int D, int T, float acc) {
    for (int d = 0; d < D; d += VEC) {
        float m[VEC];
        fx_load<VEC>(w + d, m);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc = fmaf(m[k], col[(d + k) * T], acc);
    }
    return acc;
}

// sum_e w[e * D] col[e * T]: a weight COLUMN (the transposed product of the backward)
__device__ __forceinline__ float fg_dot_col(const float* w, const float* col, int D, int T) {
    float acc = 0.f;
    for (int e = 0; e < D; ++e) acc = fmaf(w[e * D], col[e * T], acc);
    return acc;
}

// the two score vectors sd [2 F][T] and g [F * F][T] (diagonal 0) of the tile in X; ends with a barrier
__device__ __forceinline__ void fg_graph(const float* X, const float* w_attn, float* sd, float* G, int F, int D, int T,
                                         int tsh) {
    for (int idx = threadIdx.x; idx < ((2 * F) << tsh); idx += FG_NT) {
        const int t = idx & (T - 1), r = idx >> tsh;
        const int i = r < F ? r : r - F;
        const float* w = w_attn + (r < F ? 0 : D);
        const float* col = X + i * D * T + t;
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(w[d], col[d * T], s);
        sd[r * T + t] = s;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < (F << tsh); idx += FG_NT) {
        const int t = idx & (T - 1), i = idx >> tsh;
        const float si = sd[i * T + t];
        float* g = G + i * F * T + t;
        float m = -INFINITY;
        for (int j = 0; j < F; ++j) {
            if (j == i) continue;
            float al = si + sd[(F + j) * T + t];
            al = al > 0.f ? al : 0.01f * al;
            g[j * T] = al;
            m = fmaxf(m, al);
        }
        float sum = 0.f;
        for (int j = 0; j < F; ++j) {
            if (j == i) continue;
            const float e = expf(g[j * T] - m);
            g[j * T] = e;
            sum += e;
        }
        for (int j = 0; j < F; ++j) g[j * T] = j == i ? 0.f : g[j * T] / sum;
    }
    __syncthreads();
}

// the six gate pre-activations of element e of one field: gi[q] = b_ih[q D + e] + w_ih[q D + e] . a, gh likewise on h
template <int VEC>
__device__ __forceinline__ void fg_gates(const FgGru& w, const float* acol, const float* hcol, int e, int D, int T,
                                         float (&gi)[3], float (&gh)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        gi[q] = w.b_ih[q * D + e];
        gh[q] = w.b_hh[q * D + e];
    }
    for (int d = 0; d < D; d += VEC) {
        float av[VEC], hv[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            av[k] = acol[(d + k) * T];
            hv[k] = hcol[(d + k) * T];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float mi[VEC], mh[VEC];
            fx_load<VEC>(w.w_ih + (q * D + e) * w.ld + d, mi);
            fx_load<VEC>(w.w_hh + (q * D + e) * w.ld + d, mh);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                gi[q] = fmaf(mi[k], av[k], gi[q]);
                gh[q] = fmaf(mh[k], hv[k], gh[q]);
            }
        }
    }
}

// o = W_out h, aggr = g o, a = W_in aggr + bias_p of one layer: S1 <- o, S2 <- aggr, S1 <- a; ends with a barrier
template <int VEC>
__device__ __forceinline__ void fg_message(const float* Wl, const float* h, const float* G, float* S1, float* S2, int F,
                                           int D, int T, int tsh) {
    const int FD = F * D, NI = FD << tsh;
    const float* W_in = Wl;
    const float* W_out = Wl + (int64_t)FD * D;
    const float* bp = W_out + (int64_t)FD * D;
    for (int idx = threadIdx.x; idx < NI; idx += FG_NT) {
        const int t = idx & (T - 1), c = idx >> tsh, f = c / D;
        S1[idx] = fg_dot_row<VEC>(W_out + (int64_t)c * D, h + f * D * T + t, D, T, 0.f);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NI; idx += FG_NT) {
        const int t = idx & (T - 1), c = idx >> tsh, i = c / D, e = c - i * D;
        const float* g = G + i * F * T + t;
        const float* o = S1 + e * T + t;
        float acc = 0.f;
        for (int j = 0; j < F; ++j) acc = fmaf(g[j * T], o[j * D * T], acc);
        S2[idx] = acc;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NI; idx += FG_NT) {
        const int t = idx & (T - 1), c = idx >> tsh, f = c / D, e = c - f * D;
        S1[idx] = fg_dot_row<VEC>(W_in + (int64_t)c * D, S2 + f * D * T + t, D, T, bp[e]);
    }
    __syncthreads();
}

// grid: min(tiles, FG_MAX_WG) workgroups of FG_NT threads; dynamic LDS 4 * (glds + T * fg_per_sample(F, D, false))
template <int VEC>
__global__ __launch_bounds__(FG_NT) void k_fignn_fwd(FgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = a.F, D = a.D, FD = F * D, T = a.T, tsh = a.tsh, NI = FD << tsh;
    float* X = smem + a.glds;
    float* H = X + FD * T;
    float* S1 = H + FD * T;
    float* S2 = S1 + FD * T;
    float* G = S2 + FD * T;
    float* sd = G + F * F * T;
    const FgGru gw = fg_stage_gru(a, smem);
    const int64_t tiles = (a.B + T - 1) / T;
    const int64_t lwf = (a.flags & FG_REUSE) ? 0 : 2 * (int64_t)FD * D + D;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * T;
        const int rows = a.B - b0 < T ? (int)(a.B - b0) : T;
        __syncthreads();                        // the GRU is staged; the last tile's readers are done
        fg_load_tile<VEC>(X, H, a.X, a.ldx, b0, rows, FD, T, tsh);
        __syncthreads();
        fg_graph(X, a.w_attn, sd, G, F, D, T, tsh);
        float* h = H;
        float* s2 = S2;
        for (int l = 0; l < a.L; ++l) {
            fg_message<VEC>(a.W + l * lwf, h, G, S1, s2, F, D, T, tsh);
            if (a.flags & FG_GRU) {
                for (int idx = threadIdx.x; idx < NI; idx += FG_NT) {
                    const int t = idx & (T - 1), c = idx >> tsh, f = c / D, e = c - f * D;
                    float gi[3], gh[3];
                    fg_gates<VEC>(gw, S1 + f * D * T + t, h + f * D * T + t, e, D, T, gi, gh);
                    const float r = fg_sigmoid(gi[0] + gh[0]), z = fg_sigmoid(gi[1] + gh[1]);
                    const float n = tanhf(fmaf(r, gh[2], gi[2]));
                    float hn = (1.f - z) * n + z * h[idx];
                    if (a.flags & FG_RES) hn += X[idx];
                    s2[idx] = hn;
                }
                float* sw = h; h = s2; s2 = sw;
            } else {
                for (int idx = threadIdx.x; idx < NI; idx += FG_NT) {
                    float hn = S1[idx] + h[idx];
                    if (a.flags & FG_RES) hn += X[idx];
                    h[idx] = hn;
                }
            }
            __syncthreads();
            if (a.hs && l < a.L - 1) fg_store_tile<VEC>(h, a.hs + (int64_t)l * a.B * FD, FD, b0, rows, FD, T, tsh);
        }
        fg_store_tile<VEC>(h, a.h_out, FD, b0, rows, FD, T, tsh);
    }
}

// *p = v (the row's first touch) or *p += v: one owner thread per element, tiles and layers in a fixed order
__device__ __forceinline__ void fg_acc(float* p, float v, bool store) { *p = store ? v : *p + v; }

// grid: min(tiles, FG_MAX_WG) workgroups of FG_NT threads; dynamic LDS 4 * (glds + T * fg_per_sample(F, D, true))
template <int VEC>
__global__ __launch_bounds__(FG_NT) void k_fignn_bwd(FgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int F = a.F, D = a.D, FD = F * D, DD = D * D, T = a.T, tsh = a.tsh, NI = FD << tsh, L = a.L;
    const bool gru = a.flags & FG_GRU, res = a.flags & FG_RES, reuse = a.flags & FG_REUSE;
    float* H = smem + a.glds;
    float* DH = H + FD * T;
    float* DXA = DH + FD * T;
    float* P1 = DXA + FD * T;
    float* P2 = P1 + FD * T;
    float* Q1 = P2 + FD * T;
    float* Q2 = Q1 + FD * T;
    float* Q3 = Q2 + FD * T;
    float* Q4 = Q3 + FD * T;
    float* G = Q4 + FD * T;
    float* DG = G + F * F * T;
    float* sd = DG + F * F * T;
    const FgGru gw = fg_stage_gru(a, smem);
    const int64_t tiles = (a.B + T - 1) / T;
    const int64_t lw = 2 * (int64_t)FD * D + D;                 // floats of a layer's weights (and gradients)
    const int64_t og = (reuse ? 1 : L) * lw;                    // the GRU's gradients in a row
    const int64_t oa = og + (gru ? 6 * DD + 6 * D : 0);         // dW_attn
    float* row = a.partial + (int64_t)blockIdx.x * a.ldp;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * T;
        const int rows = a.B - b0 < T ? (int)(a.B - b0) : T;
        const bool first = tile == blockIdx.x;
        __syncthreads();
        fg_load_tile<VEC>(H, nullptr, a.X, a.ldx, b0, rows, FD, T, tsh);
        fg_load_tile<VEC>(DH, nullptr, a.dH, FD, b0, rows, FD, T, tsh);
        for (int idx = tid; idx < NI; idx += FG_NT) DXA[idx] = 0.f;
        for (int idx = tid; idx < ((F * F) << tsh); idx += FG_NT) DG[idx] = 0.f;
        __syncthreads();
        fg_graph(H, a.w_attn, sd, G, F, D, T, tsh);
        for (int l = L - 1; l >= 0; --l) {
            // the layer's input: hs[l - 1], x for layer 0
            if (l > 0) fg_load_tile<VEC>(H, nullptr, a.hs + (int64_t)(l - 1) * a.B * FD, FD, b0, rows, FD, T, tsh);
            else if (L > 1) fg_load_tile<VEC>(H, nullptr, a.X, a.ldx, b0, rows, FD, T, tsh);
            __syncthreads();
            const int64_t lb = reuse ? 0 : l * lw;
            const float* W_in = a.W + lb;
            const float* W_out = W_in + (int64_t)FD * D;
            const bool st = first && (l == L - 1 || !reuse);
            const bool stg = first && l == L - 1;
            fg_message<VEC>(W_in, H, G, P1, P2, F, D, T, tsh);          // P1 = a, P2 = aggr
            float* DA = DH;                                             // d a (no GRU: h' = a + h)
            if (gru) {
                for (int idx = tid; idx < NI; idx += FG_NT) {
                    const int t = idx & (T - 1), c = idx >> tsh, f = c / D, e = c - f * D;
                    float gi[3], gh[3];
                    fg_gates<VEC>(gw, P1 + f * D * T + t, H + f * D * T + t, e, D, T, gi, gh);
                    const float r = fg_sigmoid(gi[0] + gh[0]), z = fg_sigmoid(gi[1] + gh[1]);
                    const float n = tanhf(fmaf(r, gh[2], gi[2]));
                    const float dh = DH[idx];
                    if (res) DXA[idx] += dh;
                    const float dpn = dh * (1.f - z) * (1.f - n * n);
                    const float dz = dh * (H[idx] - n);
                    DH[idx] = dh * z;
                    Q1[idx] = dpn * gh[2] * r * (1.f - r);
                    Q2[idx] = dz * z * (1.f - z);
                    Q3[idx] = dpn;
                    Q4[idx] = dpn * r;
                }
                __syncthreads();
                // d w_ih | d w_hh | d b_ih | d b_hh: sums over the tile's samples and fields
                for (int item = tid; item < 6 * DD + 6 * D; item += FG_NT) {
                    float s = 0.f;
                    if (item < 6 * DD) {
                        const bool hh = item >= 3 * DD;
                        const int it = hh ? item - 3 * DD : item;
                        const int rw = it / D, d = it - rw * D, q = rw / D, e = rw - q * D;
                        const float* qp = (q == 0 ? Q1 : (q == 1 ? Q2 : (hh ? Q4 : Q3))) + e * T;
                        const float* in = (hh ? H : P1) + d * T;
                        for (int f = 0; f < F; ++f)
                            for (int t = 0; t < T; ++t) s = fmaf(qp[f * D * T + t], in[f * D * T + t], s);
                    } else {
                        const int it = item - 6 * DD;
                        const bool hh = it >= 3 * D;
                        const int rw = hh ? it - 3 * D : it, q = rw / D, e = rw - q * D;
                        const float* qp = (q == 0 ? Q1 : (q == 1 ? Q2 : (hh ? Q4 : Q3))) + e * T;
                        for (int f = 0; f < F; ++f)
                            for (int t = 0; t < T; ++t) s += qp[f * D * T + t];
                    }
                    fg_acc(row + og + item, s, stg);
                }
                __syncthreads();
                // d a -> P1, d h += w_hh^T (the gates' gradients)
                for (int idx = tid; idx < NI; idx += FG_NT) {
                    const int t = idx & (T - 1), c = idx >> tsh, f = c / D, d = c - f * D;
                    const int o = f * D * T + t;
                    float da = 0.f, dhh = 0.f;
                    for (int e = 0; e < D; ++e) {
                        const float q1 = Q1[o + e * T], q2 = Q2[o + e * T], q3 = Q3[o + e * T], q4 = Q4[o + e * T];
                        da = fmaf(gw.w_ih[e * gw.ld + d], q1, da);
                        da = fmaf(gw.w_ih[(D + e) * gw.ld + d], q2, da);
                        da = fmaf(gw.w_ih[(2 * D + e) * gw.ld + d], q3, da);
                        dhh = fmaf(gw.w_hh[e * gw.ld + d], q1, dhh);
                        dhh = fmaf(gw.w_hh[(D + e) * gw.ld + d], q2, dhh);
                        dhh = fmaf(gw.w_hh[(2 * D + e) * gw.ld + d], q4, dhh);
                    }
                    P1[idx] = da;
                    DH[idx] += dhh;
                }
                __syncthreads();
                DA = P1;
            } else if (res) {
                for (int idx = tid; idx < NI; idx += FG_NT) DXA[idx] += DH[idx];
            }
            // d bias_p, d W_in; d aggr -> Q1; o again -> Q2
            for (int e = tid; e < D; e += FG_NT) {
                float s = 0.f;
                for (int f = 0; f < F; ++f)
                    for (int t = 0; t < T; ++t) s += DA[(f * D + e) * T + t];
                fg_acc(row + lb + 2 * (int64_t)FD * D + e, s, st);
            }
            for (int item = tid; item < FD * D; item += FG_NT) {
                const int c = item / D, d = item - c * D, f = c / D;
                const float* p = DA + c * T;
                const float* q = P2 + (f * D + d) * T;
                float s = 0.f;
                for (int t = 0; t < T; ++t) s = fmaf(p[t], q[t], s);
                fg_acc(row + lb + item, s, st);
            }
            for (int idx = tid; idx < NI; idx += FG_NT) {
                const int t = idx & (T - 1), c = idx >> tsh, f = c / D, d = c - f * D;
                Q1[idx] = fg_dot_col(W_in + (int64_t)f * DD + d, DA + f * D * T + t, D, T);
                Q2[idx] = fg_dot_row<VEC>(W_out + (int64_t)c * D, H + f * D * T + t, D, T, 0.f);
            }
            __syncthreads();
            // d g += d aggr_i . o_j;  d o_j = sum_i g[i][j] d aggr_i -> Q3
            for (int idx = tid; idx < ((F * F) << tsh); idx += FG_NT) {
                const int t = idx & (T - 1), ij = idx >> tsh, i = ij / F, j = ij - i * F;
                const float* p = Q1 + i * D * T + t;
                const float* q = Q2 + j * D * T + t;
                float s = 0.f;
                for (int e = 0; e < D; ++e) s = fmaf(p[e * T], q[e * T], s);
                DG[idx] += s;
            }
            for (int idx = tid; idx < NI; idx += FG_NT) {
                const int t = idx & (T - 1), c = idx >> tsh, j = c / D, e = c - j * D;
                const float* g = G + j * T + t;
                const float* p = Q1 + e * T + t;
                float s = 0.f;
                for (int i = 0; i < F; ++i) s = fmaf(g[i * F * T], p[i * D * T], s);
                Q3[idx] = s;
            }
            __syncthreads();
            // d W_out; d h += W_out^T d o
            for (int item = tid; item < FD * D; item += FG_NT) {
                const int c = item / D, d = item - c * D, f = c / D;
                const float* p = Q3 + c * T;
                const float* q = H + (f * D + d) * T;
                float s = 0.f;
                for (int t = 0; t < T; ++t) s = fmaf(p[t], q[t], s);
                fg_acc(row + lb + (int64_t)FD * D + item, s, st);
            }
            for (int idx = tid; idx < NI; idx += FG_NT) {
                const int t = idx & (T - 1), c = idx >> tsh, f = c / D, d = c - f * D;
                DH[idx] += fg_dot_col(W_out + (int64_t)f * DD + d, Q3 + f * D * T + t, D, T);
            }
            __syncthreads();
        }
        // the graph (H holds x again): soft-max and LeakyReLU back to the two score vectors, d s_src -> Q3, d s_dst -> Q4
        for (int idx = tid; idx < (F << tsh); idx += FG_NT) {
            const int t = idx & (T - 1), i = idx >> tsh;
            const float* g = G + i * F * T + t;
            float* dg = DG + i * F * T + t;
            float dot = 0.f;
            for (int j = 0; j < F; ++j) dot = fmaf(g[j * T], dg[j * T], dot);
            const float si = sd[i * T + t];
            float acc = 0.f;
            for (int j = 0; j < F; ++j) {
                float dp = 0.f;
                if (j != i) {
                    const float pre = si + sd[(F + j) * T + t];
                    const float da = g[j * T] * (dg[j * T] - dot);
                    dp = pre > 0.f ? da : 0.01f * da;
                }
                dg[j * T] = dp;
                acc += dp;
            }
            Q3[idx] = acc;
        }
        __syncthreads();
        for (int idx = tid; idx < (F << tsh); idx += FG_NT) {
            const int t = idx & (T - 1), j = idx >> tsh;
            float acc = 0.f;
            for (int i = 0; i < F; ++i) acc += DG[(i * F + j) * T + t];
            Q4[idx] = acc;
        }
        __syncthreads();
        for (int item = tid; item < 2 * D; item += FG_NT) {
            const int d = item < D ? item : item - D;
            const float* p = item < D ? Q3 : Q4;
            float s = 0.f;
            for (int i = 0; i < F; ++i)
                for (int t = 0; t < T; ++t) s = fmaf(p[i * T + t], H[(i * D + d) * T + t], s);
            fg_acc(row + oa + item, s, first);
        }
        for (int idx = tid; idx < NI; idx += FG_NT) {
            const int t = idx & (T - 1), c = idx >> tsh, i = c / D, d = c - i * D;
            float v = DH[idx] + DXA[idx];
            v = fmaf(Q3[i * T + t], a.w_attn[d], v);
            v = fmaf(Q4[i * T + t], a.w_attn[D + d], v);
            DH[idx] = v;
        }
        __syncthreads();
        fg_store_tile<VEC>(DH, a.dX, a.lddx, b0, rows, FD, T, tsh);
    }
}

// ---- the head: a wave per sample, lane d ----------------------------------------------------------------
__global__ __launch_bounds__(FG_HEAD_NT) void k_fignn_head_fwd(const float* H, const float* Z, const float* w1,
                                                               int64_t B, int F, int D, float* logit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = FG_HEAD_NT / 64;
    const float wd = lane < D ? w1[lane] : 0.f;
    for (int64_t b = (int64_t)blockIdx.x * NW + wave; b < B; b += (int64_t)gridDim.x * NW) {
        const float* h = H + b * F * D;
        float acc = 0.f;
        for (int f = 0; f < F; ++f) {
            const float s = fx_wave_sum(lane < D ? h[f * D + lane] * wd : 0.f);
            acc = fmaf(fg_sigmoid(Z[b * F + f]), s, acc);
        }
        if (lane == 0) logit[b] = acc;
    }
}

__global__ __launch_bounds__(FG_HEAD_NT) void k_fignn_head_bwd(const float* g, const float* H, const float* Z,
                                                               const float* w1, int64_t B, int F, int D, float* dH,
                                                               float* dZ, float* partial) {
    __shared__ float red[FG_HEAD_NT / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = FG_HEAD_NT / 64;
    const float wd = lane < D ? w1[lane] : 0.f;
    float acc = 0.f;
    for (int64_t b = (int64_t)blockIdx.x * NW + wave; b < B; b += (int64_t)gridDim.x * NW) {
        const float* h = H + b * F * D;
        const float gb = g[b];
        for (int f = 0; f < F; ++f) {
            const float hv = lane < D ? h[f * D + lane] : 0.f;
            const float s = fx_wave_sum(hv * wd);
            const float wg = fg_sigmoid(Z[b * F + f]);
            const float ds = gb * wg;
            if (lane == 0) dZ[b * F + f] = gb * s * wg * (1.f - wg);
            if (lane < D) dH[b * F * D + f * D + lane] = ds * wd;
            acc = fmaf(ds, hv, acc);
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && lane < D) {
        float s = red[0][lane];
        for (int w = 1; w < NW; ++w) s += red[w][lane];
        partial[(int64_t)blockIdx.x * 64 + lane] = s;
    }
}

// ---- hosts ----------------------------------------------------------------------------------------------
static int fg_check(const char* who, int64_t B, int32_t F, int32_t D, int32_t L, int32_t flags) {
    FX_CHECK_ARG(F >= FG_MIN_F && F <= FG_MAX_F, "%s: F=%d, limit %d <= F <= %d (one field has no neighbour)", who, F,
                 FG_MIN_F, FG_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= FG_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, FG_MAX_D);
    FX_CHECK_ARG((int64_t)F * D <= FG_MAX_FD, "%s: F*D=%lld, limit %d", who, (long long)F * D, FG_MAX_FD);
    FX_CHECK_ARG(L >= 1 && L <= FG_MAX_LAYERS, "%s: layers=%d, limit 1 <= layers <= %d", who, L, FG_MAX_LAYERS);
    FX_CHECK_ARG(flags >= 0 && flags <= (FG_GRU | FG_RES | FG_REUSE), "%s: flags=%d", who, flags);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    return FX_OK;
}

extern "C" void fx_fignn_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = FG_MIN_F;
    limits[1] = FG_MAX_FD;
    limits[2] = FG_MAX_D;
    limits[3] = FG_MAX_LAYERS;
    limits[4] = FG_MAX_F;
}

extern "C" int32_t fx_fignn_tile_rows(int32_t F, int32_t D, int32_t flags, int32_t backward) {
    if (F < FG_MIN_F || F > FG_MAX_F || D < 1 || D > FG_MAX_D || F * D > FG_MAX_FD) return 0;
    return fg_plan(F, D, flags, backward != 0).T;
}

extern "C" int64_t fx_fignn_grad_floats(int32_t F, int32_t D, int32_t layers, int32_t flags) {
    if (F < 1 || D < 1 || layers < 1) return 0;
    return fg_grad_floats(F, D, layers, flags);
}

extern "C" int64_t fx_fignn_workspace_floats(int64_t B, int32_t F, int32_t D, int32_t layers, int32_t flags) {
    const int64_t head = (int64_t)FG_HEAD_WG * 64;
    if (F < FG_MIN_F || F > FG_MAX_F || D < 1 || D > FG_MAX_D || F * D > FG_MAX_FD || layers < 1) return head;
    const int T = fg_plan(F, D, flags, true).T;
    const int64_t tiles = fx_ceil_div(B > 0 ? B : 1, T), wg = tiles < FG_MAX_WG ? tiles : FG_MAX_WG;
    const int64_t n4 = (fg_grad_floats(F, D, layers, flags) + 3) / 4 * 4;
    const int64_t ws = wg > 1 ? wg * n4 : 4;
    return ws > head ? ws : head;
}

static int fg_fill(const char* who, FgArgs& p, const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D, int32_t L,
                   int32_t flags, const float* W, const float* w_ih, const float* w_hh, const float* b_ih,
                   const float* b_hh, const float* w_attn) {
    if (int st = fg_check(who, B, F, D, L, flags)) return st;
    FX_CHECK_ARG(ldx >= (int64_t)F * D, "%s: X row stride %lld < F*D", who, (long long)ldx);
    FX_CHECK_ARG(W && w_attn, "%s: null W / w_attn", who);
    FX_CHECK_ARG(!(flags & FG_GRU) || (w_ih && w_hh && b_ih && b_hh), "%s: null GRU tensor", who);
    memset(&p, 0, sizeof(p));
    p.X = X; p.ldx = ldx; p.W = W; p.w_ih = w_ih; p.w_hh = w_hh; p.b_ih = b_ih; p.b_hh = b_hh; p.w_attn = w_attn;
    p.B = B; p.F = F; p.D = D; p.L = L; p.flags = flags;
    return FX_OK;
}

static bool fg_vec4(const FgArgs& p) {
    return p.D % 4 == 0 && fx_vec_ok(p.X, p.ldx) && fx_al16(p.W) &&
           (!(p.flags & FG_GRU) || (fx_al16(p.w_ih) && fx_al16(p.w_hh)));
}

extern "C" int fx_fignn_fwd(const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D, int32_t layers, int32_t flags,
                            const float* W, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                            const float* w_attn, float* h_out, float* hs, fx_stream_t stream) {
    const char* who = "fx_fignn_fwd";
    FgArgs p;
    if (int st = fg_fill(who, p, X, ldx, B, F, D, layers, flags, W, w_ih, w_hh, b_ih, b_hh, w_attn)) return st;
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(X && h_out, "%s: null X / h_out", who);
    p.h_out = h_out; p.hs = layers > 1 ? hs : nullptr;
    const FgPlan pl = fg_plan(F, D, flags, false);
    p.T = pl.T; p.tsh = pl.tsh; p.glds = pl.glds; p.ldg = pl.ldg;
    const bool vec4 = fg_vec4(p) && fx_al16(h_out) && fx_al16(hs);
    static const hipError_t lds_ok[2] = {fx_allow_lds(k_fignn_fwd<4>, FG_LDS_MAX), fx_allow_lds(k_fignn_fwd<1>, FG_LDS_MAX)};
    FX_CHECK_HIP(lds_ok[vec4 ? 0 : 1]);
    const size_t lds = 4 * (size_t)(pl.glds + pl.T * fg_per_sample(F, D, false));
    const int64_t tiles = fx_ceil_div(B, pl.T);
    const dim3 grid((unsigned)(tiles < FG_MAX_WG ? tiles : FG_MAX_WG)), block(FG_NT);
    hipStream_t s = fx_hip_stream(stream);
    if (vec4) hipLaunchKernelGGL(k_fignn_fwd<4>, grid, block, lds, s, p);
    else hipLaunchKernelGGL(k_fignn_fwd<1>, grid, block, lds, s, p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_fignn_bwd(const float* d_h_out, const float* X, int64_t ldx, int64_t B, int32_t F, int32_t D,
                            int32_t layers, int32_t flags, const float* W, const float* w_ih, const float* w_hh,
                            const float* b_ih, const float* b_hh, const float* w_attn, const float* hs, float* dX,
                            int64_t lddx, float* grads, float* workspace, fx_stream_t stream) {
    const char* who = "fx_fignn_bwd";
    FgArgs p;
    if (int st = fg_fill(who, p, X, ldx, B, F, D, layers, flags, W, w_ih, w_hh, b_ih, b_hh, w_attn)) return st;
    FX_CHECK_ARG(lddx >= (int64_t)F * D, "%s: dX row stride %lld < F*D", who, (long long)lddx);
    FX_CHECK_ARG(grads && workspace, "%s: null grads / workspace", who);
    hipStream_t s = fx_hip_stream(stream);
    const int64_t n = fg_grad_floats(F, D, layers, flags);
    if (B == 0) {
        FX_CHECK_HIP(hipMemsetAsync(grads, 0, sizeof(float) * n, s));
        return FX_OK;
    }
    FX_CHECK_ARG(d_h_out && X && dX, "%s: null d_h_out / X / dX", who);
    FX_CHECK_ARG(layers == 1 || hs, "%s: null hs with %d layers", who, layers);
    p.dH = d_h_out; p.hs = const_cast<float*>(hs); p.dX = dX; p.lddx = lddx;
    const FgPlan pl = fg_plan(F, D, flags, true);
    p.T = pl.T; p.tsh = pl.tsh; p.glds = pl.glds; p.ldg = pl.ldg;
    const int64_t tiles = fx_ceil_div(B, pl.T), wg = tiles < FG_MAX_WG ? tiles : FG_MAX_WG;
    const int64_t n4 = (n + 3) / 4 * 4;
    p.partial = wg > 1 ? workspace : grads;
    p.ldp = wg > 1 ? n4 : n;
    const bool vec4 = fg_vec4(p) && fx_al16(d_h_out) && fx_al16(hs) && fx_vec_ok(dX, lddx);
    static const hipError_t lds_ok[2] = {fx_allow_lds(k_fignn_bwd<4>, FG_LDS_MAX), fx_allow_lds(k_fignn_bwd<1>, FG_LDS_MAX)};
    FX_CHECK_HIP(lds_ok[vec4 ? 0 : 1]);
    const size_t lds = 4 * (size_t)(pl.glds + pl.T * fg_per_sample(F, D, true));
    const dim3 grid((unsigned)wg), block(FG_NT);
    if (vec4) hipLaunchKernelGGL(k_fignn_bwd<4>, grid, block, lds, s, p);
    else hipLaunchKernelGGL(k_fignn_bwd<1>, grid, block, lds, s, p);
    FX_CHECK_LAUNCH();
    if (wg > 1) return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)wg, n4, fx_rowsum_out(grads, n));
    return FX_OK;
}

static int fg_head_check(const char* who, int64_t B, int32_t F, int32_t D) {
    FX_CHECK_ARG(F >= 1 && D >= 1 && D <= FG_MAX_D, "%s: F=%d D=%d, limit F >= 1, 1 <= D <= %d", who, F, D, FG_MAX_D);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    return FX_OK;
}

extern "C" int fx_fignn_head_fwd(const float* H, const float* Z, const float* w1, int64_t B, int32_t F, int32_t D,
                                 float* logit, fx_stream_t stream) {
    const char* who = "fx_fignn_head_fwd";
    if (int st = fg_head_check(who, B, F, D)) return st;
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(H && Z && w1 && logit, "%s: null H / Z / w1 / logit", who);
    const int64_t wg = fx_ceil_div(B, FG_HEAD_NT / 64);
    hipLaunchKernelGGL(k_fignn_head_fwd, dim3((unsigned)(wg < 4096 ? wg : 4096)), dim3(FG_HEAD_NT), 0,
                       fx_hip_stream(stream), H, Z, w1, B, F, D, logit);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_fignn_head_bwd(const float* g, const float* H, const float* Z, const float* w1, int64_t B, int32_t F,
                                 int32_t D, float* dH, float* dZ, float* dw1, float* workspace, fx_stream_t stream) {
    const char* who = "fx_fignn_head_bwd";
    if (int st = fg_head_check(who, B, F, D)) return st;
    FX_CHECK_ARG(dw1 && workspace, "%s: null dw1 / workspace", who);
    hipStream_t s = fx_hip_stream(stream);
    if (B == 0) {
        FX_CHECK_HIP(hipMemsetAsync(dw1, 0, sizeof(float) * D, s));
        return FX_OK;
    }
    FX_CHECK_ARG(g && H && Z && w1 && dH && dZ, "%s: null g / H / Z / w1 / dH / dZ", who);
    int64_t wg = fx_ceil_div(B, FG_HEAD_NT / 64);
    wg = wg < FG_HEAD_WG ? wg : FG_HEAD_WG;
    hipLaunchKernelGGL(k_fignn_head_bwd, dim3((unsigned)wg), dim3(FG_HEAD_NT), 0, s, g, H, Z, w1, B, F, D, dH, dZ,
                       wg > 1 ? workspace : dw1);
    FX_CHECK_LAUNCH();
    if (wg > 1) return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)wg, 64, fx_rowsum_out(dw1, D));
    return FX_OK;
}
