// fx_gin.hip — AOANet's GeneralizedInteractionNet (model_zoo/AOANet/src/AOANet.py:105-171): the whole stack of L
// generalized-interaction layers in one launch per direction.  The reference forms outer_product [B, S*F, D, D] per
// layer (AOANet.py:165-167; 40 GB at B 4096, F 39, D 40) and contracts it with alpha, W and h.  With n = s*F + f (what
// its two repeats do), S = F for layer 0 and O (num_subspaces) after it, and Wh[o,h,d] = W[o,h,d] h[o,d]:
//     P[b,o,s,h] = sum_d Wh[o,h,d] B_i[b,s,d]          Q[b,o,s,h] = sum_f alpha[s*F+f, o] B_0[b,f,h]
//     out[b,o,h] = sum_s P[b,o,s,h] Q[b,o,s,h]
// For one sample b and one subspace o, P_o = Wh_o B_i^T and Q_o = B_0^T alpha_o are both [h, s] matrices: the two
// products land in the SAME MFMA result layout (rows h, columns s), so P (.) Q is a multiply in registers and the sum
// over s a 16-lane butterfly.  P and Q never leave the registers in the forward.  The shared operands are Wh_o (the A
// side of P) and alpha_o (the B side of Q): every sample of a tile reads the same staged copy.
//
// Products on v_mfma_f32_16x16x4_f32: lane (r16 = lane & 15, kk = lane >> 4) holds element (r16, k = kk) of A and
// (k = kk, r16) of B and rows 4 kk + i of column r16 of the result.  How partial tiles are filled: the K side (d, f, s
// or h, whichever is summed) is padded to a multiple of 4 with ZEROS IN LDS, in both operands (rows and columns of
// every staged image past F, D, S are written as 0 when the image is staged or produced); the M and N sides are not
// padded: a lane whose row or column lies past the edge reads the LAST valid row or column instead (an index clamp),
// and what it computes is dropped: never stored, and masked to 0 before it enters the sum over s.
//
//   k_gin_fwd: 256 threads; a workgroup owns a tile of T whole samples (fx_gin_tile_rows) and walks the tiles with a grid
//       stride.  LDS: xs [T][F4][DS] the tile's B_0, staged once and kept for all layers; two images [T][O4][DS] that
//       B_i ping-pongs through from layer to layer; wh [D4][DS] = Wh_o, al [S4][FS] = alpha_o transposed ([s][f]).
//       F4, D4, O4: rounded up to 4; DS = D4 + 1, FS = F4 + 1: odd row strides.  Per layer and o: stage wh and al (Wh
//       formed while staging), then a wave takes items (sample, 16 rows of h), walks the column tiles of s, and
//       writes out[b, o, h-rows] into the next image.  After the last o the image goes to outs[l] coalesced.
//   k_gin_bwd: the same tiles, layers in reverse.  LDS adds dx [T][F4][DS] (dB_0, accumulated over all layers, written
//       once per sample), dp and dq [T][D4][SS] (dP_o and dQ_o of the tile, rows h, columns s), the layer's input
//       image (from outs[l-1]) and two dOut images.  Per layer and o:
//         A  items as in the forward recompute P_o and Q_o and leave dP = dOut (.) Q, dQ = dOut (.) P in LDS;
//         B  jobs, one 16 x 16 result tile each:
//              dB_i[s, d]   = sum_h dP[h, s] Wh_o[h, d]              (layer 0: B_i is B_0, it goes to dx)
//              dB_0[f, h]  += sum_s alpha_o[f, s] dQ[h, s]
//              dWh_o[h, d]  = sum_{b, s} dP[h, s] B_i[s, d]          K runs over the tile's samples
//              dalpha_o[f, s] = sum_{b, h} B_0[f, h] dQ[h, s]        K runs over the tile's samples
//            dW = dWh (.) h and dh = sum_h dWh (.) W are taken from the dWh tile in registers.
//       The weight gradients of a tile are added into the workgroup's OWN row of the workspace (the first tile stores):
//       always by the same lane, so no fence is needed; fx_rowsum adds the rows in a fixed order into dparams, which has
//       the layout of params.  No atomics: two runs give the same bits.
// Done differently from a once-per-workgroup staging of the weights: at the envelope's edge (D 64, F 64, O 8) one
// layer's Wh and alpha are 128 KB each, so the weights are staged per (tile, layer, o), 32 KB at the most, from L2.
// Built without packed fp32 ops and without SLP vectorisation, as the neighbouring MFMA files.
#include "fx_common.h"
#include "fx_rowsum.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define GIN_MAX_F 64
#define GIN_MAX_D 64
#define GIN_MAX_O 8
#define GIN_MAX_L 8
#define GIN_NT 256
#define GIN_MAX_WG_FWD 512
#define GIN_MAX_WG_BWD 256          // the rows of the weight-gradient partials
#define GIN_MAX_T 16
#define GIN_LDS_MAX (160 * 1024)

struct GinArgs {
    const float* B0; int64_t ldb; int64_t B;
    int F, D, O, L;
    int F4, D4, O4, DS, FS, SS, T;      // SS: row stride of dp / dq, max(F4, O4) + 1
    const float* params; float* outs;   // [L, B, O, D]
    const float* dout;                  // [B, O, D]
    float* dB0; int64_t lddb; int dx_acc;
    float* part; int64_t np;            // [workgroups, np]
};

static inline int gin_r4(int n) { return (n + 3) / 4 * 4; }
__host__ __device__ static inline int gin_layer_floats(int S, int F, int D, int O) { return O * D * D + S * F * O + O * D; }
// where layer l starts in params: [W [O,D,D] | alpha [S*F, O] | h [O,D]] per layer
__host__ __device__ static inline int64_t gin_layer_off(int l, int F, int D, int O) {
    return l == 0 ? 0 : (int64_t)gin_layer_floats(F, F, D, O) + (int64_t)(l - 1) * gin_layer_floats(O, F, D, O);
}
static inline bool gin_in_envelope(int F, int D, int O, int L) {
    return F >= 1 && F <= GIN_MAX_F && D >= 1 && D <= GIN_MAX_D && O >= 1 && O <= GIN_MAX_O && L >= 1 && L <= GIN_MAX_L;
}
// LDS, floats.  Both: wh [D4][DS] | al [max(F4, O4)][FS].  Per sample, forward: xs | 2 images [O4][DS]; backward:
// xs | dx | dp | dq | 3 images
static inline int gin_fixed_floats(int F, int D, int O) {
    const int F4 = gin_r4(F), D4 = gin_r4(D), O4 = gin_r4(O);
    return D4 * (D4 + 1) + (F4 > O4 ? F4 : O4) * (F4 + 1);
}
static inline int gin_sample_floats(int F, int D, int O, bool bwd) {
    const int F4 = gin_r4(F), D4 = gin_r4(D), O4 = gin_r4(O), DS = D4 + 1, SS = (F4 > O4 ? F4 : O4) + 1;
    return bwd ? 2 * F4 * DS + 2 * D4 * SS + 3 * O4 * DS : F4 * DS + 2 * O4 * DS;
}
// the forward aims at half the LDS (two workgroups per CU), the backward at all of it (fewer, larger tiles: fewer
// passes over the workgroup's partial row)
static inline int gin_tile(int F, int D, int O, bool bwd) {
    const int fixed = gin_fixed_floats(F, D, O), per = gin_sample_floats(F, D, O, bwd);
    int T = ((bwd ? GIN_LDS_MAX / 4 : GIN_LDS_MAX / 8) - fixed) / per;
    if (T < 1) T = (GIN_LDS_MAX / 4 - fixed) / per;
    return T > GIN_MAX_T ? GIN_MAX_T : T;
}

__device__ __forceinline__ f32x4 gin_mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// acc += sum over k4 steps of 4 of A B; ap / bp: the lane's element at k = kk, as / bs: floats between k and k + 4
__device__ __forceinline__ f32x4 gin_mm(const float* ap, int as, const float* bp, int bs, int k4, f32x4 acc) {
    for (int ks = 0; ks < k4; ++ks) acc = gin_mfma(ap[ks * as], bp[ks * bs], acc);
    return acc;
}
__device__ __forceinline__ int gin_min(int a, int b) { return a < b ? a : b; }

// the tile's B_0 images xs[t][f][d], zeros past F, D and the batch
__device__ __forceinline__ void gin_stage_x(const GinArgs& a, float* xs, int64_t b0, int rows) {
    const int per = a.F4 * a.DS;
    for (int idx = threadIdx.x; idx < a.T * per; idx += GIN_NT) {
        const int t = idx / per, r = idx - t * per, f = r / a.DS, d = r - f * a.DS;
        xs[idx] = (t < rows && f < a.F && d < a.D) ? a.B0[(b0 + t) * a.ldb + f * a.D + d] : 0.f;
    }
}
// images im[t][o][d] of src [B, O, D] rows b0 .., zeros past O, D and the batch
__device__ __forceinline__ void gin_stage_img(const GinArgs& a, float* im, const float* src, int64_t b0, int rows) {
    const int per = a.O4 * a.DS, OD = a.O * a.D;
    for (int idx = threadIdx.x; idx < a.T * per; idx += GIN_NT) {
        const int t = idx / per, r = idx - t * per, o = r / a.DS, d = r - o * a.DS;
        im[idx] = (t < rows && o < a.O && d < a.D) ? src[(b0 + t) * OD + o * a.D + d] : 0.f;
    }
}
// wh[h][d] = W[o,h,d] h[o,d] and al[s][f] = alpha[s*F+f, o] of layer parameters pl, zeros past D, S and F
__device__ __forceinline__ void gin_stage_w(const GinArgs& a, const float* pl, int S, int S4, int o, float* wh, float* al) {
    const int D = a.D, F = a.F, O = a.O, DS = a.DS, FS = a.FS;
    const float* W = pl + o * D * D;
    const float* alpha = pl + O * D * D;
    const float* hv = alpha + S * F * O + o * D;
    for (int idx = threadIdx.x; idx < a.D4 * DS; idx += GIN_NT) {
        const int h = idx / DS, d = idx - h * DS;
        wh[idx] = (h < D && d < D) ? W[h * D + d] * hv[d] : 0.f;
    }
    for (int idx = threadIdx.x; idx < S4 * FS; idx += GIN_NT) {
        const int s = idx / FS, f = idx - s * FS;
        al[idx] = (s < S && f < F) ? alpha[(s * F + f) * O + o] : 0.f;
    }
}
// the tiles P_o and Q_o (rows h of tile ht, columns s of tile nt) of one sample: x0 its B_0 image, bi its B_i image
__device__ __forceinline__ void gin_pq(const GinArgs& a, const float* wh, const float* al, const float* x0,
                                       const float* bi, int S, int ht, int nt, int r16, int kk, f32x4& p, f32x4& q) {
    const int h = gin_min(16 * ht + r16, a.D - 1), s = gin_min(16 * nt + r16, S - 1);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    p = gin_mm(wh + h * a.DS + kk, 4, bi + s * a.DS + kk, 4, a.D4 / 4, zero);
    q = gin_mm(x0 + kk * a.DS + h, 4 * a.DS, al + s * a.FS + kk, 4, a.F4 / 4, zero);
}

// grid: min(tiles, GIN_MAX_WG_FWD) workgroups of GIN_NT threads; dynamic LDS 4 * (fixed + T * sample floats)
__global__ __launch_bounds__(GIN_NT) void k_gin_fwd(GinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gin_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kk = lane >> 4;
    const int F = a.F, D = a.D, O = a.O, DS = a.DS, T = a.T;
    const int XI = a.F4 * DS, BI = a.O4 * DS, DT = (D + 15) / 16;
    float* xs = gin_lds;
    float* cur = xs + T * XI;
    float* nxt = cur + T * BI;
    float* wh = nxt + T * BI;
    float* al = wh + a.D4 * DS;
    for (int idx = tid; idx < 2 * T * BI; idx += GIN_NT) cur[idx] = 0.f;      // the images' padding stays 0
    const int64_t tiles = (a.B + T - 1) / T;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * T;
        const int rows = a.B - b0 < T ? (int)(a.B - b0) : T;
        __syncthreads();                        // the last tile's readers are done
        gin_stage_x(a, xs, b0, rows);
        for (int l = 0; l < a.L; ++l) {
            const int S = l ? O : F, S4 = l ? a.O4 : a.F4, ST = (S + 15) / 16;
            const float* bin = l ? cur : xs;
            const int bis = l ? BI : XI;
            const float* pl = a.params + gin_layer_off(l, F, D, O);
            for (int o = 0; o < O; ++o) {
                __syncthreads();                // wh / al are free; xs and the last layer's image are complete
                gin_stage_w(a, pl, S, S4, o, wh, al);
                __syncthreads();
                for (int item = wave; item < rows * DT; item += GIN_NT / 64) {
                    const int t = item / DT, ht = item - t * DT;
                    float acc[4] = {0.f, 0.f, 0.f, 0.f};
                    for (int nt = 0; nt < ST; ++nt) {
                        f32x4 p, q;
                        gin_pq(a, wh, al, xs + t * XI, bin + t * bis, S, ht, nt, r16, kk, p, q);
                        if (16 * nt + r16 < S) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[i] += p[i] * q[i];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
#pragma unroll
                        for (int off = 1; off < 16; off <<= 1) acc[i] += __shfl_xor(acc[i], off, 64);
                        const int hh = 16 * ht + 4 * kk + i;
                        if (r16 == 0 && hh < D) nxt[t * BI + o * DS + hh] = acc[i];
                    }
                }
            }
            __syncthreads();
            const int OD = O * D;
            for (int idx = tid; idx < rows * OD; idx += GIN_NT) {
                const int t = idx / OD, r = idx - t * OD, o = r / D, d = r - o * D;
                a.outs[((int64_t)l * a.B + b0 + t) * OD + r] = nxt[t * BI + o * DS + d];
            }
            float* sw = cur; cur = nxt; nxt = sw;
        }
    }
}

// v into the workgroup's partial row: the first tile stores, the later ones add (always the same lane)
__device__ __forceinline__ void gin_part(float* p, float v, bool first) { *p = first ? v : *p + v; }

// grid: min(tiles, GIN_MAX_WG_BWD) workgroups of GIN_NT threads; dynamic LDS 4 * (fixed + T * sample floats)
__global__ __launch_bounds__(GIN_NT) void k_gin_bwd(GinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gin_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kk = lane >> 4;
    const int F = a.F, D = a.D, O = a.O, DS = a.DS, FS = a.FS, SS = a.SS, T = a.T;
    const int XI = a.F4 * DS, BI = a.O4 * DS, PI = a.D4 * SS, DT = (D + 15) / 16, FT = (F + 15) / 16, OD = O * D;
    float* xs = gin_lds;
    float* dx = xs + T * XI;
    float* dp = dx + T * XI;
    float* dq = dp + T * PI;
    float* bi = dq + T * PI;
    float* gcur = bi + T * BI;
    float* gnxt = gcur + T * BI;
    float* wh = gnxt + T * BI;
    float* al = wh + a.D4 * DS;
    float* prow = a.part + (int64_t)blockIdx.x * a.np;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int64_t tiles = (a.B + T - 1) / T;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * T;
        const int rows = a.B - b0 < T ? (int)(a.B - b0) : T;
        const bool first = tile == blockIdx.x;
        __syncthreads();                        // the last tile's readers are done
        gin_stage_x(a, xs, b0, rows);
        for (int idx = tid; idx < T * XI; idx += GIN_NT) dx[idx] = 0.f;
        gin_stage_img(a, gcur, a.dout, b0, rows);
        for (int l = a.L - 1; l >= 0; --l) {
            const int S = l ? O : F, S4 = l ? a.O4 : a.F4, ST = (S + 15) / 16;
            __syncthreads();                    // the layer above is done with bi and has completed gcur
            if (l) gin_stage_img(a, bi, a.outs + (int64_t)(l - 1) * a.B * OD, b0, rows);
            const float* bin = l ? bi : xs;
            const int bis = l ? BI : XI;
            const int64_t loff = gin_layer_off(l, F, D, O);
            const float* pl = a.params + loff;
            float* gl = prow + loff;
            for (int o = 0; o < O; ++o) {
                __syncthreads();                // wh, al, dp, dq are free; the staged images are complete
                gin_stage_w(a, pl, S, S4, o, wh, al);
                __syncthreads();
                // A: dP = dOut (.) Q, dQ = dOut (.) P, zeros past D and S up to the K padding
                for (int item = wave; item < rows * DT; item += GIN_NT / 64) {
                    const int t = item / DT, ht = item - t * DT;
                    float g[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int hh = 16 * ht + 4 * kk + i;
                        g[i] = hh < D ? gcur[t * BI + o * DS + hh] : 0.f;
                    }
                    for (int nt = 0; nt < ST; ++nt) {
                        f32x4 p, q;
                        gin_pq(a, wh, al, xs + t * XI, bin + t * bis, S, ht, nt, r16, kk, p, q);
                        const int c = 16 * nt + r16;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int hh = 16 * ht + 4 * kk + i;
                            const bool live = hh < D && c < S;
                            if (hh < a.D4 && c < S4) {
                                dp[t * PI + hh * SS + c] = live ? g[i] * q[i] : 0.f;
                                dq[t * PI + hh * SS + c] = live ? g[i] * p[i] : 0.f;
                            }
                        }
                    }
                }
                __syncthreads();
                // B: one result tile per job.  The jobs that own a piece of the partial row come first: their wave
                // and lane do not depend on the tile's rows.
                const int n3 = DT, n4 = FT * ST, n1 = l ? rows * ST * DT : 0, n2 = rows * FT * DT;
                for (int j = wave; j < n3 + n4 + n1 + n2; j += GIN_NT / 64) {
                    if (j < n3) {
                        // dWh_o[h, d] = sum_{b, s} dP[h, s] B_i[s, d], a column of tiles; dW = dWh h, dh = sum_h dWh W
                        const int dd = 16 * j + r16, dc = gin_min(dd, D - 1);
                        const float hv = pl[O * D * D + S * F * O + o * D + dc];
                        float dh = 0.f;
                        for (int ht = 0; ht < DT; ++ht) {
                            const int h = gin_min(16 * ht + r16, D - 1);
                            f32x4 acc = zero;
                            for (int t = 0; t < rows; ++t)
                                acc = gin_mm(dp + t * PI + h * SS + kk, 4, bin + t * bis + kk * DS + dc, 4 * DS, S4 / 4, acc);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int hh = 16 * ht + 4 * kk + i;
                                if (hh < D && dd < D) {
                                    const int wi = (o * D + hh) * D + dd;
                                    gin_part(gl + wi, acc[i] * hv, first);
                                    dh += acc[i] * pl[wi];
                                }
                            }
                        }
                        dh += __shfl_xor(dh, 16, 64);
                        dh += __shfl_xor(dh, 32, 64);
                        if (kk == 0 && dd < D) gin_part(gl + O * D * D + S * F * O + o * D + dd, dh, first);
                    } else if (j < n3 + n4) {
                        // dalpha_o[f, s] = sum_{b, h} B_0[f, h] dQ[h, s]
                        const int jj = j - n3, ft = jj / ST, st = jj - ft * ST;
                        const int f = gin_min(16 * ft + r16, F - 1), sc = 16 * st + r16, s = gin_min(sc, S - 1);
                        f32x4 acc = zero;
                        for (int t = 0; t < rows; ++t)
                            acc = gin_mm(xs + t * XI + f * DS + kk, 4, dq + t * PI + kk * SS + s, 4 * SS, a.D4 / 4, acc);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int ff = 16 * ft + 4 * kk + i;
                            if (ff < F && sc < S) gin_part(gl + O * D * D + (sc * F + ff) * O + o, acc[i], first);
                        }
                    } else if (j < n3 + n4 + n1) {
                        // (layers above 0) dB_i[s, d] = sum_h dP[h, s] Wh_o[h, d] into the next dOut image, summed over o
                        const int jj = j - n3 - n4, t = jj / (ST * DT), r = jj - t * ST * DT, st = r / DT, dt = r - st * DT;
                        const int s = gin_min(16 * st + r16, S - 1), dd = 16 * dt + r16, dc = gin_min(dd, D - 1);
                        const f32x4 acc = gin_mm(dp + t * PI + kk * SS + s, 4 * SS, wh + kk * DS + dc, 4 * DS, a.D4 / 4, zero);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int ss = 16 * st + 4 * kk + i;
                            if (ss < S && dd < D) {
                                float* dst = gnxt + t * BI + ss * DS + dd;
                                *dst = o ? *dst + acc[i] : acc[i];
                            }
                        }
                    } else {
                        // dB_0[f, h] += sum_s alpha_o[f, s] dQ[h, s]; layer 0: + dB_i[f, d], B_i being B_0
                        const int jj = j - n3 - n4 - n1, t = jj / (FT * DT), r = jj - t * FT * DT, ft = r / DT, dt = r - ft * DT;
                        const int f = gin_min(16 * ft + r16, F - 1), dd = 16 * dt + r16, dc = gin_min(dd, D - 1);
                        f32x4 acc = gin_mm(al + kk * FS + f, 4 * FS, dq + t * PI + dc * SS + kk, 4, S4 / 4, zero);
                        if (l == 0) acc = gin_mm(dp + t * PI + kk * SS + f, 4 * SS, wh + kk * DS + dc, 4 * DS, a.D4 / 4, acc);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int ff = 16 * ft + 4 * kk + i;
                            if (ff < F && dd < D) dx[t * XI + ff * DS + dd] += acc[i];
                        }
                    }
                }
            }
            float* sw = gcur; gcur = gnxt; gnxt = sw;
        }
        __syncthreads();
        const int FD = F * D;
        for (int idx = tid; idx < rows * FD; idx += GIN_NT) {
            const int t = idx / FD, r = idx - t * FD, f = r / D, d = r - f * D;
            float* dst = a.dB0 + (b0 + t) * a.lddb + r;
            const float v = dx[t * XI + f * DS + d];
            *dst = a.dx_acc ? *dst + v : v;
        }
    }
}

static int gin_check(const char* who, int64_t B, int32_t F, int32_t D, int32_t O, int32_t L, int64_t ldb) {
    FX_CHECK_ARG(F >= 1 && F <= GIN_MAX_F, "%s: F=%d, limit 1 <= F <= %d", who, F, GIN_MAX_F);
    FX_CHECK_ARG(D >= 1 && D <= GIN_MAX_D, "%s: D=%d, limit 1 <= D <= %d", who, D, GIN_MAX_D);
    FX_CHECK_ARG(O >= 1 && O <= GIN_MAX_O, "%s: O=%d, limit 1 <= O <= %d", who, O, GIN_MAX_O);
    FX_CHECK_ARG(L >= 1 && L <= GIN_MAX_L, "%s: L=%d, limit 1 <= L <= %d", who, L, GIN_MAX_L);
    FX_CHECK_ARG(B >= 1, "%s: B=%lld, limit B >= 1", who, (long long)B);
    FX_CHECK_ARG(ldb >= (int64_t)F * D, "%s: B_0 sample stride %lld < F*D", who, (long long)ldb);
    return FX_OK;
}

static void gin_fill(GinArgs& p, int64_t B, int F, int D, int O, int L, bool bwd) {
    memset(&p, 0, sizeof(p));
    p.B = B; p.F = F; p.D = D; p.O = O; p.L = L;
    p.F4 = gin_r4(F); p.D4 = gin_r4(D); p.O4 = gin_r4(O);
    p.DS = p.D4 + 1; p.FS = p.F4 + 1; p.SS = (p.F4 > p.O4 ? p.F4 : p.O4) + 1;
    p.T = gin_tile(F, D, O, bwd);
}
static inline size_t gin_lds_bytes(const GinArgs& p, bool bwd) {
    return 4 * ((size_t)gin_fixed_floats(p.F, p.D, p.O) + (size_t)p.T * gin_sample_floats(p.F, p.D, p.O, bwd));
}
static inline int64_t gin_bwd_grid(int64_t B, int T) {
    const int64_t tiles = fx_ceil_div(B, T);
    return tiles < GIN_MAX_WG_BWD ? tiles : GIN_MAX_WG_BWD;
}

extern "C" void fx_gin_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = GIN_MAX_F;
    limits[1] = GIN_MAX_D;
    limits[2] = GIN_MAX_O;
    limits[3] = GIN_MAX_L;
    limits[4] = GIN_MAX_WG_FWD;     // workgroups of a launch at most (the backward: GIN_MAX_WG_BWD, fewer)
    limits[5] = GIN_MAX_T;          // samples of a tile at most
}

extern "C" int32_t fx_gin_tile_rows(int32_t F, int32_t D, int32_t O, int32_t bwd) {
    return gin_in_envelope(F, D, O, 1) ? gin_tile(F, D, O, bwd != 0) : 0;
}

extern "C" int64_t fx_gin_param_floats(int32_t F, int32_t D, int32_t O, int32_t L) {
    return gin_in_envelope(F, D, O, L) ? gin_layer_off(L, F, D, O) : 0;
}

extern "C" int64_t fx_gin_workspace_floats(int64_t B, int32_t F, int32_t D, int32_t O, int32_t L) {
    if (!gin_in_envelope(F, D, O, L) || B < 1) return 0;
    return gin_bwd_grid(B, gin_tile(F, D, O, true)) * gin_layer_off(L, F, D, O);
}

extern "C" int fx_gin_fwd(const float* B0, int64_t ldb, int64_t B, int32_t F, int32_t D, int32_t O, int32_t L,
                          const float* params, float* outs, fx_stream_t stream) {
    const char* who = "fx_gin_fwd";
    if (int st = gin_check(who, B, F, D, O, L, ldb)) return st;
    FX_CHECK_ARG(B0 && params && outs, "%s: null B_0 / params / outs", who);
    static const hipError_t lds_ok = fx_allow_lds(k_gin_fwd, GIN_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    GinArgs p;
    gin_fill(p, B, F, D, O, L, false);
    p.B0 = B0; p.ldb = ldb; p.params = params; p.outs = outs;
    const int64_t tiles = fx_ceil_div(B, p.T);
    hipLaunchKernelGGL(k_gin_fwd, dim3((unsigned)(tiles < GIN_MAX_WG_FWD ? tiles : GIN_MAX_WG_FWD)), dim3(GIN_NT),
                       gin_lds_bytes(p, false), fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_gin_bwd(const float* dout, const float* B0, int64_t ldb, int64_t B, int32_t F, int32_t D, int32_t O,
                          int32_t L, const float* params, const float* outs, float* dB0, int64_t lddb,
                          int32_t dx_accumulate, float* dparams, float* workspace, fx_stream_t stream) {
    const char* who = "fx_gin_bwd";
    if (int st = gin_check(who, B, F, D, O, L, ldb)) return st;
    FX_CHECK_ARG(lddb >= (int64_t)F * D, "%s: dB_0 sample stride %lld < F*D", who, (long long)lddb);
    FX_CHECK_ARG(dout && B0 && params && outs, "%s: null dout / B_0 / params / outs", who);
    FX_CHECK_ARG(dB0 && dparams && workspace, "%s: null dB_0 / dparams / workspace", who);
    static const hipError_t lds_ok = fx_allow_lds(k_gin_bwd, GIN_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    GinArgs p;
    gin_fill(p, B, F, D, O, L, true);
    p.B0 = B0; p.ldb = ldb; p.params = params; p.outs = const_cast<float*>(outs); p.dout = dout;
    p.dB0 = dB0; p.lddb = lddb; p.dx_acc = dx_accumulate != 0;
    p.part = workspace; p.np = gin_layer_off(L, F, D, O);
    const int64_t grid = gin_bwd_grid(B, p.T);
    hipStream_t s = fx_hip_stream(stream);
    hipLaunchKernelGGL(k_gin_bwd, dim3((unsigned)grid), dim3(GIN_NT), gin_lds_bytes(p, true), s, p);
    FX_CHECK_LAUNCH();
    return fx_rowsum<double, FX_ROWS_SLICES>(s, workspace, (int)grid, p.np, fx_rowsum_out(dparams, p.np));
}
