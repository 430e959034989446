// fx_crossmix.hip — DCNv2's low-rank mixture cross network (CrossNetMix) on the matrix cores.
// Reference: fuxictr/pytorch/layers/interactions/cross_net.py:132-201.  Per layer l, from x_0 = x [B, W]:
//     s_e = gating_e . x_l,  g = softmax_e(s),  h_e = tanh(C_e tanh(V_e^T x_l)),
//     x_{l+1} = x_0 * ([U_1 | .. | U_E] [g_1 h_1 ; .. ; g_E h_E] + b) + x_l        (sum_e g_e = 1 folds the bias)
// so a layer is a DOWN product  Z[B, E r + E] = x_l [V_1 | .. | V_E | gating^T]  (the E gate scores are its last
// columns), a per-sample CHAIN on Z (tanh, the r x r products with C_e, tanh, the soft-max, the scaling by g_e:
// P[B, E r]) and an UP product  x_0 * (P [U_1 | .. | U_E]^T + b) + x_l.
//
// All three products run on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate).  A workgroup (four waves)
// owns a tile of CM_ROWS = 16 samples, the M of one MFMA tile, and takes it through every layer of the stack in one
// launch; it strides over the tiles when there are more tiles than workgroups.  U, V [E, W, r], C [E, r, r] and the
// gate vectors [W] are read in place, streamed from L2: nothing is repacked.  Lane l of a wave holds row l & 15 of
// the A operand / column l & 15 of B and D, k = l >> 4 of A and B, and rows 4 (l >> 4) + i of D.
//   down   the waves split the N = E r + E columns into 16-wide tiles (wave w: tiles w, w + 4, ..; at most CM_MAXT,
//          their accumulators stay in registers over the whole K = W loop).  x_l passes through LDS CM_KC columns
//          at a time (coalesced loads, zero-filled past W and past the batch): the A operand is one ds_read_b32, row
//          stride = 4 mod 64 floats, so the 64 lanes of a read hit 64 different banks.  B is V itself: 16 consecutive
//          floats of a row of V_e per k.  No partial sums cross waves: nothing to reduce, the order is fixed.
//   chain  Z [16, N] lies in LDS.  tanh in place; one thread per sample does the E-way soft-max; the r x r products
//          are MFMA tiles (expert, 16 columns) dealt to the waves, A from LDS, B = C_e from L1; their epilogue
//          writes P = g_e tanh(.) to LDS.  tanh is -em / (2 + em) with em = expm1(-2 |a|) in (-1, 0]: no
//          difference of nearly equal numbers near 0, exactly 1 beyond |a| ~ 9, finite for every finite a.
//   up     the waves split W into 16-wide column tiles; K = E r comes from LDS, B is U (16 bytes apart along k for
//          the four k-lanes, r floats apart along the columns).  The epilogue x_0 * (acc + b) + x_l writes
//          x_{l+1}: 64 consecutive bytes per row and k-lane group.  x_1 .. x_{L-1} go to `xs`, which the backward
//          needs anyway and from which the same workgroup reads the next layer's A operand back after a barrier;
//          the last layer writes `out`.  With `zs` the down product's result is kept for the backward as well.
// The backward walks the layers in reverse in one launch, again a tile of 16 samples per workgroup.  Per layer it
// reads Z_l (saved) and recomputes the chain; then CM_KC columns of W at a time: the up product once more (pre =
// P U^T + b), dpre = dx_{l+1} * x_0 (to memory for dU, its column sums to the workgroup's partial row for dbias, the
// tile to LDS), dx_0 += dx_{l+1} * pre, and dP += dpre U over the chunk (the down product's form: N split over the
// waves).  The chain's backward runs in LDS (dC_l by MFMA over the tile's 16 samples into the partial row); P and
// dZ go to memory for dU, dV and dgating; dx_l = dx_{l+1} + dZ [V | gating]^T is the up product's form and lands in
// dX, which carries dx between the layers (every element is read and written by the same thread).  At layer 0 the
// dx_0 sums are added.  dU_l = dpre^T P, dV_l = x_l^T dZ and dgating = sum_l dZ_gate^T x_l are [W x B] . [B x n]
// products for the project's GEMM (ops.crossmix_bwd); dC and dbias leave through fx_rowsum in a fixed order.
// No atomics anywhere: two runs give the same bits.
#include "fx_common.h"
#include "fx_rowsum.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CM_ROWS 16            // samples per tile: the M of one MFMA
#define CM_WAVES 4
#define CM_NT (64 * CM_WAVES)
#define CM_KC 128             // columns of x_l (of dpre) in LDS at a time
#define CM_KCP (CM_KC + 4)    // its row stride: = 4 mod 64
#define CM_MAXT 5             // 16-wide column tiles of the down product per wave: 4 * 5 * 16 >= 256 + 16
#define CM_MAX_L 8
#define CM_MAX_E 16
#define CM_MAX_R 64
#define CM_MAX_ER 256
#define CM_MAX_W 4096
#define CM_MAX_WG 512         // workgroups of a launch (two per CU): the rows of the backward's partial sums
#define CM_LDS_MAX (128 * 1024)

struct CmArgs {
    const float* U[CM_MAX_L];
    const float* V[CM_MAX_L];
    const float* C[CM_MAX_L];
    const float* bias[CM_MAX_L];
    const float* gate[CM_MAX_E];
    const float* X; int64_t ldx;
    float* out; int64_t ldo;             // forward
    float* xs;                           // [L - 1, B, W]: x_1 .. x_{L-1}
    float* zs;                           // [L, B, NG]: the down products (forward: may be null)
    const float* dOut; int64_t lddo;     // backward
    float* dX; int64_t lddx;
    float* dx0;                          // [B, W]: the x_0 share of dX until layer 0
    float* dpre;                         // [L, B, W]
    float* P;                            // [L, B, N1]
    float* dZ;                           // [L, B, NG]
    float* partial; int64_t ldp;         // per workgroup [L x (E r r) | L x W]
    int64_t B;
    int W, r, E, L, N1, NG, ZP, PP;      // N1 = E r, NG = N1 + E; ZP, PP: LDS row strides of [16, NG] and [16, N1]
};

// row stride (floats) of an LDS matrix of n columns: >= n and = 4 mod 64
__host__ __device__ __forceinline__ int cm_stride(int n) { return (n + 59) / 64 * 64 + 4; }

__device__ __forceinline__ float cm_tanh(float a) {
    const float em = expm1f(-2.f * fabsf(a));
    const float m = -em / (2.f + em);
    return a < 0.f ? -m : m;
}

__device__ __forceinline__ f32x4 cm_mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---- the N-split product: D[16, n] += A[16, k0 .. k0 + kn) M[k, n] with A in LDS (row stride CM_KCP) ----------
// A wave's column tiles are ct = wave + 4 t.  Column c < N1 is (e, j) = (c / r, c % r): M[k, c] = mat[e][k][j], the
// lane's offset e W r + j and k stride r; column N1 + e (with_gate) is gate vector e: stride 1; past that: none.
struct CmCols {
    const float* base[CM_MAXT];
    int stride[CM_MAXT];
    int nt;
};

__device__ __forceinline__ void cm_cols(CmCols& d, const CmArgs* ka, const float* mat, bool with_gate, int wave,
                                        int r16) {
    const int ncol = with_gate ? ka->NG : ka->N1;
    const int tiles = (ncol + 15) >> 4;
    d.nt = tiles > wave ? (tiles - wave + CM_WAVES - 1) / CM_WAVES : 0;
#pragma unroll
    for (int t = 0; t < CM_MAXT; ++t) {
        const int c = 16 * (wave + CM_WAVES * t) + r16;
        d.base[t] = nullptr;
        d.stride[t] = 0;
        if (c < ka->N1) {
            const int e = c / ka->r;
            d.base[t] = mat + (int64_t)e * ka->W * ka->r + (c - e * ka->r);
            d.stride[t] = ka->r;
        } else if (c < ncol) {
            d.base[t] = ka->gate[c - ka->N1];
            d.stride[t] = 1;
        }
    }
}

__device__ __forceinline__ void cm_nsplit(f32x4 (&acc)[CM_MAXT], const CmCols& d, const float* A, int k0, int W,
                                          int r16, int kk) {
    const int kn = W - k0 < CM_KC ? W - k0 : CM_KC;
    const float* ap = A + r16 * CM_KCP + kk;
    for (int ks = 0; ks < kn; ks += 4) {
        const float a = ap[ks];                       // zero past W (the staging fills whole rows)
        const int w = k0 + ks + kk;
#pragma unroll
        for (int t = 0; t < CM_MAXT; ++t) {
            if (t < d.nt) {
                const float b = (d.base[t] && w < W) ? d.base[t][(int64_t)w * d.stride[t]] : 0.f;
                acc[t] = cm_mfma(a, b, acc[t]);
            }
        }
    }
}

// the accumulators of the N-split product to LDS [16, ncol] (row stride ld) and, with `g`, to memory rows of ncol
__device__ __forceinline__ void cm_nsplit_store(const f32x4 (&acc)[CM_MAXT], int nt, float* lds, int ld, int ncol,
                                                float* g, int64_t row0, int64_t B, int wave, int r16, int kk) {
#pragma unroll
    for (int t = 0; t < CM_MAXT; ++t) {
        const int c = 16 * (wave + CM_WAVES * t) + r16;
        if (t < nt && c < ncol) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * kk + i;
                lds[row * ld + c] = acc[t][i];
                if (g && row0 + row < B) g[(row0 + row) * ncol + c] = acc[t][i];
            }
        }
    }
}

// ---- the W-split product: one 16-wide column tile of D[16, W] = A[16, K] M^T, column w ---------------------
// A in LDS (row stride lda), K = (e, j) over mat [E, W, r] and, with_gate, E more over the gate vectors.  Two
// accumulator chains (even and odd k steps) meet in a fixed order.
__device__ __forceinline__ f32x4 cm_wtile(const CmArgs* ka, const float* A, int lda, const float* mat, bool with_gate,
                                          int w, int r16, int kk) {
    const int W = ka->W, r = ka->r, E = ka->E;
    const bool wok = w < W;
    const int wc = wok ? w : 0;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float* arow = A + r16 * lda;
    for (int e = 0; e < E; ++e) {
        const float* mp = mat + ((int64_t)e * W + wc) * r;
        const float* ap = arow + e * r;
        for (int j0 = 0; j0 < r; j0 += 8) {
            int j = j0 + kk;
            bool ok = j < r;
            acc0 = cm_mfma(ok ? ap[j] : 0.f, (ok && wok) ? mp[j] : 0.f, acc0);
            if (j0 + 4 < r) {
                j += 4;
                ok = j < r;
                acc1 = cm_mfma(ok ? ap[j] : 0.f, (ok && wok) ? mp[j] : 0.f, acc1);
            }
        }
    }
    if (with_gate) {
        for (int e0 = 0; e0 < E; e0 += 4) {
            const int e = e0 + kk;
            const bool ok = e < E;
            const float* gp = ka->gate[ok ? e : 0];
            acc0 = cm_mfma(ok ? arow[ka->N1 + e] : 0.f, (ok && wok) ? gp[wc] : 0.f, acc0);
        }
    }
    return acc0 + acc1;
}

// ---- the chain's r x r products: tile (e, 16 columns from c0) of D[16, r] = A[:, e r + k] Cm[e][..] ---------
// element (k, c) of the B operand is Cm[e r r + k sk + c sc]: forward (sk, sc) = (1, r): C_e^T; backward (r, 1): C_e
__device__ __forceinline__ f32x4 cm_ctile(const float* A, int lda, const float* Ce, int r, int sk, int sc, int c0,
                                          int r16, int kk) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int c = c0 + r16;
    const float* ap = A + r16 * lda;
    for (int k0 = 0; k0 < r; k0 += 4) {
        const int k = k0 + kk;
        const bool ok = k < r;
        acc = cm_mfma(ok ? ap[k] : 0.f, (ok && c < r) ? Ce[k * sk + c * sc] : 0.f, acc);
    }
    return acc;
}

// x_l (or dOut / dX ..) [B, W] rows row0 .. row0 + 15, columns k0 .. k0 + CM_KC, into LDS; zeros outside
__device__ __forceinline__ void cm_stage(float* lds, const float* src, int64_t ld, int64_t row0, int64_t B, int k0,
                                         int W) {
    for (int idx = threadIdx.x; idx < CM_ROWS * CM_KC; idx += CM_NT) {
        const int rr = idx / CM_KC, c = idx % CM_KC;
        const int w = k0 + c;
        lds[rr * CM_KCP + c] = (row0 + rr < B && w < W) ? src[(row0 + rr) * ld + w] : 0.f;
    }
}

// Z [16, NG] in LDS -> t1 = tanh(Z[:, :N1]) in place and g [16, CM_MAX_E] = softmax of the last E columns
__device__ __forceinline__ void cm_chain_head(const CmArgs* ka, float* zt, float* gt) {
    const int rr = threadIdx.x >> 4, c16 = threadIdx.x & 15;
    float* zr = zt + rr * ka->ZP;
    for (int c = c16; c < ka->N1; c += 16) zr[c] = cm_tanh(zr[c]);
    if (c16 == 0) {
        const float* s = zr + ka->N1;
        float m = s[0];
        for (int e = 1; e < ka->E; ++e) m = fmaxf(m, s[e]);
        float sum = 0.f;
        for (int e = 0; e < ka->E; ++e) sum += expf(s[e] - m);
        const float inv = 1.f / sum;
        for (int e = 0; e < ka->E; ++e) gt[rr * CM_MAX_E + e] = expf(s[e] - m) * inv;
    }
}

// h = tanh(t1 C_e^T) -> ht (when not null) and P = g h -> pt, the tiles dealt to the waves
__device__ __forceinline__ void cm_chain_mid(const CmArgs* ka, const float* Cl, const float* zt, const float* gt,
                                             float* ht, float* pt, int wave, int r16, int kk) {
    const int r = ka->r, JT = (r + 15) >> 4;
    for (int tt = wave; tt < ka->E * JT; tt += CM_WAVES) {
        const int e = tt / JT, c0 = (tt - e * JT) * 16;
        const f32x4 acc = cm_ctile(zt + e * r, ka->ZP, Cl + e * r * r, r, 1, r, c0, r16, kk);
        if (c0 + r16 < r) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * kk + i;
                const float h = cm_tanh(acc[i]);
                if (ht) ht[row * ka->PP + e * r + c0 + r16] = h;
                pt[row * ka->PP + e * r + c0 + r16] = gt[row * CM_MAX_E + e] * h;
            }
        }
    }
}

__global__ __launch_bounds__(CM_NT) void k_crossmix_fwd(CmArgs args) {
    const CmArgs* ka = (const CmArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) float cm_lds[];
    const int W = ka->W, L = ka->L;
    const int64_t B = ka->B;
    float* xt = cm_lds;                          // [16, CM_KCP]
    float* zt = xt + CM_ROWS * CM_KCP;           // [16, ZP]
    float* pt = zt + CM_ROWS * ka->ZP;           // [16, PP]
    float* gt = pt + CM_ROWS * ka->PP;           // [16, CM_MAX_E]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int64_t tiles = (B + CM_ROWS - 1) / CM_ROWS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * CM_ROWS;
        for (int l = 0; l < L; ++l) {
            const float* xl = l == 0 ? ka->X : ka->xs + (int64_t)(l - 1) * B * W;
            const int64_t ldl = l == 0 ? ka->ldx : W;
            // ---- down
            CmCols d;
            cm_cols(d, ka, ka->V[l], true, wave, r16);
            f32x4 acc[CM_MAXT];
#pragma unroll
            for (int t = 0; t < CM_MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < W; k0 += CM_KC) {
                __threadfence_block();
                __syncthreads();                 // xt is free; the rows of xs written by the layer before are visible
                cm_stage(xt, xl, ldl, row0, B, k0, W);
                __syncthreads();
                cm_nsplit(acc, d, xt, k0, W, r16, kk);
            }
            cm_nsplit_store(acc, d.nt, zt, ka->ZP, ka->NG, ka->zs ? ka->zs + (int64_t)l * B * ka->NG : nullptr, row0, B,
                            wave, r16, kk);
            __syncthreads();
            // ---- chain
            cm_chain_head(ka, zt, gt);
            __syncthreads();
            cm_chain_mid(ka, ka->C[l], zt, gt, nullptr, pt, wave, r16, kk);
            __syncthreads();
            // ---- up
            float* xn = l == L - 1 ? ka->out : ka->xs + (int64_t)l * B * W;
            const int64_t ldn = l == L - 1 ? ka->ldo : W;
            const float* bl = ka->bias[l];
            for (int ct = wave; ct * 16 < W; ct += CM_WAVES) {
                const int w = ct * 16 + r16;
                const f32x4 y = cm_wtile(ka, pt, ka->PP, ka->U[l], false, w, r16, kk);
                if (w < W) {
                    const float b = bl[w];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int64_t row = row0 + 4 * kk + i;
                        if (row < B)
                            xn[row * ldn + w] = ka->X[row * ka->ldx + w] * (y[i] + b) + xl[row * ldl + w];
                    }
                }
            }
        }
        __syncthreads();                         // the next tile's chain must not overtake this one's up product
    }
}

__global__ __launch_bounds__(CM_NT) void k_crossmix_bwd(CmArgs args) {
    const CmArgs* ka = (const CmArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) float cm_lds[];
    const int W = ka->W, r = ka->r, E = ka->E, L = ka->L, N1 = ka->N1, NG = ka->NG, ZP = ka->ZP, PP = ka->PP;
    const int64_t B = ka->B;
    float* dt = cm_lds;                          // [16, CM_KCP]  dpre, CM_KC columns at a time
    float* zt = dt + CM_ROWS * CM_KCP;           // [16, ZP]      Z, then t1 | gate scores
    float* dzt = zt + CM_ROWS * ZP;              // [16, ZP]      dZ
    float* ht = dzt + CM_ROWS * ZP;              // [16, PP]      h
    float* pt = ht + CM_ROWS * PP;               // [16, PP]      P = g h
    float* dpt = pt + CM_ROWS * PP;              // [16, PP]      dP, then da2
    float* gt = dpt + CM_ROWS * PP;              // [16, CM_MAX_E] g
    float* dgt = gt + CM_ROWS * CM_MAX_E;        // [16, CM_MAX_E] dg
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kk = lane >> 4;
    const int rr = threadIdx.x >> 4, c16 = threadIdx.x & 15;      // the element-wise passes: 16 threads per sample
    const int JT = (r + 15) >> 4;
    const int64_t tiles = (B + CM_ROWS - 1) / CM_ROWS;
    float* part = ka->partial + (int64_t)blockIdx.x * ka->ldp;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * CM_ROWS;
        const bool first = tile == blockIdx.x;   // the workgroup's first tile stores its partial sums, later ones add
        for (int l = L - 1; l >= 0; --l) {
            const float* dn = l == L - 1 ? ka->dOut : ka->dX;        // dx_{l+1}
            const int64_t lddn = l == L - 1 ? ka->lddo : ka->lddx;
            const float* Ul = ka->U[l];
            const float* Cl = ka->C[l];
            __threadfence_block();
            __syncthreads();                     // LDS is free; dX and dx0 of the layer above are visible
            // ---- Z_l, the chain again
            {
                const float* zg = ka->zs + (int64_t)l * B * NG;
                for (int c = c16; c < NG; c += 16) zt[rr * ZP + c] = row0 + rr < B ? zg[(row0 + rr) * NG + c] : 0.f;
            }
            __syncthreads();
            cm_chain_head(ka, zt, gt);
            __syncthreads();
            cm_chain_mid(ka, Cl, zt, gt, ht, pt, wave, r16, kk);
            // ---- pre, dpre, dx_0 and dP = dpre U, CM_KC columns of W at a time
            CmCols d;
            cm_cols(d, ka, Ul, false, wave, r16);
            f32x4 acc[CM_MAXT];
#pragma unroll
            for (int t = 0; t < CM_MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            float* dpre_g = ka->dpre + (int64_t)l * B * W;
            float* dbias_p = part + (int64_t)L * N1 * r + (int64_t)l * W;
            for (int k0 = 0; k0 < W; k0 += CM_KC) {
                __syncthreads();                 // pt is written (first pass); dt is free (later ones)
                for (int ctl = wave; ctl < CM_KC / 16 && k0 + 16 * ctl < W; ctl += CM_WAVES) {
                    const int w = k0 + 16 * ctl + r16;
                    const f32x4 y = cm_wtile(ka, pt, PP, Ul, false, w, r16, kk);
                    const float b = w < W ? ka->bias[l][w] : 0.f;
                    float colsum = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int64_t row = row0 + 4 * kk + i;
                        float dp = 0.f;
                        if (row < B && w < W) {
                            const float g = dn[row * lddn + w];
                            dp = g * ka->X[row * ka->ldx + w];
                            const float t0 = g * (y[i] + b);
                            float* d0 = ka->dx0 + row * W + w;
                            *d0 = l == L - 1 ? t0 : *d0 + t0;
                            dpre_g[row * W + w] = dp;
                        }
                        dt[(4 * kk + i) * CM_KCP + 16 * ctl + r16] = dp;
                        colsum += dp;
                    }
                    colsum += __shfl_xor(colsum, 16);
                    colsum += __shfl_xor(colsum, 32);
                    if (kk == 0 && w < W) dbias_p[w] = first ? colsum : dbias_p[w] + colsum;
                }
                __syncthreads();
                cm_nsplit(acc, d, dt, k0, W, r16, kk);
            }
            cm_nsplit_store(acc, d.nt, dpt, PP, N1, nullptr, row0, B, wave, r16, kk);
            __syncthreads();
            // ---- the chain's backward: dg_e = dP_e . h_e, then the soft-max, dh = dP g, da2 = dh (1 - h^2)
            if (c16 < E) {
                const float* dp = dpt + rr * PP + c16 * r;
                const float* hp = ht + rr * PP + c16 * r;
                float s = 0.f;
                for (int j = 0; j < r; ++j) s += dp[j] * hp[j];
                dgt[rr * CM_MAX_E + c16] = s;
            }
            __syncthreads();
            if (c16 < E) {
                float dot = 0.f;
                for (int e = 0; e < E; ++e) dot += gt[rr * CM_MAX_E + e] * dgt[rr * CM_MAX_E + e];
                dzt[rr * ZP + N1 + c16] = gt[rr * CM_MAX_E + c16] * (dgt[rr * CM_MAX_E + c16] - dot);
            }
            for (int e = 0; e < E; ++e) {
                const float g = gt[rr * CM_MAX_E + e];
                for (int j = c16; j < r; j += 16) {
                    const int c = rr * PP + e * r + j;
                    const float h = ht[c];
                    dpt[c] = dpt[c] * g * (1.f - h * h);
                }
            }
            __syncthreads();
            // dC_l[e][j][k] = sum_samples da2[s][e r + j] t1[s][e r + k]: 16 x 16 tiles over the tile's 16 samples
            for (int tt = wave; tt < E * JT * JT; tt += CM_WAVES) {
                const int e = tt / (JT * JT), j0 = (tt / JT % JT) * 16, k0 = (tt % JT) * 16;
                f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s0 = 0; s0 < CM_ROWS; s0 += 4) {
                    const int s = s0 + kk;
                    const float a = j0 + r16 < r ? dpt[s * PP + e * r + j0 + r16] : 0.f;
                    const float b = k0 + r16 < r ? zt[s * ZP + e * r + k0 + r16] : 0.f;
                    c4 = cm_mfma(a, b, c4);
                }
                if (k0 + r16 < r) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = j0 + 4 * kk + i;
                        if (j < r) {
                            float* p = part + (int64_t)l * N1 * r + (e * r + j) * r + k0 + r16;
                            *p = first ? c4[i] : *p + c4[i];
                        }
                    }
                }
            }
            // dt1 = da2 C_e, dZ = dt1 (1 - t1^2)
            for (int tt = wave; tt < E * JT; tt += CM_WAVES) {
                const int e = tt / JT, c0 = (tt - e * JT) * 16;
                const f32x4 g4 = cm_ctile(dpt + e * r, PP, Cl + e * r * r, r, r, 1, c0, r16, kk);
                if (c0 + r16 < r) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = 4 * kk + i;
                        const float t1 = zt[row * ZP + e * r + c0 + r16];
                        dzt[row * ZP + e * r + c0 + r16] = g4[i] * (1.f - t1 * t1);
                    }
                }
            }
            __syncthreads();
            if (row0 + rr < B) {
                float* pg = ka->P + ((int64_t)l * B + row0 + rr) * N1;
                float* zg = ka->dZ + ((int64_t)l * B + row0 + rr) * NG;
                for (int c = c16; c < N1; c += 16) pg[c] = pt[rr * PP + c];
                for (int c = c16; c < NG; c += 16) zg[c] = dzt[rr * ZP + c];
            }
            // ---- dx_l = dx_{l+1} + dZ [V | gating]^T; layer 0: + the dx_0 sums
            for (int ct = wave; ct * 16 < W; ct += CM_WAVES) {
                const int w = ct * 16 + r16;
                const f32x4 y = cm_wtile(ka, dzt, ZP, ka->V[l], true, w, r16, kk);
                if (w < W) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int64_t row = row0 + 4 * kk + i;
                        if (row < B) {
                            float v = dn[row * lddn + w] + y[i];
                            if (l == 0) v += ka->dx0[row * W + w];
                            ka->dX[row * ka->lddx + w] = v;
                        }
                    }
                }
            }
        }
    }
}

// ---- hosts ----------------------------------------------------------------------------------------------
static size_t cm_lds_bytes(int r, int E, bool backward) {
    const int ZP = cm_stride(E * r + E), PP = cm_stride(E * r);
    const int per = backward ? CM_KCP + 2 * ZP + 3 * PP + 2 * CM_MAX_E : CM_KCP + ZP + PP + CM_MAX_E;
    return sizeof(float) * CM_ROWS * (size_t)per;
}

static int64_t cm_workgroups(int64_t B) {
    const int64_t tiles = fx_ceil_div(B > 0 ? B : 1, CM_ROWS);
    return tiles < CM_MAX_WG ? tiles : CM_MAX_WG;
}

static int64_t cm_partial_ld(int32_t W, int32_t r, int32_t E, int32_t L) {
    return ((int64_t)L * ((int64_t)E * r * r + W) + 3) / 4 * 4;
}

static int cm_fill(const char* who, CmArgs& p, const float* X, int64_t ldx, int64_t B, int32_t W, int32_t r, int32_t E,
                   int32_t L, const float* const* U, const float* const* V, const float* const* C,
                   const float* const* bias, const float* const* gate) {
    FX_CHECK_ARG(W >= 1 && W <= CM_MAX_W, "%s: W=%d, limit 1 <= W <= %d", who, W, CM_MAX_W);
    FX_CHECK_ARG(r >= 1 && r <= CM_MAX_R, "%s: low_rank=%d, limit 1 <= low_rank <= %d", who, r, CM_MAX_R);
    FX_CHECK_ARG(E >= 1 && E <= CM_MAX_E, "%s: num_experts=%d, limit 1 <= num_experts <= %d", who, E, CM_MAX_E);
    FX_CHECK_ARG(E * r <= CM_MAX_ER, "%s: num_experts*low_rank=%d, limit %d", who, E * r, CM_MAX_ER);
    FX_CHECK_ARG(L >= 1 && L <= CM_MAX_L, "%s: layers=%d, limit 1 <= layers <= %d", who, L, CM_MAX_L);
    FX_CHECK_ARG(B >= 0, "%s: B=%lld", who, (long long)B);
    FX_CHECK_ARG(ldx >= W, "%s: X row stride %lld < W", who, (long long)ldx);
    FX_CHECK_ARG(U && V && C && bias && gate, "%s: null U / V / C / bias / gate list", who);
    memset(&p, 0, sizeof(p));
    for (int l = 0; l < L; ++l) {
        FX_CHECK_ARG(U[l] && V[l] && C[l] && bias[l], "%s: null U / V / C / bias of layer %d", who, l);
        p.U[l] = U[l]; p.V[l] = V[l]; p.C[l] = C[l]; p.bias[l] = bias[l];
    }
    for (int e = 0; e < E; ++e) {
        FX_CHECK_ARG(gate[e], "%s: null gate vector %d", who, e);
        p.gate[e] = gate[e];
    }
    p.X = X; p.ldx = ldx; p.B = B; p.W = W; p.r = r; p.E = E; p.L = L;
    p.N1 = E * r; p.NG = E * r + E; p.ZP = cm_stride(p.NG); p.PP = cm_stride(p.N1);
    return FX_OK;
}

extern "C" void fx_crossmix_limits(int32_t* limits) {
    if (!limits) return;
    limits[0] = CM_ROWS;
    limits[1] = CM_MAX_W;
    limits[2] = CM_MAX_R;
    limits[3] = CM_MAX_E;
    limits[4] = CM_MAX_ER;
    limits[5] = CM_MAX_L;
    limits[6] = CM_MAX_WG;
}

extern "C" int64_t fx_crossmix_workspace_floats(int64_t B, int32_t W, int32_t r, int32_t E, int32_t L) {
    if (B < 0 || W < 1 || W > CM_MAX_W || r < 1 || r > CM_MAX_R || E < 1 || E > CM_MAX_E || E * r > CM_MAX_ER ||
        L < 1 || L > CM_MAX_L)
        return 0;
    return (B * W + 3) / 4 * 4 + cm_workgroups(B) * cm_partial_ld(W, r, E, L);
}

extern "C" int fx_crossmix_fwd(const float* X, int64_t ldx, int64_t B, int32_t W, int32_t r, int32_t E, int32_t L,
                               const float* const* U, const float* const* V, const float* const* C,
                               const float* const* bias, const float* const* gate, float* out, int64_t ldo,
                               float* xs, float* zs, fx_stream_t stream) {
    const char* who = "fx_crossmix_fwd";
    CmArgs p;
    if (int st = cm_fill(who, p, X, ldx, B, W, r, E, L, U, V, C, bias, gate)) return st;
    FX_CHECK_ARG(ldo >= W, "%s: out row stride %lld < W", who, (long long)ldo);
    if (B == 0) return FX_OK;
    FX_CHECK_ARG(X && out, "%s: null X / out", who);
    FX_CHECK_ARG(L == 1 || xs, "%s: null xs with %d layers", who, L);
    p.out = out; p.ldo = ldo; p.xs = xs; p.zs = zs;
    static const hipError_t lds_ok = fx_allow_lds(k_crossmix_fwd, CM_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    hipLaunchKernelGGL(k_crossmix_fwd, dim3((unsigned)cm_workgroups(B)), dim3(CM_NT), cm_lds_bytes(r, E, false),
                       fx_hip_stream(stream), p);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_crossmix_bwd(const float* dOut, int64_t lddo, const float* X, int64_t ldx, int64_t B, int32_t W,
                               int32_t r, int32_t E, int32_t L, const float* const* U, const float* const* V,
                               const float* const* C, const float* const* bias, const float* const* gate,
                               const float* zs, float* dX, int64_t lddx, float* dpre, float* P, float* dZ, float* dC,
                               float* dbias, float* workspace, fx_stream_t stream) {
    const char* who = "fx_crossmix_bwd";
    CmArgs p;
    if (int st = cm_fill(who, p, X, ldx, B, W, r, E, L, U, V, C, bias, gate)) return st;
    FX_CHECK_ARG(lddo >= W && lddx >= W, "%s: dOut / dX row stride %lld / %lld < W", who, (long long)lddo,
                 (long long)lddx);
    FX_CHECK_ARG(B >= 1, "%s: B=%lld (an empty batch has no gradient to sum)", who, (long long)B);
    FX_CHECK_ARG(dOut && X && zs && dX && dpre && P && dZ && dC && dbias && workspace,
                 "%s: null dOut / X / zs / dX / dpre / P / dZ / dC / dbias / workspace", who);
    const int64_t wg = cm_workgroups(B);
    p.dOut = dOut; p.lddo = lddo; p.zs = const_cast<float*>(zs);
    p.dX = dX; p.lddx = lddx; p.dpre = dpre; p.P = P; p.dZ = dZ;
    p.dx0 = workspace;
    p.partial = workspace + (B * W + 3) / 4 * 4;
    p.ldp = cm_partial_ld(W, r, E, L);
    static const hipError_t lds_ok = fx_allow_lds(k_crossmix_bwd, CM_LDS_MAX);
    FX_CHECK_HIP(lds_ok);
    hipStream_t s = fx_hip_stream(stream);
    hipLaunchKernelGGL(k_crossmix_bwd, dim3((unsigned)wg), dim3(CM_NT), cm_lds_bytes(r, E, true), s, p);
    FX_CHECK_LAUNCH();
    return fx_rowsum<double, FX_ROWS_SLICES>(s, p.partial, (int)wg, p.ldp,
                                             fx_rowsum_out(dC, (int64_t)L * E * r * r, dbias, (int64_t)L * W));
}
