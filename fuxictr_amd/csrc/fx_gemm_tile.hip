// fx_gemm_tile.hip — fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products,
// fp32 accumulate, 157 TFLOP/s dense peak on MI355X) with a fused epilogue: the tile kernels and their
// launch helpers.  Which kernel a problem gets is decided in fx_gemm.hip; the entry points this unit exports
// (fx_gemm_tile_launch_*, fx_gemm_tr_ok) are declared in fx_gemm_int.h.
//
// Replaces the aten::addmm / relu / mul / add launches of
//   fuxictr/pytorch/layers/blocks/mlp_block.py:96            (Linear -> ReLU stack)
//   fuxictr/pytorch/layers/interactions/cross_net.py:126-129 (X_{i+1} = X_i + X_0 * (W X_i + b))
// and their autograd (dX = dZ W, dW = dZ^T X, db = colsum dZ) triggered at rank_model.py:320.
//
// Tiling (one wave = 64 lanes, 4 waves per workgroup, one workgroup per CU at B=4096):
//   block tile 128x128x32, LDS double-buffered (67.5 KB), k-major tiles T[k][m] so that an MFMA operand
//   fragment (lane l: row l&31, k = l>>5) is one conflict-free ds_read_b32;
//   wave tile 64x64 = 2x2 MFMA tiles of 32x32 -> 4 independent accumulators (64 VGPRs);
//   global->register prefetch of tile t+1 is issued before the MFMAs of tile t;
//   blockIdx is remapped so the 8 n-tiles that share one A row-panel run on the same XCD (L2).
#include "fx_common.h"
#include "fx_gemm_int.h"

// Operand tile loader for an R x 32 tile (R = 64 or 128 rows of the non-contracted dimension).
// KC: element (r,k) at P[r*ld + k] (k contiguous) else at P[k*ld + r] (r contiguous).
// LDS image is always k-major T[k][LD]: LD = R+1 when filled by transposing 4-byte writes
// (conflict-free), R+4 when filled by 16-byte writes (keeps 16-B alignment).
template <int R, bool KC, bool VEC>
struct TileLoader {
    static constexpr int NST = R / 32;            // float4 staging registers per thread
    static constexpr int LD = KC ? R + 1 : R + 4;
    float4 st[NST];

    __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, int64_t r0,
                                         int64_t Rext, int64_t k0, int64_t kend) {
#pragma unroll
        for (int p = 0; p < NST; ++p) {
            const int q = threadIdx.x + 256 * p;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (KC) {
                const int64_t r = r0 + (q >> 3);
                const int64_t k = k0 + ((q & 7) << 2);
                if (r < Rext) {
                    const float* src = P + r * ld + k;
                    if constexpr (VEC) {
                        if (k < kend) v = *reinterpret_cast<const float4*>(src);
                    } else {
                        if (k + 0 < kend) v.x = src[0];
                        if (k + 1 < kend) v.y = src[1];
                        if (k + 2 < kend) v.z = src[2];
                        if (k + 3 < kend) v.w = src[3];
                    }
                }
            } else {
                const int64_t k = k0 + q / (R / 4);
                const int64_t r = r0 + ((q % (R / 4)) << 2);
                if (k < kend) {
                    const float* src = P + k * ld + r;
                    if constexpr (VEC) {
                        if (r < Rext) v = *reinterpret_cast<const float4*>(src);
                    } else {
                        if (r + 0 < Rext) v.x = src[0];
                        if (r + 1 < Rext) v.y = src[1];
                        if (r + 2 < Rext) v.z = src[2];
                        if (r + 3 < Rext) v.w = src[3];
                    }
                }
            }
            st[p] = v;
        }
    }

    __device__ __forceinline__ void store(float* __restrict__ T) const {
#pragma unroll
        for (int p = 0; p < NST; ++p) {
            const int q = threadIdx.x + 256 * p;
            if constexpr (KC) {
                const int r = q >> 3, kq = (q & 7) << 2;
                T[(kq + 0) * LD + r] = st[p].x;
                T[(kq + 1) * LD + r] = st[p].y;
                T[(kq + 2) * LD + r] = st[p].z;
                T[(kq + 3) * LD + r] = st[p].w;
            } else {
                const int k = q / (R / 4), r = (q % (R / 4)) << 2;
                *reinterpret_cast<float4*>(T + k * LD + r) = st[p];
            }
        }
    }
};

// BM x BN x 32 block tile, 4 waves as 2 (m) x 2 (n); a wave owns (BM/2) x (BN/2) = MI x NJ MFMA
// tiles of 32x32.  128x128 (one workgroup per CU at 67.5 KB LDS... two fit) is the efficient
// shape when the grid has >= 2 workgroups per CU; at B = 4096 the towers give exactly 256 such
// tiles, so 128x64 / 64x64 are used there to keep 2-4 workgroups per CU in flight: the barrier /
// LDS-refill bubble of one workgroup is then covered by the MFMAs of another.
template <int BM, int BN, bool A_KC, bool B_KC, bool A_VEC, bool B_VEC>
__global__ __launch_bounds__(256) void k_gemm_f32(GemmArgs a) {
    using LoaderA = TileLoader<BM, A_KC, A_VEC>;
    using LoaderB = TileLoader<BN, B_KC, B_VEC>;
    constexpr int LDA = LoaderA::LD, LDB = LoaderB::LD;
    constexpr int MI = BM / 64, NJ = BN / 64;
    __shared__ __attribute__((aligned(16))) float As[2][FX_BK * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][FX_BK * LDB];

    // XCD-aware tile mapping: workgroup L runs on XCD L % 8; give each XCD a contiguous range of
    // tiles (row-major over (tm, tn)) so the n-tiles sharing an A panel share one L2.
    const int64_t nwg = (int64_t)a.tiles_m * a.tiles_n;
    const int64_t L = blockIdx.x;
    int64_t T = L;
    if (nwg >= 8) {
        const int64_t q = nwg >> 3, r = nwg & 7, xcd = L & 7;
        T = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
    }
    const int64_t m0 = (T / a.tiles_n) * BM;
    const int64_t n0 = (T % a.tiles_n) * BN;
    const int z = blockIdx.y;
    const int64_t kbeg = (int64_t)z * a.k_chunk;
    const int64_t kend = (kbeg + a.k_chunk < a.K) ? kbeg + a.k_chunk : a.K;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;

    // optional fused row sums of op(A) (bias gradient when op(A) = dZ^T): blocks of the first
    // tile column add up their A tiles straight from LDS
    const bool do_rowsum = (a.epi.rowsum != nullptr) && (n0 == 0);
    float rsum = 0.f;

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    LoaderA la;
    LoaderB lb;
    const int64_t nk = (kend > kbeg) ? (kend - kbeg + FX_BK - 1) / FX_BK : 0;
    if (nk > 0) {
        la.load(a.A, a.lda, m0, a.M, kbeg, kend);
        lb.load(a.B, a.ldb, n0, a.N, kbeg, kend);
        la.store(As[0]);
        lb.store(Bs[0]);
    }
    __syncthreads();
    for (int64_t t = 0; t < nk; ++t) {
        const int cur = (int)(t & 1);
        if (t + 1 < nk) {
            la.load(a.A, a.lda, m0, a.M, kbeg + (t + 1) * FX_BK, kend);
            lb.load(a.B, a.ldb, n0, a.N, kbeg + (t + 1) * FX_BK, kend);
        }
        const float* as = As[cur] + half * LDA + wm * (BM / 2) + l31;
        const float* bs = Bs[cur] + half * LDB + wn * (BN / 2) + l31;
        if (do_rowsum && threadIdx.x < BM) {
            const float* col = As[cur] + threadIdx.x;
#pragma unroll
            for (int k = 0; k < FX_BK; ++k) rsum += col[k * LDA];
        }
        // Software-pipelined fragment reads, two k-pairs deep: the LDS reads of k-pair s+2 are
        // issued right after the MFMAs of k-pair s (same register set), so an LDS latency is
        // always covered by MFMAs.  Pinned with sched_group_barrier — left alone, hipcc sinks
        // every read next to its use and pays a full LDS latency per MFMA group.
        float fa[2][MI], fb[2][NJ];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[s2][i] = as[(2 * s2) * LDA + 32 * i];
#pragma unroll
            for (int j = 0; j < NJ; ++j) fb[s2][j] = bs[(2 * s2) * LDB + 32 * j];
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
        for (int s2 = 0; s2 < FX_BK / 2; ++s2) {
            const int c = s2 & 1;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i], fb[c][j],
                                                                     acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, MI * NJ, 0);
            if (s2 + 2 < FX_BK / 2) {
#pragma unroll
                for (int i = 0; i < MI; ++i) fa[c][i] = as[(2 * s2 + 4) * LDA + 32 * i];
#pragma unroll
                for (int j = 0; j < NJ; ++j) fb[c][j] = bs[(2 * s2 + 4) * LDB + 32 * j];
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
        }
        if (t + 1 < nk) {
            la.store(As[cur ^ 1]);
            lb.store(Bs[cur ^ 1]);
        }
        __syncthreads();
    }

    if (do_rowsum && threadIdx.x < BM && m0 + threadIdx.x < a.M) {
        if (a.split_k > 1) a.ws[(int64_t)a.split_k * a.M * a.N + (int64_t)z * a.M + m0 + threadIdx.x] = rsum;
        else a.epi.rowsum[m0 + threadIdx.x] = rsum;
    }
    // C/D layout of 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t n = n0 + wn * (BN / 2) + j * 32 + l31;
            if (n >= a.N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m >= a.M) continue;
                if (a.split_k > 1) {
                    a.ws[((int64_t)z * a.M + m) * a.N + n] = acc[i][j][r];
                } else {
                    a.C[m * a.ldc + n] = fx_epilogue(a.epi, acc[i][j][r], m, n);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Software-pipelined variant for 16-byte-aligned operands (every tower GEMM of the B=4096 step).
// The kernel above stops its MFMA stream at every k-tile boundary (wait for the prefetched
// registers, 8-32 ds_writes, barrier, fragment-read latency) — ~15-20 % of a tile when only one
// workgroup fits a CU.  Here the boundary work is spread over the MFMA stream instead:
//   * two register staging sets: the global loads of tile t+2 are issued at the top of tile t,
//     the registers of tile t+1 (loaded a whole tile earlier) go to the other LDS stage during
//     MFMA groups 2..12, one ds_write after each MFMA;
//   * ONE barrier per tile after group 13; groups 14/15 already read the first fragments of tile
//     t+1 from the other stage, so the next tile starts with its MFMAs;
//   * MFMA operands in VGPR form (amdgpu_waves_per_eu(2,2)): with AGPR accumulators the compiler
//     copied all 64 of them in and out around the loop's branches.
// Out-of-range rows / the K tail are clamped addresses + zero selects (no exec-mask branches).
// ---------------------------------------------------------------------------------------------
template <int R, bool KC>
struct PipeLoader {
    static constexpr int NST = R / 32;
    static constexpr int LD = KC ? R + 1 : R + 4;
    const float* P;
    int32_t ld;
    int32_t rc[NST];       // KC: clamped row * ld ; else: clamped first row of the float4
    int32_t kl[NST];       // k of this thread's float4 inside a tile
    uint32_t rok;          // bit p: the row(s) of float4 p exist
    uint32_t voff[NST];    // byte offset of float4 p in tile 0 (valid when the rows exist)
    int32_t kbeg, kend;

    __device__ __forceinline__ void init(const float* P_, int64_t ld_, int64_t r0, int64_t Rext,
                                         int64_t kbeg_, int64_t kend_) {
        P = P_;
        ld = (int32_t)ld_;
        kbeg = (int32_t)kbeg_;
        kend = (int32_t)kend_;
        rok = 0;
#pragma unroll
        for (int p = 0; p < NST; ++p) {
            const int q = threadIdx.x + 256 * p;
            if constexpr (KC) {
                const int32_t r = (int32_t)r0 + (q >> 3);
                kl[p] = (q & 7) << 2;
                if (r < (int32_t)Rext) rok |= 1u << p;
                rc[p] = (r < (int32_t)Rext ? r : (int32_t)Rext - 1) * ld;
                voff[p] = (uint32_t)(rc[p] + kbeg + kl[p]) * 4u;
            } else {
                const int32_t r = (int32_t)r0 + ((q % (R / 4)) << 2);
                kl[p] = q / (R / 4);
                if (r < (int32_t)Rext) rok |= 1u << p;
                rc[p] = r < (int32_t)Rext ? r : (int32_t)Rext - 4;
                voff[p] = (uint32_t)((kbeg + kl[p]) * ld + rc[p]) * 4u;
            }
        }
    }

    // Issues the loads only; the zero select of out-of-range elements happens in store_one, so no
    // instruction between here and the LDS write (a tile later) has to wait for the data.
    // Returns the validity bits of the NST float4s.
    __device__ __forceinline__ uint32_t load(int64_t t, float4 (&st)[NST]) const {
        uint32_t okm = 0;
#pragma unroll
        for (int p = 0; p < NST; ++p) {
            const int32_t k = kbeg + (int32_t)t * FX_BK + kl[p];
            if ((k < kend) && ((rok >> p) & 1u)) okm |= 1u << p;
            if constexpr (KC) {
                const int32_t kc = k < kend ? k : kend - 4;
                st[p] = *reinterpret_cast<const float4*>(P + (rc[p] + kc));
            } else {
                const int32_t kc = k < kend ? k : kend - 1;
                st[p] = *reinterpret_cast<const float4*>(P + (kc * ld + rc[p]));
            }
        }
        return okm;
    }

    // tile fully inside the matrix: uniform tile base + constant 32-bit per-lane byte offset (the
    // global_load saddr form: no per-lane address arithmetic in the loop)
    template <int p>
    __device__ __forceinline__ void load_plain(int64_t t, float4 (&st)[NST], uint32_t& okm) const {
        const int64_t tile_off = KC ? t * (FX_BK * 4) : t * (FX_BK * 4) * (int64_t)ld;
        const char* base = reinterpret_cast<const char*>(P) + tile_off;
        st[p] = *reinterpret_cast<const float4*>(base + voff[p]);
        okm = (1u << NST) - 1u;
    }

    template <int p>
    __device__ __forceinline__ void load_one(int64_t t, float4 (&st)[NST], uint32_t& okm) const {
        const int32_t k = kbeg + (int32_t)t * FX_BK + kl[p];
        if ((k < kend) && ((rok >> p) & 1u)) okm |= 1u << p;
        else okm &= ~(1u << p);
        if constexpr (KC) {
            const int32_t kc = k < kend ? k : kend - 4;
            st[p] = *reinterpret_cast<const float4*>(P + (rc[p] + kc));
        } else {
            const int32_t kc = k < kend ? k : kend - 1;
            st[p] = *reinterpret_cast<const float4*>(P + (kc * ld + rc[p]));
        }
    }

    // one LDS write instruction: component `comp` of float4 p (KC, transposing) or the whole float4
    template <int p, int comp, bool MASK>
    __device__ __forceinline__ void store_piece(float* __restrict__ T, const float4 (&st)[NST],
                                                uint32_t okm) const {
        const int q = threadIdx.x + 256 * p;
        const bool ok = MASK ? ((okm >> p) & 1u) : true;
        if constexpr (KC) {
            const int r = q >> 3, kq = (q & 7) << 2;
            const float x = comp == 0 ? st[p].x : comp == 1 ? st[p].y : comp == 2 ? st[p].z : st[p].w;
            T[(kq + comp) * LD + r] = ok ? x : 0.f;
        } else {
            const int k = q / (R / 4), r = (q % (R / 4)) << 2;
            float4 v;
            v.x = ok ? st[p].x : 0.f;
            v.y = ok ? st[p].y : 0.f;
            v.z = ok ? st[p].z : 0.f;
            v.w = ok ? st[p].w : 0.f;
            *reinterpret_cast<float4*>(T + k * LD + r) = v;
        }
    }

    template <int p>
    __device__ __forceinline__ void store_one(float* __restrict__ T, const float4 (&st)[NST],
                                              uint32_t okm) const {
        const int q = threadIdx.x + 256 * p;
        const bool ok = (okm >> p) & 1u;
        float4 v;
        v.x = ok ? st[p].x : 0.f;
        v.y = ok ? st[p].y : 0.f;
        v.z = ok ? st[p].z : 0.f;
        v.w = ok ? st[p].w : 0.f;
        if constexpr (KC) {
            const int r = q >> 3, kq = (q & 7) << 2;
            T[(kq + 0) * LD + r] = v.x;
            T[(kq + 1) * LD + r] = v.y;
            T[(kq + 2) * LD + r] = v.z;
            T[(kq + 3) * LD + r] = v.w;
        } else {
            const int k = q / (R / 4), r = (q % (R / 4)) << 2;
            *reinterpret_cast<float4*>(T + k * LD + r) = v;
        }
    }
};

template <int BM, int BN, bool A_KC, bool B_KC>
struct PipeSmem {
    static constexpr int SA = FX_BK * PipeLoader<BM, A_KC>::LD, SB = FX_BK * PipeLoader<BN, B_KC>::LD;
    static constexpr int FLOATS = 2 * SA + 2 * SB;
};

// One output tile (linear tile index L of tiles_m x tiles_n, K slab z) of the pipelined GEMM.  A
// device function so that one launch can carry tiles of more than one problem (k_gemm_f32_pair).
// TR: the MFMA is issued with its operands swapped, so the accumulators hold the TRANSPOSED 32x32
// tile — a lane owns ONE row m of C and, per group of four registers, four ADJACENT columns — and the
// epilogue reads its operands and writes C as 16-byte vectors: 4 store instructions per 32x32 tile
// instead of 16 (the drain of a launch is store-issue bound: all workgroups of a launch reach their
// epilogue together).  a*b commutes, the k order is unchanged: bit-identical results.  Needs N % 4 == 0
// and 16-byte aligned C / epilogue operands (fx_gemm_tr_ok).
template <int BM, int BN, bool A_KC, bool B_KC, bool TR = false>
__device__ __forceinline__ void fx_gemm_pipe_tile(const GemmArgs& a, const int64_t L, const int z,
                                                  float* const fx_gemm_smem) {
    FX_LAB_STAMP(0);
    using LoaderA = PipeLoader<BM, A_KC>;
    using LoaderB = PipeLoader<BN, B_KC>;
    constexpr int LDA = LoaderA::LD, LDB = LoaderB::LD;
    constexpr int NSA = LoaderA::NST, NSB = LoaderB::NST, NS = NSA + NSB;
    constexpr int MI = BM / 64, NJ = BN / 64;
    constexpr int SA = FX_BK * LDA, SB = FX_BK * LDB;
    constexpr int NG = FX_BK / 2;                      // MFMA groups (k-pairs) per tile
    float* const As0 = fx_gemm_smem;
    float* const Bs0 = fx_gemm_smem + 2 * SA;

    const int64_t nwg = (int64_t)a.tiles_m * a.tiles_n;
    int64_t T = L;
    if (nwg >= 8) {
        const int64_t q = nwg >> 3, r = nwg & 7, xcd = L & 7;
        T = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
    }
    const int64_t m0 = (T / a.tiles_n) * BM;
    const int64_t n0 = (T % a.tiles_n) * BN;
    const int64_t kbeg = (int64_t)z * a.k_chunk;
    const int64_t kend = (kbeg + a.k_chunk < a.K) ? kbeg + a.k_chunk : a.K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    // Fused row sums of op(A) (the bias gradient when op(A) = dZ^T): a by-product of the A fragments the
    // waves of the first tile column hold anyway — lane l sums A[row l & 31][k] over the k of its half,
    // one exact fma (x * 1 + s) per fragment beside the MFMAs, the two halves meet in one shuffle at
    // the end.  (Round 2 summed 32 LDS values per row and k-tile at the top of the tile body: the
    // n0 == 0 workgroups ran 10 % longer than the rest and ended the launch late,
    // profiles/r03_gemm_lab_b.txt.)  rs_scale = 0 for every other wave: no branch in the loop.
    const bool do_rowsum = (a.epi.rowsum != nullptr) && (n0 == 0) && (wn == 0);
    const float rs_scale = do_rowsum ? 1.f : 0.f;
    float rs[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) rs[i] = 0.f;

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int64_t nk = (kend > kbeg) ? (kend - kbeg + FX_BK - 1) / FX_BK : 0;
    if (nk > 0) {
        LoaderA la;
        LoaderB lb;
        la.init(a.A, a.lda, m0, a.M, kbeg, kend);
        lb.init(a.B, a.ldb, n0, a.N, kbeg, kend);
        float4 ra[2][NSA], rb[2][NSB];
        uint32_t oka[2], okb[2];
        oka[0] = la.load(0, ra[0]);
        okb[0] = lb.load(0, rb[0]);
        oka[1] = la.load(1, ra[1]);      // past the last tile: clamped addresses, all bits clear
        okb[1] = lb.load(1, rb[1]);
        fx_static_for<0, NSA>([&](auto p) { la.template store_one<p.value>(As0, ra[0], oka[0]); });
        fx_static_for<0, NSB>([&](auto p) { lb.template store_one<p.value>(Bs0, rb[0], okb[0]); });
        __syncthreads();
        FX_LAB_STAMP(1);
        const int foff_a = half * LDA + wm * (BM / 2) + l31;
        const int foff_b = half * LDB + wn * (BN / 2) + l31;
        float fa[2][MI], fb[2][NJ];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[c][i] = As0[foff_a + (2 * c) * LDA + 32 * i];
#pragma unroll
            for (int j = 0; j < NJ; ++j) fb[c][j] = Bs0[foff_b + (2 * c) * LDB + 32 * j];
        }
        int s = 0;                                      // LDS stage of tile t
        // MASK = false: the tile being written to LDS (t+1) lies fully inside the matrix, its
        // registers go to LDS as they are (1 instruction per write instead of and/cmp/cndmask/write)
        auto body = [&](int64_t t, auto par, auto msk) {
            constexpr int P = decltype(par)::value;
            constexpr bool MASK = decltype(msk)::value;
            const int sn = s ^ 1;
            // (tile t+1 sits in register set P^1; past the last tile the loads are clamped)
            const uint32_t oka_n = oka[P ^ 1], okb_n = okb[P ^ 1];
            const int64_t tl = t + 2;
            const float* as = As0 + s * SA + foff_a;
            const float* bs = Bs0 + s * SB + foff_b;
            const float* asn = As0 + sn * SA + foff_a;
            const float* bsn = Bs0 + sn * SB + foff_b;
            float* wa = As0 + sn * SA;
            float* wb = Bs0 + sn * SB;

            // One k-pair group = MI*NJ MFMAs.  Its LDS work — MI+NJ fragment reads for group g+2
            // and this group's share of the refill writes — is issued ONE instruction after each
            // MFMA (measured, scripts/ubench/mfma_stream*.hip: a clump of 8 LDS instructions between
            // two groups costs the MFMA pipe ~10 %, spread out it is free with two waves per SIMD).
            fx_static_for<0, NG>([&](auto gg) {
                constexpr int g = decltype(gg)::value;
                constexpr int c = g & 1;
                constexpr int S = MI * NJ;
                constexpr int PA = A_KC ? 4 : 1, PB = B_KC ? 4 : 1;        // LDS writes per float4
                constexpr int NP = NSA * PA + NSB * PB;                     // write pieces per tile
                // groups [0, GL): the NS global loads of tile t+2 (with their address arithmetic);
                // groups [G0, G0+GW): the LDS writes of tile t+1; barrier after group NG-3
                constexpr int GL = 4, G0 = GL, GW = NG - 3 - G0;
                constexpr int llo = g < GL ? (g * NS + GL - 1) / GL : 0;
                constexpr int lhi = g < GL ? ((g + 1) * NS + GL - 1) / GL : 0;
                constexpr int lo = (g >= G0 && g < G0 + GW) ? ((g - G0) * NP + GW - 1) / GW : 0;
                constexpr int hi = (g >= G0 && g < G0 + GW) ? ((g - G0 + 1) * NP + GW - 1) / GW : 0;
                constexpr int NOPS = MI + NJ + (hi - lo) + (lhi - llo);
                float nfa[MI], nfb[NJ];
                fx_static_for<0, S>([&](auto mm) {
                    constexpr int m = decltype(mm)::value;
                    constexpr int i = m / NJ, j = m % NJ;
                    if constexpr (TR)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[c][j], fa[c][i], acc[i][j],
                                                                         0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i], fb[c][j], acc[i][j],
                                                                         0, 0, 0);
                    fx_static_for<0, NOPS>([&](auto oo) {
                        constexpr int o = decltype(oo)::value;
                        if constexpr (o % S == m) {
                            if constexpr (o < MI) {
                                if constexpr (g + 2 < NG) nfa[o] = as[(2 * g + 4) * LDA + 32 * o];
                                else nfa[o] = asn[(2 * (g + 2 - NG)) * LDA + 32 * o];
                            } else if constexpr (o < MI + NJ) {
                                constexpr int jj = o - MI;
                                if constexpr (g + 2 < NG) nfb[jj] = bs[(2 * g + 4) * LDB + 32 * jj];
                                else nfb[jj] = bsn[(2 * (g + 2 - NG)) * LDB + 32 * jj];
                            } else if constexpr (g < GL) {
                                constexpr int idx = llo + (o - MI - NJ);
                                if constexpr (MASK) {
                                    if constexpr (idx < NSA) la.template load_one<idx>(tl, ra[P], oka[P]);
                                    else lb.template load_one<idx - NSA>(tl, rb[P], okb[P]);
                                } else {
                                    if constexpr (idx < NSA) la.template load_plain<idx>(tl, ra[P], oka[P]);
                                    else lb.template load_plain<idx - NSA>(tl, rb[P], okb[P]);
                                }
                            } else {
                                constexpr int pp = lo + (o - MI - NJ);
                                if constexpr (pp < NSA * PA)
                                    la.template store_piece<pp / PA, pp % PA, MASK>(wa, ra[P ^ 1], oka_n);
                                else
                                    lb.template store_piece<(pp - NSA * PA) / PB, (pp - NSA * PA) % PB,
                                                            MASK>(wb, rb[P ^ 1], okb_n);
                            }
                        }
                    });
                    __builtin_amdgcn_sched_barrier(0);
                });
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    // (inline asm on purpose: left to the compiler the MI fmas are SLP-packed into
                    // v_pk_fma_f32, which costs the matrix pipe ~22 cycles per issue beside MFMAs —
                    // MI355X_MICROARCH.md, "price of one filler beside MFMAs")
                    asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(rs[i]) : "s"(rs_scale), "v"(fa[c][i]));
                    fa[c][i] = nfa[i];
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) fb[c][j] = nfb[j];
                // Barrier once per tile, after group NG-3: every read of stage s has been issued (the
                // fragments of the last two groups were fetched in groups NG-4/NG-3) and is complete
                // (lgkmcnt(0)), every wave's writes of stage sn are complete; groups NG-2/NG-1 then
                // prefetch from sn.  Two stages are enough: nobody reads s after this barrier, and
                // the next writes into s (tile t+2's data) come after it in program order.
                if constexpr (g == NG - 3) {
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            s = sn;
        };
        // pairs in the loop, odd tail outside: a skip path inside the loop would join two different
        // "loads in flight" states at the back edge and the compiler then waits vmcnt(0) there
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        const int64_t nk_full = (kend - kbeg) / FX_BK;           // tiles with all 32 k inside
        // plain bodies: tile t+1 (written to LDS) and tile t+2 (loaded) have all 32 k inside.  Tiles on
        // the M / N edge take them too (round 4; FX_GEMM_EDGE_PLAIN=0 restores the masked bodies): the
        // rows past the edge are loaded from clamped, in-range addresses (voff is built from rc) and
        // reach the MFMAs unmasked, but a row m >= M of A only ever feeds row m of C and a column
        // n >= N of B only column n — neither is stored (nor is its row sum).  Only the K tail has to
        // be zero.  624-wide operands (the 39 x 16 record): 10 % of the tiles of a launch were running
        // the masked bodies for their whole K loop and ended the launch late.
        const bool rows_full = (m0 + BM <= a.M) && (n0 + BN <= a.N);
        const int64_t n_plain = (rows_full || a.edge_plain) ? nk_full - 2 : 0;
        int64_t t = 0;
        for (; t + 1 < n_plain; t += 2) {
            body(t, P0{}, std::false_type{});
            body(t + 1, P1{}, std::false_type{});
        }
        for (; t + 1 < nk; t += 2) {
            body(t, P0{}, std::true_type{});
            body(t + 1, P1{}, std::true_type{});
        }
        if (t < nk) body(t, P0{}, std::true_type{});
    }
    FX_LAB_STAMP(2);

    if (a.epi.rowsum != nullptr && n0 == 0) {         // workgroup-uniform
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const float tot = rs[i] + __shfl_xor(rs[i], 32, 64);
            const int64_t m = m0 + wm * (BM / 2) + i * 32 + l31;
            if (do_rowsum && half == 0 && m < a.M) {
                if (a.split_k > 1) a.ws[(int64_t)a.split_k * a.M * a.N + (int64_t)z * a.M + m] = tot;
                else a.epi.rowsum[m] = tot;
            }
        }
    }
    if constexpr (TR) {
        // lane: row m = l31 of the wave tile; registers 4q .. 4q+3: columns 8q + 4*half + 0..3
        constexpr int NT = MI * NJ;
        const int64_t mb = m0 + wm * (BM / 2) + l31, nb = n0 + wn * (BN / 2) + 4 * half;
        if (a.split_k > 1) {
            fx_static_for<0, NT>([&](auto tt) {
                constexpr int i = decltype(tt)::value / NJ, j = decltype(tt)::value % NJ;
                const int64_t m = mb + i * 32;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t n = nb + j * 32 + 8 * q;
                    if (m < a.M && n < a.N)
                        *reinterpret_cast<float4*>(a.ws + ((int64_t)z * a.M + m) * a.N + n) =
                            make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2],
                                        acc[i][j][4 * q + 3]);
                }
            });
        } else {
            FxEpiOps4 ops[2][4];
            auto load_tile = [&](auto tt, FxEpiOps4 (&o)[4]) {
                constexpr int i = decltype(tt)::value / NJ, j = decltype(tt)::value % NJ;
                const int64_t m = mb + i * 32;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t n = nb + j * 32 + 8 * q;
                    if (m < a.M && n < a.N) fx_epi_load4(a.epi, m, n, o[q]);
                }
            };
            load_tile(std::integral_constant<int, 0>{}, ops[0]);
            fx_static_for<0, NT>([&](auto tt) {
                constexpr int t = decltype(tt)::value;
                constexpr int i = t / NJ, j = t % NJ;
                if constexpr (t + 1 < NT) load_tile(std::integral_constant<int, t + 1>{}, ops[(t + 1) & 1]);
                const int64_t m = mb + i * 32;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t n = nb + j * 32 + 8 * q;
                    if (m < a.M && n < a.N) {
                        const float4 v = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1],
                                                     acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
                        *reinterpret_cast<float4*>(a.C + m * a.ldc + n) =
                            fx_epi_apply4(a.epi, v, m, n, ops[t & 1][q]);
                    }
                }
            });
        }
    } else {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int64_t n = n0 + wn * (BN / 2) + j * 32 + l31;
                if (n >= a.N) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t m = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (m >= a.M) continue;
                    if (a.split_k > 1) {
                        a.ws[((int64_t)z * a.M + m) * a.N + n] = acc[i][j][r];
                    } else {
                        a.C[m * a.ldc + n] = fx_epilogue(a.epi, acc[i][j][r], m, n);
                    }
                }
            }
        }
    }
#ifdef FX_GEMM_LAB
    if (a.trace) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        FX_LAB_STAMP(3);
        if (threadIdx.x == 0) {
            const int64_t w = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8;
            a.trace[w + 4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
            a.trace[w + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // HW_REG_XCC_ID
        }
    }
#endif
}

template <int BM, int BN, bool A_KC, bool B_KC, int W = 2, bool TR = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, W)))
void k_gemm_f32_pipe(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[PipeSmem<BM, BN, A_KC, B_KC>::FLOATS];
    fx_gemm_pipe_tile<BM, BN, A_KC, B_KC, TR>(a, blockIdx.x, blockIdx.y, smem);
}

// Two independent GEMMs in ONE launch (fx_gemm_f32_batch): the weight gradient dW = dZ^T X (problem 1,
// operands m-/n-contiguous, split-K slabs) and the input gradient dX = dZ W (problem 2) of a layer
// share dZ and neither depends on the other.  Launched separately each pays its own ramp — all
// workgroups resident at once, prologue loads and epilogue stores in lock step, ~6 us of idle matrix
// pipes per launch (K sweep in profiles/r02_gemm_probe.txt); in one grid the second problem's
// workgroups start as the first one's retire, and the 624-wide CrossNet shapes (640 tiles on 1024
// slots) no longer leave a third of the CUs one workgroup short.
template <int BM, int BN, bool A1, bool B1, bool A2, bool B2, int W, bool TR = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, W)))
void k_gemm_f32_pair(GemmArgs a1, GemmArgs a2) {
    constexpr int F1 = PipeSmem<BM, BN, A1, B1>::FLOATS, F2 = PipeSmem<BM, BN, A2, B2>::FLOATS;
    __shared__ __attribute__((aligned(16))) float smem[F1 > F2 ? F1 : F2];
    const int64_t n1 = (int64_t)a1.tiles_m * a1.tiles_n, w1 = n1 * a1.split_k;
    const int64_t L = blockIdx.x;
    if (L < w1) {
        fx_gemm_pipe_tile<BM, BN, A1, B1, TR>(a1, L % n1, (int)(L / n1), smem);
    } else {
        const int64_t n2 = (int64_t)a2.tiles_m * a2.tiles_n, L2 = L - w1;
        fx_gemm_pipe_tile<BM, BN, A2, B2, TR>(a2, L2 % n2, (int)(L2 / n2), smem);
    }
}

// Up to FX_MULTI_MAX independent GEMMs in ONE launch on 128-row tiles, two workgroups per CU
// (fx_gemm_f32_batch).  Round 3 timelines (profiles/r03_gemm_lab_a.txt): a 128x128 workgroup — one wave per
// SIMD with four accumulators — streams its K loop at 0.91-0.95 of the matrix-pipe peak on its own, while
// the four 64x64 workgroups of a CU (one accumulator per wave) finish between 50 and 81 us of an 81-us
// launch: the SIMD arbitrates oldest-first, the early finishers leave the late ones alone on the pipe at
// a third of its rate.  So: big tiles, and a SECOND problem's workgroup as the co-resident instead of
// three more of the same — the dW and dX products of a layer (and, for DCNv2's parallel structure, the
// cross and the deep layer of the same depth) fill each other's prologue / epilogue gaps.
// cfg bit 0: A k-contiguous, bit 1: B k-contiguous, bit 2: 128x64 tile (else 128x128).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_gemm_f32_multi(MultiArgs a) {
    constexpr int F0 = PipeSmem<128, 128, false, false>::FLOATS, F1 = PipeSmem<128, 128, true, true>::FLOATS,
                  F2 = PipeSmem<128, 128, true, false>::FLOATS;
    constexpr int FM = F0 > F1 ? (F0 > F2 ? F0 : F2) : (F1 > F2 ? F1 : F2);
    __shared__ __attribute__((aligned(16))) float smem[FM];
    int i = 0;
    while (i + 1 < a.n && (int32_t)blockIdx.x >= a.start[i + 1]) ++i;
    // the problem's arguments are read through the kernarg segment pointer (uniform scalar loads):
    // indexing the by-value struct with a run-time index made the compiler copy it to scratch
    const MultiArgs* ka = (const MultiArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const GemmArgs& g = ka->p[i];
    int64_t L = (int64_t)blockIdx.x - a.start[i];
    const int64_t nt = (int64_t)g.tiles_m * g.tiles_n;
    const int z = (int)(L / nt);
    L -= (int64_t)z * nt;
    switch (ka->cfg[i]) {
        case 0: fx_gemm_pipe_tile<128, 128, false, false, true>(g, L, z, smem); break;
        case 1: fx_gemm_pipe_tile<128, 128, true, false, true>(g, L, z, smem); break;
        case 2: fx_gemm_pipe_tile<128, 128, false, true, true>(g, L, z, smem); break;
        case 3: fx_gemm_pipe_tile<128, 128, true, true, true>(g, L, z, smem); break;
        case 4: fx_gemm_pipe_tile<128, 64, false, false, true>(g, L, z, smem); break;
        case 5: fx_gemm_pipe_tile<128, 64, true, false, true>(g, L, z, smem); break;
        case 6: fx_gemm_pipe_tile<128, 64, false, true, true>(g, L, z, smem); break;
        default: fx_gemm_pipe_tile<128, 64, true, true, true>(g, L, z, smem); break;
    }
}

// (Round 2 experiment, removed again: a variant that kept k-contiguous operands in their global
// layout in LDS — T[r][36], one ds_write_b128 per staging float4, one ds_read_b128 per lane and 8-k
// block, i.e. 12 instead of 48 LDS instructions per 16 MFMAs of a 64x64 tile — measured the SAME
// as this kernel on every tower shape (78.9 vs 78.7 us at 4096x1024x1024, identical K slope,
// profiles/r02_gemm_probe.txt): the 64x64 loop is not bound by LDS traffic or instruction issue.)

static int fx_gemm_tr_mode() {     // FX_GEMM_TR=0: 4-byte epilogue stores everywhere (A/B runs)
    static const int mode = fx_env_int("FX_GEMM_TR", 1);
    return mode;
}

static bool fx_al16(const void* p, int64_t ld) {
    return p == nullptr || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0);
}

// the 16-byte epilogue (TR) applies: every vector access of fx_epilogue4 / the slab stores is aligned
bool fx_gemm_tr_ok(const GemmArgs& a) {
    const fx_gemm_epilogue& e = a.epi;
    return fx_gemm_tr_mode() && (a.N & 3) == 0 && fx_al16(a.C, a.ldc) && fx_al16(e.bias, 0) &&
           fx_al16(e.zout, e.ldz) && fx_al16(e.mul, e.ldmul) && fx_al16(e.mask, e.ldmask) &&
           fx_al16(e.add, e.ldadd) && (a.split_k == 1 || fx_al16(a.ws, 0));
}

template <int BM, int BN, bool A_KC, bool B_KC, bool TR>
static int fx_gemm_launch_pipe_tr(dim3 grid, hipStream_t s, const GemmArgs& a) {
    if constexpr (BM * BN <= 64 * 64) {
        // 64x64 tiles need ~110 VGPRs: 4 waves/SIMD = 4 workgroups per CU (LDS 4 x 34 KB), so the
        // 1024 tiles of a 4096 x 1024 layer are all resident in ONE round (2 per CU took two; the
        // 2- and 3-wave builds of round 2, FX_GEMM_W64, measured slower and are gone)
        hipLaunchKernelGGL((k_gemm_f32_pipe<BM, BN, A_KC, B_KC, 4, TR>), grid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL((k_gemm_f32_pipe<BM, BN, A_KC, B_KC, 2, TR>), grid, dim3(256), 0, s, a);
    }
    return FX_OK;
}

template <int BM, int BN, bool A_KC, bool B_KC>
static int fx_gemm_launch_pipe(dim3 grid, hipStream_t s, const GemmArgs& a) {
    if (fx_gemm_tr_ok(a)) return fx_gemm_launch_pipe_tr<BM, BN, A_KC, B_KC, true>(grid, s, a);
    return fx_gemm_launch_pipe_tr<BM, BN, A_KC, B_KC, false>(grid, s, a);
}

template <int BM, int BN>
static int fx_gemm_dispatch_pipe(bool a_kc, bool b_kc, dim3 grid, hipStream_t s, const GemmArgs& a) {
    if (a_kc && b_kc) return fx_gemm_launch_pipe<BM, BN, true, true>(grid, s, a);
    if (a_kc) return fx_gemm_launch_pipe<BM, BN, true, false>(grid, s, a);
    if (b_kc) return fx_gemm_launch_pipe<BM, BN, false, true>(grid, s, a);
    return fx_gemm_launch_pipe<BM, BN, false, false>(grid, s, a);
}

template <int BM, int BN, bool A_KC, bool B_KC>
static void fx_gemm_dispatch_vec(bool av, bool bv, dim3 grid, hipStream_t s, const GemmArgs& a) {
    if (av && bv)
        hipLaunchKernelGGL((k_gemm_f32<BM, BN, A_KC, B_KC, true, true>), grid, dim3(256), 0, s, a);
    else if (av)
        hipLaunchKernelGGL((k_gemm_f32<BM, BN, A_KC, B_KC, true, false>), grid, dim3(256), 0, s, a);
    else if (bv)
        hipLaunchKernelGGL((k_gemm_f32<BM, BN, A_KC, B_KC, false, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_gemm_f32<BM, BN, A_KC, B_KC, false, false>), grid, dim3(256), 0, s, a);
}

template <int BM, int BN>
static void fx_gemm_dispatch_layout(bool a_kc, bool b_kc, bool av, bool bv, dim3 grid,
                                    hipStream_t s, const GemmArgs& a) {
    if (a_kc && b_kc) fx_gemm_dispatch_vec<BM, BN, true, true>(av, bv, grid, s, a);
    else if (a_kc) fx_gemm_dispatch_vec<BM, BN, true, false>(av, bv, grid, s, a);
    else if (b_kc) fx_gemm_dispatch_vec<BM, BN, false, true>(av, bv, grid, s, a);
    else fx_gemm_dispatch_vec<BM, BN, false, false>(av, bv, grid, s, a);
}

// ---- what fx_gemm.hip launches (fx_gemm_int.h) --------------------------------------------------------
static dim3 fx_gemm_tile_grid(const GemmArgs& a) {
    return dim3((unsigned)((int64_t)a.tiles_m * a.tiles_n), (unsigned)a.split_k);
}

int fx_gemm_tile_launch_pipe(int bm, int bn, bool a_kc, bool b_kc, const GemmArgs& a, hipStream_t s) {
    const dim3 grid = fx_gemm_tile_grid(a);
    if (bm == 128 && bn == 128) return fx_gemm_dispatch_pipe<128, 128>(a_kc, b_kc, grid, s, a);
    if (bm == 128) return fx_gemm_dispatch_pipe<128, 64>(a_kc, b_kc, grid, s, a);
    return fx_gemm_dispatch_pipe<64, 64>(a_kc, b_kc, grid, s, a);
}

void fx_gemm_tile_launch_plain(int bm, int bn, bool a_kc, bool b_kc, bool av, bool bv, const GemmArgs& a,
                               hipStream_t s) {
    const dim3 grid = fx_gemm_tile_grid(a);
    if (bm == 128 && bn == 128) fx_gemm_dispatch_layout<128, 128>(a_kc, b_kc, av, bv, grid, s, a);
    else if (bm == 128) fx_gemm_dispatch_layout<128, 64>(a_kc, b_kc, av, bv, grid, s, a);
    else fx_gemm_dispatch_layout<64, 64>(a_kc, b_kc, av, bv, grid, s, a);
}

static int64_t fx_gemm_tile_wgs(const GemmArgs& a) { return (int64_t)a.tiles_m * a.tiles_n * a.split_k; }

void fx_gemm_tile_launch_pair_bwd(const GemmArgs& dw, const GemmArgs& dx, hipStream_t s) {
    const dim3 grid((unsigned)(fx_gemm_tile_wgs(dw) + fx_gemm_tile_wgs(dx)));
    if (fx_gemm_tr_ok(dw) && fx_gemm_tr_ok(dx))
        hipLaunchKernelGGL((k_gemm_f32_pair<64, 64, false, false, true, false, 4, true>), grid, dim3(256), 0, s,
                           dw, dx);
    else
        hipLaunchKernelGGL((k_gemm_f32_pair<64, 64, false, false, true, false, 4, false>), grid, dim3(256), 0, s,
                           dw, dx);
}

void fx_gemm_tile_launch_pair_fwd(const GemmArgs& first, const GemmArgs& second, hipStream_t s) {
    const dim3 grid((unsigned)(fx_gemm_tile_wgs(first) + fx_gemm_tile_wgs(second)));
    hipLaunchKernelGGL((k_gemm_f32_pair<64, 64, true, true, true, true, 4, true>), grid, dim3(256), 0, s, first,
                       second);
}

void fx_gemm_tile_launch_multi(const MultiArgs& ma, int64_t workgroups, hipStream_t s) {
    hipLaunchKernelGGL(k_gemm_f32_multi, dim3((unsigned)workgroups), dim3(256), 0, s, ma);
}
