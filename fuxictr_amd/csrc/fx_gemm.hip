// fx_gemm.hip — the host side of the dense GEMMs: validation, K split and tile choice of a problem
// (fx_gemm_prepare), the predicates that say which kernels may take it, the planners of the multi-problem
// launches, and the two entry points fx_gemm_f32 / fx_gemm_f32_batch.  No kernel lives here: the tile kernels
// are in fx_gemm_tile.hip (fp32 MFMA) and fx_gemm_x6.hip (split bf16), the skinny ones in fx_gemm_skinny.hip,
// the slab reduces in fx_gemm_reduce.hip; their host launchers are declared in fx_gemm_int.h.
#include "fx_common.h"
#include "fx_gemm_int.h"

#include <mutex>

// The strategy record (fx_gemm_last_strategy): what the last fx_gemm_f32 / fx_gemm_f32_batch call of THIS thread
// launched.  Host side only, a thread_local struct written on the way to the launch: nothing on the device, no
// lock (backward batches come from the autograd engine's thread and have their own record).  Diagnostic only.
static thread_local fx_gemm_strategy_record fx_rec;
static thread_local bool fx_rec_in_batch = false;     // fx_gemm_f32 called from the single launches of a batch

static void fx_rec_reset(int32_t n_problems) {
    memset(&fx_rec, 0, sizeof(fx_rec));
    fx_rec.n_problems = n_problems;
}

// one problem of the call: the arm that took it, its tile, its K slabs, 16-byte epilogue on / off.  A batch of
// more than FX_GEMM_RECORD_SLOTS problems (single launches only) keeps the last ones.
static void fx_rec_put(int slot, int32_t arm, int bm, int bn, int32_t split_k, bool tr) {
    fx_rec.arm[slot] = arm; fx_rec.tile_bm[slot] = bm; fx_rec.tile_bn[slot] = bn;
    fx_rec.split_k[slot] = split_k; fx_rec.tr[slot] = tr ? 1 : 0;
    if (slot >= fx_rec.n) fx_rec.n = slot + 1;
}

static void fx_rec_push(int32_t arm, int bm, int bn, int32_t split_k, bool tr) {
    if (fx_rec.n == FX_GEMM_RECORD_SLOTS) {
        for (int i = 1; i < FX_GEMM_RECORD_SLOTS; ++i) {
            fx_rec.arm[i - 1] = fx_rec.arm[i]; fx_rec.tile_bm[i - 1] = fx_rec.tile_bm[i];
            fx_rec.tile_bn[i - 1] = fx_rec.tile_bn[i]; fx_rec.split_k[i - 1] = fx_rec.split_k[i];
            fx_rec.tr[i - 1] = fx_rec.tr[i];
        }
        fx_rec.n = FX_GEMM_RECORD_SLOTS - 1;
    }
    fx_rec_put(fx_rec.n, arm, bm, bn, split_k, tr);
    if (!fx_rec_in_batch) fx_rec.strategy = arm;
}

extern "C" int fx_gemm_last_strategy(fx_gemm_strategy_record* out) {
    if (out) *out = fx_rec;
    return fx_rec.strategy;
}

static int fx_gemm_pipe_mode() {   // FX_GEMM_PIPE=0 falls back to the unpipelined kernel (A/B runs)
    static const int mode = fx_env_int("FX_GEMM_PIPE", 1);
    return mode;
}

// Validation, K split and tile choice of one GEMM: fills `a`, bm, bn (M == 0 || N == 0: nothing to do,
// a.M stays 0).
static int fx_gemm_prepare(int32_t transa, int32_t transb, int64_t M, int64_t N, int64_t K,
                           const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                           int64_t ldc, const fx_gemm_epilogue* epi_host, int32_t split_k,
                           float* workspace, GemmArgs& a, int& bm_out, int& bn_out) {
    memset(&a, 0, sizeof(a));
    FX_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "fx_gemm_f32: negative dimension");
    if (M == 0 || N == 0) return FX_OK;
    FX_CHECK_ARG(A && B && C, "fx_gemm_f32: null matrix");
    FX_CHECK_ARG(lda >= (transa ? M : K) && ldb >= (transb ? K : N) && ldc >= N,
                 "fx_gemm_f32: leading dimension too small (lda=%lld ldb=%lld ldc=%lld)",
                 (long long)lda, (long long)ldb, (long long)ldc);
    if (split_k < 1) split_k = 1;
    FX_CHECK_ARG(split_k == 1 || workspace, "fx_gemm_f32: split_k > 1 needs a workspace");
    a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K;
    if (epi_host) a.epi = *epi_host;
    // K per split, rounded up to the k-tile so every split starts on a 16-B boundary
    int64_t kc = fx_ceil_div(fx_ceil_div(K, split_k), FX_BK) * FX_BK;
    if (kc < FX_BK) kc = FX_BK;
    split_k = (int32_t)fx_ceil_div(K > 0 ? K : 1, kc);
    a.k_chunk = kc;
    a.split_k = split_k;
    a.ws = workspace;
    // tile shape: the largest one that still gives ~2 workgroups per CU (256 CUs)
    int bm = 128, bn = 128;
    {
        static const int forced = []() {   // FX_GEMM_TILE=128x128|128x64|64x64 (experiments)
            const char* e = getenv("FX_GEMM_TILE");
            if (!e) return 0;
            if (!strcmp(e, "128x128")) return 1;
            if (!strcmp(e, "128x64")) return 2;
            if (!strcmp(e, "64x64")) return 3;
            return 0;
        }();
        // Measured on MI355X (profiles/r01_gemm_pipe.txt).  Bare GEMMs favour the big tile (4096^3:
        // 134 TFLOP/s at 128x128 vs 116 at 64x64), but inside the training step every GEMM has an
        // epilogue that touches 16-32 MB (bias+ReLU, ReLU mask, split-K slabs): with one 128x128
        // workgroup per CU all epilogues run at the same time and nothing covers them; with 64x64
        // tiles three workgroups share a CU and one's epilogue hides under the others' MFMAs.
        // Whole DeepFM step: 1.20 ms (64x64) vs 1.22 (128x64) vs 1.24 (128x128 where it fits).
        // So: 128x128 only when there are >= 4 waves of them (epilogues then overlap anyway), 64x64 below that;
        // 128x64 is the tile of N <= 64 alone.  (A rule "128x64 when that gives >= 2048 workgroups" stood between
        // the two until it was seen that no shape reaches it: ceil(N/64) <= 2 ceil(N/128), so fewer than 1024
        // workgroups of 128x128 are fewer than 2048 of 128x64.)
        const int64_t t128 = fx_ceil_div(M, 128) * fx_ceil_div(N, 128) * split_k;
        if (forced == 2) { bn = 64; }
        else if (forced == 3) { bm = 64; bn = 64; }
        else if (forced == 0 && N <= 64) {
            bn = 64;   // e.g. the DIN attention MLP: 204800 x 64 x 64 — do not pad N to 128
        } else if (forced == 0 && !fx_gemm_pipe_mode()) {
            if (t128 < 448) { bm = 64; bn = 64; }      // the unpipelined kernel's rule
        // (round 3: with the 16-byte epilogue a 128x128 workgroup per CU ties with four 64x64 ones on
        // some boxes — 71.3 vs 71.4 us for 4096x1024x1024 — and loses 4 % on others — 78.2 vs 75.2 us,
        // whole DeepFM step 1.043 vs 1.026 ms, profiles/r03_gemm_lab_h.txt: the single launches keep 64x64)
        } else if (forced == 0 && t128 < 1024) {
            bm = 64; bn = 64;
        }
    }
    a.tiles_m = (int32_t)fx_ceil_div(M, bm);
    a.tiles_n = (int32_t)fx_ceil_div(N, bn);
    {
        // FX_GEMM_EDGE_PLAIN=0: masked bodies on edge tiles (A/B)
        static const int edge_plain = fx_env_int("FX_GEMM_EDGE_PLAIN", 1);
        a.edge_plain = edge_plain;
    }
#ifdef FX_GEMM_LAB
    a.trace = fx_gemm_lab_trace;
#endif
    bm_out = bm;
    bn_out = bn;
    return FX_OK;
}

// av / bv: op(A) / op(B) can be read as 16-byte vectors along its contiguous dimension
static void fx_gemm_operand_vec(int32_t transa, int32_t transb, const GemmArgs& a, bool& av, bool& bv) {
    const bool a_kc = !transa, b_kc = transb != 0;
    const bool a_al = (a.lda % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.A) & 15) == 0);
    const bool b_al = (a.ldb % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.B) & 15) == 0);
    av = a_al && (a_kc ? (a.K % 4 == 0) : (a.M % 4 == 0));
    bv = b_al && (b_kc ? (a.K % 4 == 0) : (a.N % 4 == 0));
}

// operand alignment / offset range (32-bit byte offsets) the pipelined kernel needs
static bool fx_gemm_pipe_ok(int32_t transa, int32_t transb, const GemmArgs& a) {
    bool av, bv;
    fx_gemm_operand_vec(transa, transb, a, av, bv);
    const bool small_offsets = (transa ? a.K * a.lda : a.M * a.lda) < (int64_t)0x3FFFFFF0 &&
                               (transb ? a.N * a.ldb : a.K * a.ldb) < (int64_t)0x3FFFFFF0;
    return fx_gemm_pipe_mode() && av && bv && small_offsets && a.k_chunk >= 4;
}

// The split-bf16 kernels (fx_gemm_x6.hip) take a prepared problem when its operands satisfy the pipelined
// kernel's alignment rules and the 16-byte epilogue's, the output has at least a few 128x128 tiles per slab
// and a fused row sum is asked of a row-contiguous op(A) only (the weight gradients' dZ^T).  Measured on one
// box against the fp32-MFMA kernels (profiles/r05_gemm_x6s_lab_a.txt): 4096x1024x1024 forward 50.6 vs 86.6 us,
// dX 52.4 vs 88.5, dW (4 slabs) 57.3 vs 91.7, 4096x624x624 29.3 vs 43.0; a 256x256x128 product loses
// (8.4 vs 7.2 us): small outputs stay on the fp32 kernels' 64x64 tiles.
#define FX_X6_MIN_WGS 96
static bool fx_gemm_x6_shape(int64_t M, int64_t N, int64_t K) {
    return fx_gemm_x6_enabled() && M >= 128 && N >= 128 && K >= 64;
}

static bool fx_gemm_x6_ok(int32_t transa, int32_t transb, const GemmArgs& a) {
    if (!fx_gemm_x6_shape(a.M, a.N, a.K)) return false;
    if (!fx_gemm_pipe_ok(transa, transb, a) || !fx_gemm_tr_ok(a)) return false;
    if (a.epi.rowsum && !transa) return false;
    // one 8-wave workgroup per CU at ~1.7x the fp32 kernels' per-CU rate against 64x64 tiles that fill the chip
    // with a quarter of the output.  Measured on one box (profiles/r05_gemm_x6_tile_threshold.txt, K = 1024
    // forward with bias + ReLU): 128 tiles 40.5 vs 48.6 us, 96 tiles 38.6 vs 46.7, 64 tiles 36.6 vs 30.8 —
    // the split-bf16 kernels take a launch from 96 workgroups up
    return fx_ceil_div(a.M, 128) * fx_ceil_div(a.N, 128) * a.split_k >= FX_X6_MIN_WGS;
}

// K slabs of a problem on the x6 kernels: about 1024 deep (fx_multi_plan's rule), within the caller's cap
static int32_t fx_splitk_rule_x6(int64_t K, int32_t cap) {
    if (cap <= 1) return 1;
    int64_t sk = (K + 512) / 1024;
    if (sk > cap) sk = cap;
    return (int32_t)(sk < 1 ? 1 : sk);
}

// One GEMM: skinny kernels, else the split-bf16 kernels, else the pipelined fp32-MFMA kernel, else the plain one.
extern "C" int fx_gemm_f32(int32_t transa, int32_t transb, int64_t M, int64_t N, int64_t K,
                           const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                           int64_t ldc, const fx_gemm_epilogue* epi_host, int32_t split_k,
                           float* workspace, fx_stream_t stream) {
    GemmArgs a;
    int bm = 0, bn = 0;
    int rc = fx_gemm_prepare(transa, transb, M, N, K, A, lda, B, ldb, C, ldc, epi_host, split_k, workspace, a,
                             bm, bn);
    if (!fx_rec_in_batch) fx_rec_reset(1);
    if (rc != FX_OK) return rc;
    if (M == 0 || N == 0) return FX_OK;
    hipStream_t s = fx_hip_stream(stream);
    FX_CHECK_ARG(!a.epi.rowsum || (K > 8 && !(N <= 4 && !transa)),
                 "fx_gemm_f32: epilogue.rowsum is not available on the K<=8 / N<=4 skinny paths");
    if (fx_gemm_skinny_launch(transa, transb, a, s, &rc)) {
        if (rc == FX_OK) fx_rec_push(FX_GEMM_SKINNY, 0, 0, a.split_k, false);
        return rc;
    }
    const bool a_kc = !transa, b_kc = transb != 0;
    if (fx_gemm_x6_ok(transa, transb, a)) {
        a.tiles_m = (int32_t)fx_ceil_div(M, 128);
        a.tiles_n = (int32_t)fx_ceil_div(N, 128);
        rc = fx_gemm_x6_launch(a_kc, b_kc, a, s);
        if (rc != FX_OK) return rc;
        fx_rec_push(FX_GEMM_X6, 128, 128, a.split_k, true);
    } else if (fx_gemm_pipe_ok(transa, transb, a)) {
        rc = fx_gemm_tile_launch_pipe(bm, bn, a_kc, b_kc, a, s);
        if (rc != FX_OK) return rc;
        FX_CHECK_LAUNCH();
        fx_rec_push(FX_GEMM_PIPE, bm, bn, a.split_k, fx_gemm_tr_ok(a));
    } else {
        bool av, bv;
        fx_gemm_operand_vec(transa, transb, a, av, bv);
        fx_gemm_tile_launch_plain(bm, bn, a_kc, b_kc, av, bv, a, s);
        FX_CHECK_LAUNCH();
        fx_rec_push(FX_GEMM_PLAIN, bm, bn, a.split_k, false);
        fx_rec.plain_vec[fx_rec.n - 1] = (av ? 1 : 0) | (bv ? 2 : 0);
    }
    if (a.split_k > 1) {
        fx_launch_splitk_reduce(a, s);
        FX_CHECK_LAUNCH();
    }
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------
// fx_gemm_f32_batch: several independent GEMMs in as few launches as possible.  The first of these that takes
// the problem list launches it (fx_batch_try_*, in this order):
//   1. multi x6      2 .. FX_MULTI_MAX non-skinny problems that all qualify for the split-bf16 kernels: one
//                    grid of 128x128 tiles, K slabs from fx_x6_plan_splits, longest workgroups first;
//   2. multi fp32    2 .. FX_MULTI_MAX aligned, non-skinny problems of a backward pass (at least one K split):
//                    ONE k_gemm_f32_multi grid on 128-row tiles, two workgroups per CU; tile (128x128 |
//                    128x64) and K slabs per problem from fx_multi_plan, longest workgroups first;
//   3. backward pair the dW / dX pair of a layer on 64x64 tiles (what FX_GEMM_MULTI=0 or a launch of fewer
//                    than 512 workgroups leaves to it);
//   4. head backward the two gradients of a Linear(hidden -> 1) head in one pass (FX_HEAD_FUSE=0: off);
//   5. forward pair  two x W^T products on 64x64 tiles, the longer one first (FX_GEMM_FWDPAIR=0: off);
//   else             problem by problem through fx_gemm_f32.
// FX_GEMM_PAIR=0 turns 1, 2, 3 and 5 off; FX_GEMM_MULTI=0 turns 1 and 2 off; FX_GEMM_BF16X6=0 turns 1 off.
// ---------------------------------------------------------------------------------------------
struct MultiPlanItem {
    int tile;      // 0: 128x128, 1: 128x64
    int sk;
};

struct MultiShape {
    int64_t M, N, K;
    int splittable;      // 0: no K split; else the LARGEST number of slabs the caller's workspace holds
};

// Tile and K split of every problem of one multi-problem launch.  Rules read off the forced-configuration
// sweeps of round 3 (profiles/r03_gemm_lab_f.txt; a list-scheduling model of the launch was tried first
// and ranked the candidates poorly — 16 % off the best configuration on DCNv2's first layer):
//   * a K split brings the slabs of a weight gradient to ~1024 deep (what the other problems of the
//     launch run: equal workgroup lengths pack best), within the caller's cap;
//   * 128x128 tiles, unless the problem then has fewer workgroups than CUs AND is one of the small
//     products of the launch (< 0.7 of the largest one's flops): 128x64 doubles its workgroups (the
//     624-wide CrossNet products: 100 / 160 -> 200 / 320 workgroups fill the second slot of the CUs
//     beside the deep layer's 256 + 256) — 258 -> 234 us on cross + deep 1024, 201 -> 182 us on the
//     first layer;
//   * returns the launch's workgroup count on 128x128 tiles: below 512 (two per CU) the grid cannot
//     keep both slots busy and the 64x64 pair kernel / single launches win (pair 1024x624: 147 vs 126
//     us, 256x512: 57 vs 30 us, profiles/r03_gemm_lab_g.txt) — the caller falls back.
// FX_MULTI_CFG="tile,sk;tile,sk;..." overrides (experiments).
static int64_t fx_multi_plan(const MultiShape* sh, int n, MultiPlanItem* plan) {
    double fmax = 0.0;
    for (int i = 0; i < n; ++i) {
        const double f = (double)sh[i].M * sh[i].N * sh[i].K;
        if (f > fmax) fmax = f;
    }
    int64_t wg128 = 0;         // workgroups of the launch on 128x128 tiles
    for (int i = 0; i < n; ++i) {
        int sk = 1;
        if (sh[i].splittable > 1) {
            sk = (int)((sh[i].K + 512) / 1024);
            if (sk > sh[i].splittable) sk = sh[i].splittable;
            if (sk < 1) sk = 1;
        }
        const int64_t t128 = fx_ceil_div(sh[i].M, 128) * fx_ceil_div(sh[i].N, 128);
        const double f = (double)sh[i].M * sh[i].N * sh[i].K;
        plan[i].sk = sk;
        plan[i].tile = (sh[i].N <= 64 || (t128 * sk < 256 && f < 0.7 * fmax)) ? 1 : 0;
        wg128 += t128 * sk;
    }
    static const char* forced = getenv("FX_MULTI_CFG");
    if (forced) {
        const char* q = forced;
        for (int i = 0; i < n && *q; ++i) {
            plan[i].tile = atoi(q);
            while (*q && *q != ',' && *q != ';') ++q;
            if (*q == ',') {
                ++q;
                const int sk = atoi(q);
                if (sk >= 1 && sk <= (sh[i].splittable ? sh[i].splittable : 1)) plan[i].sk = sk;
                while (*q && *q != ';') ++q;
            }
            if (*q == ';') ++q;
            if (sh[i].N <= 64) plan[i].tile = 1;
        }
        return 1 << 20;
    }
    return wg128;
}

// split_k of a problem is the LARGEST slab count its workspace holds; the 64x64 paths use the rule of
// round 2 below that cap: about 1024 workgroups, a power of two, K slabs of >= 256
static int32_t fx_splitk_rule64(int64_t M, int64_t N, int64_t K, int32_t cap) {
    if (cap <= 1) return 1;
    const int64_t tiles = fx_ceil_div(M, 64) * fx_ceil_div(N, 64);
    int64_t s = 1;
    if (tiles >= 768) s = 1;
    else if (tiles <= 4) { s = fx_ceil_div(512, tiles); if (s > 256) s = 256; }
    else {
        const double want = 1024.0 / (double)tiles;
        while ((double)s * 1.5 < want) s *= 2;
        if (s > 16) s = 16;
    }
    if (s > K / 256) s = K / 256;
    if (s > cap) s = cap;
    return (int32_t)(s < 1 ? 1 : s);
}

static bool fx_gemm_skinny(const fx_gemm_problem& q) {
    return fx_gemm_is_skinny(q.transa, q.transb, q.M, q.N, q.K, q.workspace);
}

static int fx_gemm_prepare(const fx_gemm_problem& q, int32_t split_k, GemmArgs& a) {
    int bm = 0, bn = 0;     // (the batch paths count tiles_m / tiles_n in their own tile)
    return fx_gemm_prepare(q.transa, q.transb, q.M, q.N, q.K, q.A, q.lda, q.B, q.ldb, q.C, q.ldc, q.epilogue,
                           split_k, q.workspace, a, bm, bn);
}

// order[0 .. n) = 0 .. n-1 by descending key: the longest workgroups go first in a grid.  (A selection by strict
// `>` exchanges: problems of equal key keep the order this gives them — grid order decides which problem's
// tiles start first.)
static void fx_order_desc(const double* key, int n, int* order) {
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int a2 = 0; a2 < n; ++a2)
        for (int b2 = a2 + 1; b2 < n; ++b2)
            if (key[order[b2]] > key[order[a2]]) { const int t = order[a2]; order[a2] = order[b2]; order[b2] = t; }
}

static bool fx_gemm_pair_on() {       // FX_GEMM_PAIR=0: always problem by problem, but for the head (A/B runs)
    static const bool on = fx_env_int("FX_GEMM_PAIR", 1) != 0;
    return on;
}

static int fx_gemm_multi_mode() {     // FX_GEMM_MULTI=0: the 64x64 pair / per-problem paths of round 2
    static const int mode = fx_env_int("FX_GEMM_MULTI", 1);
    return mode;
}

// K slabs of the problems of one split-bf16 multi-problem launch.  One 8-wave workgroup per CU: the launch is a
// list-scheduling problem on 256 machines — a workgroup costs a fixed part (pipeline fill + epilogue: ~9 us) plus
// ~1.2 us per k tile, workgroups start in grid order (longest first) as CUs free up — and the slab count of the
// weight gradients is the one free parameter: 1024 x 624 x 4096 (dW) beside 4096 x 624 x 1024 (dX) is 160 + 160
// workgroups of 32 k tiles at 4 slabs — a full round and a quarter-full one, 64 k tiles of wall time — but
// 320 + 160 workgroups that pack into ~48 at 8 slabs.  Every combination of {1,2,3,4,6,8,12,16} slabs (within
// the caller's workspace cap, slabs >= 256 deep) is simulated, plus what its slab reduces cost; the best one is
// kept per shape set (the simulation runs once per distinct launch).
struct FxX6PlanKey {
    int64_t d[FX_MULTI_MAX][4];
    int n;
    bool operator==(const FxX6PlanKey& o) const { return n == o.n && memcmp(d, o.d, sizeof(d)) == 0; }
};

static double fx_x6_makespan(const int64_t* tiles, const int64_t* ktiles, const int32_t* sk, const int* order,
                             int n) {
    double cu[256];
    for (int i = 0; i < 256; ++i) cu[i] = 0.0;
    // CUs as a binary min-heap on their free time (all zero: already a heap)
    auto sift = [&](int i) {
        for (;;) {
            int l = 2 * i + 1, r = l + 1, m = i;
            if (l < 256 && cu[l] < cu[m]) m = l;
            if (r < 256 && cu[r] < cu[m]) m = r;
            if (m == i) return;
            const double t = cu[i]; cu[i] = cu[m]; cu[m] = t;
            i = m;
        }
    };
    double end = 0.0;
    for (int oi = 0; oi < n; ++oi) {
        const int i = order[oi];
        const double len = 9.0 + 1.2 * (double)fx_ceil_div(ktiles[i], sk[i]);
        const int64_t jobs = tiles[i] * sk[i];
        for (int64_t j = 0; j < jobs; ++j) {
            cu[0] += len;
            if (cu[0] > end) end = cu[0];
            sift(0);
        }
    }
    return end;
}

static void fx_x6_plan_splits(const fx_gemm_problem* p, int n, int32_t* sk_out) {
    // (forward batches are launched from the main thread, backward ones from the autograd engine's thread: the
    // cache is locked — ADVICE r5 — and a plan never exceeds this problem's workspace cap, see the clamp below)
    static FxX6PlanKey keys[64];
    static int32_t plans[64][FX_MULTI_MAX];
    static int n_cached = 0, n_next = 0;
    static std::mutex mtx;
    std::lock_guard<std::mutex> lock(mtx);
    FxX6PlanKey key;
    memset(&key, 0, sizeof(key));
    key.n = n;
    int64_t tiles[FX_MULTI_MAX], ktiles[FX_MULTI_MAX];
    int32_t cap[FX_MULTI_MAX];
    for (int i = 0; i < n; ++i) {
        cap[i] = (p[i].split_k > 1 && p[i].workspace) ? p[i].split_k : 1;
        key.d[i][0] = p[i].M; key.d[i][1] = p[i].N; key.d[i][2] = p[i].K; key.d[i][3] = cap[i];
        tiles[i] = fx_ceil_div(p[i].M, 128) * fx_ceil_div(p[i].N, 128);
        ktiles[i] = fx_ceil_div(p[i].K, FX_BK);
    }
    for (int c = 0; c < n_cached; ++c)
        if (keys[c] == key) {
            for (int i = 0; i < n; ++i) sk_out[i] = plans[c][i] <= cap[i] ? plans[c][i] : cap[i];
            return;
        }
    // FX_X6_PLAN=0: ~1024-deep slabs (round 5's first cut)
    static const bool planner_on = fx_env_int("FX_X6_PLAN", 1) != 0;
    static const int cand[8] = {1, 2, 3, 4, 6, 8, 12, 16};
    int32_t best[FX_MULTI_MAX], cur[FX_MULTI_MAX];
    for (int i = 0; i < n; ++i) best[i] = cur[i] = fx_splitk_rule_x6(p[i].K, cap[i]);
    if (planner_on) {
        double best_t = 1e30;
        int idx[FX_MULTI_MAX] = {0, 0, 0, 0};
        for (;;) {
            bool ok = true;
            for (int i = 0; i < n && ok; ++i) {
                cur[i] = cap[i] > 1 ? cand[idx[i]] : 1;
                ok = cur[i] <= cap[i] && (cur[i] == 1 || p[i].K / cur[i] >= 256);
            }
            if (ok) {
                int order[FX_MULTI_MAX];
                double wl[FX_MULTI_MAX];
                for (int i = 0; i < n; ++i) wl[i] = (double)fx_ceil_div(p[i].K, cur[i]);
                fx_order_desc(wl, n, order);
                double t = fx_x6_makespan(tiles, ktiles, cur, order, n);
                for (int i = 0; i < n; ++i)        // the slab reduce launches that follow (k_splitk_reduce_v4)
                    if (cur[i] > 1) t += 2.5 + (double)cur[i] * (double)p[i].M * (double)p[i].N * 4.0 / 5.0e6;
                if (t < best_t - 1e-9) {
                    best_t = t;
                    for (int i = 0; i < n; ++i) best[i] = cur[i];
                }
            }
            int i = 0;
            for (; i < n; ++i) {
                if (cap[i] > 1 && ++idx[i] < 8) break;
                idx[i] = 0;
            }
            if (i == n) break;
        }
    }
    for (int i = 0; i < n; ++i) sk_out[i] = best[i] <= cap[i] ? best[i] : cap[i];
    keys[n_next] = key;                       // (64 shape sets, oldest replaced)
    for (int i = 0; i < n; ++i) plans[n_next][i] = best[i];
    n_next = (n_next + 1) & 63;
    if (n_cached < 64) ++n_cached;
}

// Which slab rule a problem of a batch gets when it is launched on its own: the x6 rule (~1024-deep
// slabs) only if the x6 kernels will really take it — enough 128x128 tiles x slabs, a fused row sum only on a
// row-contiguous op(A); a 256x256 or 512x512 weight gradient with K = 4096 otherwise ran on the fp32 kernels'
// 64x64 tiles with 4 slabs where their own rule gives 16 (a quarter of the chip).  (Operand alignment is checked
// again in fx_gemm_f32; a misaligned problem only loses the better split.)
static bool fx_batch_wants_x6(const fx_gemm_problem& q) {
    if (!fx_gemm_x6_shape(q.M, q.N, q.K)) return false;
    if (q.epilogue && q.epilogue->rowsum && !q.transa) return false;
    const int32_t sk = fx_splitk_rule_x6(q.K, q.workspace ? q.split_k : 1);
    return fx_ceil_div(q.M, 128) * fx_ceil_div(q.N, 128) * sk >= FX_X6_MIN_WGS;
}

// The strategies of fx_gemm_f32_batch.  Each returns FX_OK with *launched = true when it took the whole
// problem list, FX_OK with *launched untouched when the list is not its case, or an error.
//
// Up to FX_MULTI_MAX problems in one grid of the split-bf16 kernels (one workgroup of 8 waves per CU, 128x128
// tiles only): any 2 .. 4 problems that all qualify, K-split or not — the tiles of the shorter problems fill
// the CUs the longest one leaves.
static int fx_batch_try_multi_x6(const fx_gemm_problem* p, int32_t n, fx_stream_t stream, bool* launched) {
    if (!fx_gemm_pair_on() || n < 2 || n > FX_MULTI_MAX || !fx_gemm_x6_enabled() || !fx_gemm_multi_mode())
        return FX_OK;
    for (int i = 0; i < n; ++i) {
        const fx_gemm_problem& q = p[i];
        if (fx_gemm_skinny(q) || !q.A || !q.B || !q.C || !fx_gemm_x6_shape(q.M, q.N, q.K)) return FX_OK;
    }
    MultiArgs ma;
    memset(&ma, 0, sizeof(ma));
    int order[FX_MULTI_MAX];
    int32_t sk[FX_MULTI_MAX];
    double wl[FX_MULTI_MAX];
    fx_x6_plan_splits(p, n, sk);
    for (int i = 0; i < n; ++i) wl[i] = (double)fx_ceil_div(p[i].K, sk[i]) + (sk[i] == 1 ? 1.0 : 0.0);
    fx_order_desc(wl, n, order);                             // longest workgroups first
    int64_t wgs = 0;
    for (int oi = 0; oi < n; ++oi) {
        const fx_gemm_problem& q = p[order[oi]];
        GemmArgs& a = ma.p[oi];
        const int rc = fx_gemm_prepare(q, sk[order[oi]], a);
        if (rc != FX_OK) return rc;
        a.tiles_m = (int32_t)fx_ceil_div(q.M, 128);
        a.tiles_n = (int32_t)fx_ceil_div(q.N, 128);
        if (!fx_gemm_pipe_ok(q.transa, q.transb, a) || !fx_gemm_tr_ok(a) || (a.epi.rowsum && !q.transa))
            return FX_OK;
        ma.cfg[oi] = (q.transa ? 0 : 1) | (q.transb ? 2 : 0);
        ma.start[oi] = (int32_t)wgs;
        wgs += (int64_t)a.tiles_m * a.tiles_n * a.split_k;
    }
    ma.start[n] = (int32_t)wgs;
    for (int oi = n + 1; oi <= FX_MULTI_MAX; ++oi) ma.start[oi] = (int32_t)wgs;
    ma.n = n;
    if (wgs < FX_X6_MIN_WGS || wgs > 0x3FFFFFFF) return FX_OK;
    hipStream_t s = fx_hip_stream(stream);
    const int rc = fx_gemm_x6_launch_multi(ma, wgs, s);
    if (rc != FX_OK) return rc;
    fx_launch_splitk_reduces(ma.p, n, s);
    FX_CHECK_LAUNCH();
    for (int oi = 0; oi < n; ++oi) fx_rec_put(order[oi], FX_GEMM_MULTI_X6, 128, 128, ma.p[oi].split_k, true);
    fx_rec.strategy = FX_GEMM_MULTI_X6;
    *launched = true;
    return FX_OK;
}

// Up to FX_MULTI_MAX problems of a backward pass as one k_gemm_f32_multi grid on 128-row tiles.
static int fx_batch_try_multi(const fx_gemm_problem* p, int32_t n, fx_stream_t stream, bool* launched) {
    if (!fx_gemm_pair_on() || n < 2 || n > FX_MULTI_MAX || !fx_gemm_multi_mode()) return FX_OK;
    // (two forward-type products — no K split anywhere — measured no better as one grid than as two
    // launches with their own tile shapes: 125 vs 122 us for DCNv2's cross + deep forward)
    bool any_split = false;
    for (int i = 0; i < n; ++i) any_split = any_split || (p[i].split_k > 1 && p[i].workspace);
    if (!any_split) return FX_OK;
    MultiShape sh[FX_MULTI_MAX];
    for (int i = 0; i < n; ++i) {
        const fx_gemm_problem& q = p[i];
        if (q.M < 64 || q.N < 16 || q.K < 64 || fx_gemm_skinny(q) || !q.A || !q.B || !q.C) return FX_OK;
        sh[i].M = q.M; sh[i].N = q.N; sh[i].K = q.K;
        sh[i].splittable = (q.split_k > 1 && q.workspace) ? q.split_k : 0;
    }
    MultiPlanItem plan[FX_MULTI_MAX];
    if (fx_multi_plan(sh, n, plan) < 512) return FX_OK;
    MultiArgs ma;
    memset(&ma, 0, sizeof(ma));
    // longest workgroups first
    int order[FX_MULTI_MAX];
    double wl[FX_MULTI_MAX];
    for (int i = 0; i < n; ++i)
        wl[i] = (double)fx_ceil_div(p[i].K, plan[i].sk) * (plan[i].tile ? 64 : 128) + (plan[i].sk == 1 ? 1.0 : 0.0);
    fx_order_desc(wl, n, order);
    int64_t wgs = 0;
    for (int oi = 0; oi < n; ++oi) {
        const fx_gemm_problem& q = p[order[oi]];
        const MultiPlanItem& pl = plan[order[oi]];
        GemmArgs& a = ma.p[oi];
        const int rc = fx_gemm_prepare(q, pl.sk, a);
        if (rc != FX_OK) return rc;
        a.tiles_m = (int32_t)fx_ceil_div(q.M, 128);
        a.tiles_n = (int32_t)fx_ceil_div(q.N, pl.tile ? 64 : 128);
        if (!fx_gemm_pipe_ok(q.transa, q.transb, a) || !fx_gemm_tr_ok(a)) return FX_OK;
        ma.cfg[oi] = (q.transa ? 0 : 1) | (q.transb ? 2 : 0) | (pl.tile ? 4 : 0);
        ma.start[oi] = (int32_t)wgs;
        wgs += (int64_t)a.tiles_m * a.tiles_n * a.split_k;
    }
    ma.start[n] = (int32_t)wgs;
    for (int oi = n + 1; oi <= FX_MULTI_MAX; ++oi) ma.start[oi] = (int32_t)wgs;
    ma.n = n;
    if (wgs <= 0 || wgs > 0x3FFFFFFF) return FX_OK;
    hipStream_t s = fx_hip_stream(stream);
    fx_gemm_tile_launch_multi(ma, wgs, s);
    FX_CHECK_LAUNCH();
    fx_launch_splitk_reduces(ma.p, n, s);
    FX_CHECK_LAUNCH();
    for (int oi = 0; oi < n; ++oi)
        fx_rec_put(order[oi], FX_GEMM_MULTI_F32, 128, (ma.cfg[oi] & 4) ? 64 : 128, ma.p[oi].split_k, true);
    fx_rec.strategy = FX_GEMM_MULTI_F32;
    *launched = true;
    return FX_OK;
}

// The dW = dZ^T X / dX = dZ W pair of a layer in one grid of 64x64 tiles (round 2's pair kernel).
static int fx_batch_try_pair_bwd(const fx_gemm_problem* p, int32_t n, fx_stream_t stream, bool* launched) {
    if (!(n == 2 && fx_gemm_pair_on() && p[0].transa && !p[0].transb && !p[1].transa && !p[1].transb))
        return FX_OK;
    GemmArgs a[2];
    for (int i = 0; i < 2; ++i) {
        const fx_gemm_problem& q = p[i];
        const int rc = fx_gemm_prepare(q, fx_gemm_skinny(q) ? q.split_k : fx_splitk_rule64(q.M, q.N, q.K, q.split_k),
                                       a[i]);
        if (rc != FX_OK) return rc;
        // (the pair kernel is the 64x64 build: force that tile whatever the single-GEMM rule says)
        a[i].tiles_m = (int32_t)fx_ceil_div(q.M, 64);
        a[i].tiles_n = (int32_t)fx_ceil_div(q.N, 64);
        if (!(q.M > 0 && q.N > 0 && !fx_gemm_skinny(q) && fx_gemm_pipe_ok(q.transa, q.transb, a[i]))) return FX_OK;
    }
    hipStream_t s = fx_hip_stream(stream);
    fx_gemm_tile_launch_pair_bwd(a[0], a[1], s);
    FX_CHECK_LAUNCH();
    for (int i = 0; i < 2; ++i)
        if (a[i].split_k > 1) {
            fx_launch_splitk_reduce(a[i], s);
            FX_CHECK_LAUNCH();
        }
    for (int i = 0; i < 2; ++i)
        fx_rec_put(i, FX_GEMM_PAIR_BWD, 64, 64, a[i].split_k, fx_gemm_tr_ok(a[0]) && fx_gemm_tr_ok(a[1]));
    fx_rec.strategy = FX_GEMM_PAIR_BWD;
    *launched = true;
    return FX_OK;
}

// The two gradients of a Linear(hidden -> 1) head in one pass over the hidden activations
// (k_head_bwd_v4).  FX_HEAD_FUSE=0: the two skinny launches.
static int fx_batch_try_head_bwd(const fx_gemm_problem* p, int32_t n, fx_stream_t stream, bool* launched) {
    static const bool head_on = fx_env_int("FX_HEAD_FUSE", 1) != 0;
    if (!(n == 2 && head_on && p[0].transa && !p[0].transb && p[0].M == 1 && p[0].workspace && p[0].split_k >= 1 &&
          !p[1].transa && !p[1].transb && p[1].K == 1 && p[1].M == p[0].K && p[1].N == p[0].N &&
          p[1].A == p[0].A && p[1].lda == p[0].lda && p[0].N >= 16 && p[0].N % 4 == 0))
        return FX_OK;
    const fx_gemm_problem& q0 = p[0];
    const fx_gemm_problem& q1 = p[1];
    const fx_gemm_epilogue* e1 = q1.epilogue;
    const bool plain = !e1 || (!e1->bias && !e1->zout && e1->act == 0 && !e1->mul && !e1->add && !e1->rowsum &&
                               (!e1->mask || (e1->mask == q0.B && e1->ldmask == q0.ldb)));
    const bool al = q0.ldb % 4 == 0 && q1.ldc % 4 == 0 &&
                    (((uintptr_t)q0.B | (uintptr_t)q0.workspace | (uintptr_t)q1.C | (uintptr_t)q1.B) & 15) == 0;
    if (!(plain && al && q0.B && q0.C && q1.B && q1.C)) return FX_OK;
    HeadBwdArgs h;
    int rc = fx_gemm_prepare(q0, q0.split_k, h.dw);
    if (rc != FX_OK) return rc;
    h.dx = q1.C;
    h.ldx = q1.ldc;
    h.w = q1.B;
    h.use_mask = (e1 && e1->mask) ? 1 : 0;
    rc = fx_head_bwd_launch(h, fx_hip_stream(stream));
    if (rc != FX_OK) return rc;
    fx_rec_put(0, FX_GEMM_HEAD_BWD, 0, 0, h.dw.split_k, false);
    fx_rec_put(1, FX_GEMM_HEAD_BWD, 0, 0, 1, false);
    fx_rec.strategy = FX_GEMM_HEAD_BWD;
    *launched = true;
    return FX_OK;
}

// Two FORWARD products (x W^T: the cross layer and the deep layer of one DCNv2 depth) in one grid of
// 64x64 tiles, the longer problem's tiles first: the 640 tiles of the 624-wide cross product leave
// 384 of the 1024 resident slots empty on their own and all reach their (four-operand) epilogue
// together; behind the deep layer's 1024 tiles they fill slots as those retire.  FX_GEMM_FWDPAIR=0:
// problem by problem.
static int fx_batch_try_pair_fwd(const fx_gemm_problem* p, int32_t n, fx_stream_t stream, bool* launched) {
    static const bool fwdpair_on = fx_env_int("FX_GEMM_FWDPAIR", 1) != 0;
    if (!(n == 2 && fx_gemm_pair_on() && fwdpair_on && !p[0].transa && p[0].transb && !p[1].transa && p[1].transb))
        return FX_OK;
    GemmArgs a[2];
    for (int i = 0; i < 2; ++i) {
        const fx_gemm_problem& q = p[i];
        if (!(q.M > 0 && q.N > 0 && !fx_gemm_skinny(q))) return FX_OK;
        const int rc = fx_gemm_prepare(q, 1, a[i]);
        if (rc != FX_OK) return rc;
        a[i].tiles_m = (int32_t)fx_ceil_div(q.M, 64);
        a[i].tiles_n = (int32_t)fx_ceil_div(q.N, 64);
        if (!(a[i].split_k == 1 && fx_gemm_pipe_ok(q.transa, q.transb, a[i]) && fx_gemm_tr_ok(a[i]))) return FX_OK;
    }
    const bool swap = (double)p[1].N * p[1].K > (double)p[0].N * p[0].K;   // more work per row first
    // (alternating the two problems' tiles in proportion to their counts instead — every CU
    // starting with a mix of long and short tiles — measured 1.490 vs 1.451 ms: worse than two
    // launches; the longer problem first it is)
    fx_gemm_tile_launch_pair_fwd(swap ? a[1] : a[0], swap ? a[0] : a[1], fx_hip_stream(stream));
    FX_CHECK_LAUNCH();
    for (int i = 0; i < 2; ++i) fx_rec_put(i, FX_GEMM_PAIR_FWD, 64, 64, 1, true);
    fx_rec.strategy = FX_GEMM_PAIR_FWD;
    fx_rec.swapped = swap ? 1 : 0;
    *launched = true;
    return FX_OK;
}

extern "C" int fx_gemm_f32_batch(const fx_gemm_problem* p, int32_t n, fx_stream_t stream) {
    FX_CHECK_ARG(n >= 0 && (n == 0 || p), "fx_gemm_f32_batch: bad problem list");
    typedef int (*fx_batch_try_fn)(const fx_gemm_problem*, int32_t, fx_stream_t, bool*);
    static const fx_batch_try_fn tries[] = {fx_batch_try_multi_x6, fx_batch_try_multi, fx_batch_try_pair_bwd,
                                            fx_batch_try_head_bwd, fx_batch_try_pair_fwd};
    fx_rec_reset(n);
    for (fx_batch_try_fn try_fn : tries) {
        bool launched = false;
        const int rc = try_fn(p, n, stream, &launched);
        if (rc != FX_OK || launched) return rc;
    }
    // problem by problem, each with the slab rule of the kernels that will take it
    fx_rec.strategy = FX_GEMM_SINGLES;
    for (int i = 0; i < n; ++i) {
        const fx_gemm_problem& q = p[i];
        fx_rec_in_batch = true;
        const int rc = fx_gemm_f32(q.transa, q.transb, q.M, q.N, q.K, q.A, q.lda, q.B, q.ldb, q.C,
                                   q.ldc, q.epilogue,
                                   fx_gemm_skinny(q) ? q.split_k
                                   : fx_batch_wants_x6(q) ? fx_splitk_rule_x6(q.K, q.workspace ? q.split_k : 1)
                                                          : fx_splitk_rule64(q.M, q.N, q.K, q.split_k),
                                   q.workspace, stream);
        fx_rec_in_batch = false;
        if (rc != FX_OK) return rc;
    }
    return FX_OK;
}
