// fx_rowopt.hip — the sparse-row optimizer: "update, or catch up, the rows of 1..4 table groups", once.
//
//   update     k_sparse_update_multi   Adam / SGD step of the unique rows of a de-dup result in every table group
//                                      that shares it (fx_sparse_adam_multi / fx_sparse_sgd_multi)
//   catch-up   k_catchup_rows          exact mode: the zero-gradient Adam steps a dense optimizer would have applied
//                                      to the listed rows since last_step (fx_adam_catchup_rows; fx_dedup_catchup of
//                                      fx_fused.hip launches it through fx_catchup_rows_launch)
//              k_catchup_all           the same for every row of one table: the flush (fx_adam_catchup_all)
//   fetch      k_owner_fetch_rows      owner side of the row-sharded forward: catch-up + gather into the send block
//   regularizer k_reg_stats / k_reg_cross / k_reg_dense   the dense embedding-regularizer term
//
// Tables are fp32 or bf16, packed or fields of a row record (fx_row_state).
//
// What this replaces in the reference (paths relative to the reference checkout):
//   torch.optim.Adam / SGD step over every table row          rank_model.py:322, torch_utils.py:76
//   the embedding regularizer                                 rank_model.py:95-112
#include "fx_common.h"


// ---------------------------------------------------------------------------------------------
// shared device pieces
// ---------------------------------------------------------------------------------------------
struct FxTableDev {
    void* table;           // fp32, or bf16 when `bf16` is set (moments / gradients are always fp32)
    float* m;
    float* v;
    int32_t* last_step;
    const float* G;        // update kernels only
    int32_t D, vec, lanes_log2, bf16;
    int64_t tld, mld, vld, lld;   // row strides of table / m / v (elements) and of last_step (ints): D, D, D, 1 for
                                  // packed arrays; all = W when the four point into one row record (round 6)
};

// d/dp of (l1 * |p| + l2/2 * p^2): the embedding regularizer of rank_model.py:106-112
__device__ __forceinline__ float fx_reg_grad(float p, float l1, float l2) {
    float r = l2 * p;
    if (l1 != 0.f) r += p > 0.f ? l1 : (p < 0.f ? -l1 : 0.f);
    return r;
}

// zero-gradient Adam replay of one row (fx_adam_replay, fx_common.h), in two halves so that a lane group can
// issue the loads of EVERY table group before it waits for any of them: the rows live in multi-GB
// tables, every access is a TLB miss + an HBM access (~8 us per dependent round trip measured: the
// chain last_step -> m,v -> p costs 25 us for 25 K rows), so the state of a row —
// last_step, m, v AND p, of the D-float table and of the D=1 table — is requested in one go.
template <int VEC>
struct FxRowRegs {
    float p[VEC], m[VEC], v[VEC];
    int last;
    bool on;       // this lane holds elements of the row
    bool act;      // this lane takes part at all (sub < lanes of the table)
};

template <int VEC, bool WANT_LAST = true>
__device__ __forceinline__ void fx_row_load(const FxTableDev& t, int64_t row, int sub,
                                            FxRowRegs<VEC>& r) {
    const int lanes = 1 << t.lanes_log2;
    r.act = sub < lanes;
    const int d0 = sub * VEC;
    r.on = r.act && d0 < t.D;
    r.last = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) r.p[k] = r.m[k] = r.v[k] = 0.f;
    if (WANT_LAST && r.act) r.last = t.last_step[row * t.lld];
    if (r.on) {
        fx_load<VEC>(t.m + row * t.mld + d0, r.m);
        fx_load<VEC>(t.v + row * t.vld + d0, r.v);
        fx_tab_load<VEC>(t.table, t.bf16, row * t.tld + d0, r.p);
    }
}

template <int VEC>
__device__ __forceinline__ void fx_catchup_finish(const FxTableDev& t, int64_t row, int sub,
                                                  FxRowRegs<VEC>& r, const fx_scalars& sc, int upto,
                                                  const FxLogs& lg, const FxSeries& ser) {
    if (!r.act) return;
    const int last = r.last;
    const int k_steps = upto - last;
    if (k_steps <= 0) return;
    if (r.on) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < VEC; ++k) any = any || (r.m[k] != 0.f) || (r.v[k] != 0.f);
        if (any) {
            fx_adam_replay<VEC>(r.p, r.m, r.v, last, k_steps, sc, lg, ser);
            fx_tab_store<VEC>(t.table, t.bf16, row * t.tld + sub * VEC, r.p);
            fx_store<VEC>(t.m + row * t.mld + sub * VEC, r.m);
            fx_store<VEC>(t.v + row * t.vld + sub * VEC, r.v);
        }
    }
    if (sub == 0) t.last_step[row * t.lld] = upto;
}

template <int VEC>
__device__ __forceinline__ void fx_catchup_row(const FxTableDev& t, int64_t row, int sub,
                                               const fx_scalars& sc, int upto, const FxLogs& lg,
                                               const FxSeries& ser) {
    FxRowRegs<VEC> r;
    fx_row_load<VEC>(t, row, sub, r);
    fx_catchup_finish<VEC>(t, row, sub, r, sc, upto, lg, ser);
}

// ---------------------------------------------------------------------------------------------
// The DeepFM / xDeepFM shape of the catch-up — a 16-float row (4 lanes x 4 floats) and the D = 1 row of
// LogisticRegression under the same id — as ONE replay by the row's quad of lanes (round 5).
//
// Step i after `last` moves an element by  u_i = lr/(1-b1^(t+i)) . m b1^i / (sqrt(v) b2^(i/2) / sqrt(1-b2^(t+i)) + eps)
// (fx_adam_replay).  Factored:  u_i = (lr m / sqrt(v)) . w_i / (g_i + eps / sqrt(v))  with
//     w_i = b1^i / (1 - b1^(t+i)),   g_i = b2^(i/2) / sqrt(1 - b2^(t+i))
// the same for every element of the row: an element costs  acc += w_i . rcp(g_i + c)  per step (3 instructions,
// fx_adam_replay: 6), the sum is applied to p once.  (w_i, g_i) cost 10 instructions with two
// transcendentals: lane s of the quad computes them for step 4q + s + 1 of round q and the quad reads each
// other's pair through DPP quad broadcasts — 2.5 + 2 instructions a step instead of 10 on every lane.  The D = 1
// row rides as a fifth element (lane 0; zeros elsewhere) instead of a second pass with a quarter of the
// lanes.  19.75 instructions per step where the two passes of fx_adam_replay issued ~49 (k_catchup_rows
// is VALU-bound: a wave runs as long as its coldest row).
// The terms shrink by >= 5 % a step (b1 / sqrt(b2) over the ratio of the bias corrections), so once a
// step's terms are below 2^-29 of every sum of the quad the rest cannot change them in fp32: the quad is
// done; the wave leaves when all its quads are (no lane leaves the loop alone: there is no divergence).
// Against the reference's step-by-step `p -= u_i` this sums the same terms in the same order in fp32 and
// rounds p once instead of k times; what it drops is below 2^-29 of the move (tests: exact mode == dense
// torch Adam stepped k times).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float fx_quad_bcast(float x, int u) {      // lane u of this lane's quad
    const int v = __float_as_int(x);
    int r;
    switch (u) {
        case 0: r = __builtin_amdgcn_mov_dpp(v, 0x00, 0xF, 0xF, true); break;      // quad_perm [0,0,0,0]
        case 1: r = __builtin_amdgcn_mov_dpp(v, 0x55, 0xF, 0xF, true); break;
        case 2: r = __builtin_amdgcn_mov_dpp(v, 0xAA, 0xF, 0xF, true); break;
        default: r = __builtin_amdgcn_mov_dpp(v, 0xFF, 0xF, 0xF, true); break;
    }
    return __int_as_float(r);
}

__device__ __forceinline__ bool fx_quad_any(bool x) {
    const unsigned long long b = __ballot(x);
    const int q4 = (threadIdx.x & 63) & ~3;
    return ((b >> q4) & 0xFull) != 0ull;
}

// LR = false: the D = 16 table alone (DCNv2, DLRM, ...: models without a first-order term).
// r0 / r1 leave with the row as it stands after the catch-up (the owner fetch of the row-sharded path sends it
// from there: one code path, one rounding, for 1 rank and for N).
template <bool LR>
__device__ __forceinline__ void fx_catchup_quad(const FxTableDev& t0, const FxTableDev& t1, int64_t row, int sub,
                                                const fx_scalars& sc, int upto, const FxLogs& lg,
                                                const FxSeries& ser, FxRowRegs<4>& r0, FxRowRegs<1>& r1) {
    fx_row_load<4, false>(t0, row, sub, r0);
    if constexpr (LR) fx_row_load<1, false>(t1, row, sub, r1);
    else { r1.p[0] = r1.m[0] = r1.v[0] = 0.f; r1.on = r1.act = false; r1.last = 0; }
    const int last = t0.last_step[row * t0.lld];      // (same address in the four lanes: one access)
    const int last1 = LR ? t1.last_step[row * t1.lld] : last;
    const int k0 = upto - last, k1 = upto - last1;
    if (last1 != last) {
        // the two tables were not touched together (cannot happen under one id plan): the plain replays
        r0.last = last; r1.last = last1;
        fx_catchup_finish<4>(t0, row, sub, r0, sc, upto, lg, ser);
        fx_catchup_finish<1>(t1, row, sub, r1, sc, upto, lg, ser);
        return;
    }
    if (k0 <= 0) return;                               // (the whole quad: `last` is the row's)
    (void)k1;
    // this lane's five elements: 4 of the D-float row + the D = 1 row (lane 0)
    float pe[5], me[5], ve[5];
#pragma unroll
    for (int e = 0; e < 4; ++e) { pe[e] = r0.p[e]; me[e] = r0.m[e]; ve[e] = r0.v[e]; }
    pe[4] = r1.p[0]; me[4] = r1.m[0]; ve[4] = r1.v[0];
    bool any_state = false, moving = false;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        any_state |= (me[e] != 0.f) || (ve[e] != 0.f);
        moving |= (me[e] != 0.f);
    }
    const int kk = k0 < FX_REPLAY_MAX ? k0 : FX_REPLAY_MAX;
    if (ser.tab != nullptr && k0 > FX_SERIES_KDIR) {
        // (round 6) the sum of the missed steps from the series table: no step loop (fx_common.h)
        if (moving) fx_series_move<5>(pe, me, ve, last, k0, sc, ser, lg);
    } else if (fx_quad_any(moving)) {
        float c[5], sc_e[5], acc[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            const float r = sqrtf(ve[e]);
            const bool live = (me[e] != 0.f) && (r > 0.f);
            const float inv = live ? 1.f / r : 0.f;
            c[e] = live ? sc.eps * inv : 1.f;          // (a dead element: acc grows harmlessly, scale 0)
            sc_e[e] = sc.lr * me[e] * inv;
            acc[e] = 0.f;
        }
        // lane `sub` owns the steps 4 q + sub + 1
        const float b1 = sc.beta1, b2 = sc.beta2, sb2 = sqrtf(sc.beta2);
        const float b1_2 = b1 * b1, b2_2 = b2 * b2, sb2_2 = sb2 * sb2;
        const float b1_4 = b1_2 * b1_2, b2_4 = b2_2 * b2_2, sb2_4 = sb2_2 * sb2_2;
        float bi = sub == 0 ? b1 : sub == 1 ? b1_2 : sub == 2 ? b1_2 * b1 : b1_4;          // b1^(sub+1)
        float sb = sub == 0 ? sb2 : sub == 1 ? sb2_2 : sub == 2 ? sb2_2 * sb2 : sb2_4;
        // the bias corrections as d = 1 - b^(t+i), advanced by d' = (1 - b^4) + b^4 d (round 6: 1 - b2^t is
        // 0.001 t early in a run; b2^t rounded to fp32 first left it with a relative error of 3e-5 / t)
        // (lc*: torch's python-side doubles — fx_beta_f64)
        float d1 = (float)(1.0 - exp2(lg.lc1 * (double)(last + sub + 1)));
        float d2 = (float)(1.0 - exp2(lg.lc2 * (double)(last + sub + 1)));
        const float e1_4 = (float)(1.0 - exp2(4.0 * lg.lc1)), e2_4 = (float)(1.0 - exp2(4.0 * lg.lc2));
        const int nr = (kk + 3) >> 2;
        for (int q = 0; q < nr; ++q) {
            const int i = 4 * q + sub + 1;
            float w = bi * __builtin_amdgcn_rcpf(d1);
            const float g = sb * __builtin_amdgcn_rsqf(d2);
            w = i <= kk ? w : 0.f;
            bi *= b1_4; sb *= sb2_4;
            d1 = fmaf(b1_4, d1, e1_4); d2 = fmaf(b2_4, d2, e2_4);
            float term[5];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float wu = fx_quad_bcast(w, u), gu = fx_quad_bcast(g, u);
#pragma unroll
                for (int e = 0; e < 5; ++e) {
                    term[e] = wu * __builtin_amdgcn_rcpf(gu + c[e]);
                    acc[e] += term[e];
                }
            }
            // (term[] = the round's last step.)  Done when it can no longer change any live sum of the quad.
            bool small = true;
#pragma unroll
            for (int e = 0; e < 5; ++e) small &= (sc_e[e] == 0.f) || (term[e] <= acc[e] * 1.862645e-9f);   // 2^-29
            // (quads that have counted all their steps have left the loop and do not vote; the ones still
            // here leave together)
            if (__all(!fx_quad_any(!small))) break;
        }
#pragma unroll
        for (int e = 0; e < 5; ++e) pe[e] = fmaf(-sc_e[e], acc[e], pe[e]);
    }
    // the decay of the moments over ALL missed steps, in closed form
    if (any_state) {
        const float f1 = (float)exp2(lg.lb1 * (double)k0), f2 = (float)exp2(lg.lb2 * (double)k0);
#pragma unroll
        for (int e = 0; e < 5; ++e) { me[e] *= f1; ve[e] *= f2; }
    }
    if (r0.on) {
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) any |= (r0.m[e] != 0.f) || (r0.v[e] != 0.f);
        if (any) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { r0.p[e] = pe[e]; r0.m[e] = me[e]; r0.v[e] = ve[e]; }
            fx_tab_store<4>(t0.table, t0.bf16, row * t0.tld + sub * 4, r0.p);
            fx_store<4>(t0.m + row * t0.mld + sub * 4, r0.m);
            fx_store<4>(t0.v + row * t0.vld + sub * 4, r0.v);
        }
    }
    if (r1.on && ((r1.m[0] != 0.f) || (r1.v[0] != 0.f))) {
        r1.p[0] = pe[4]; r1.m[0] = me[4]; r1.v[0] = ve[4];
        fx_tab_store<1>(t1.table, t1.bf16, row * t1.tld, r1.p);
        fx_store<1>(t1.m + row * t1.mld, r1.m);
        fx_store<1>(t1.v + row * t1.vld, r1.v);
    }
    if (sub == 0) {
        t0.last_step[row * t0.lld] = upto;
        if constexpr (LR) t1.last_step[row * t1.lld] = upto;
    }
}

// FX_CATCHUP_QUAD=0: the two plain replays (A/B runs)
static const bool fx_catchup_quad_on = fx_env_int("FX_CATCHUP_QUAD", 1) != 0;

// one unique row of a de-dup result, in every table group that shares the id plan
__device__ __forceinline__ void fx_catchup_tables(const FxTableDev* t, int n_tables, int64_t row,
                                                  int sub, const fx_scalars& sc, int upto, const FxLogs& lg,
                                                  const FxSeries& ser) {
    if (n_tables == 2 && t[0].vec == 4 && t[1].vec == 1) {
        // the D-float tables + the D=1 tables of LogisticRegression: all eight loads in flight
        FxRowRegs<4> r0;
        FxRowRegs<1> r1;
        fx_row_load<4>(t[0], row, sub, r0);
        fx_row_load<1>(t[1], row, sub, r1);
        fx_catchup_finish<4>(t[0], row, sub, r0, sc, upto, lg, ser);
        fx_catchup_finish<1>(t[1], row, sub, r1, sc, upto, lg, ser);
        return;
    }
    for (int i = 0; i < n_tables; ++i) {
        const FxTableDev& tb = t[i];
        if (tb.vec == 4) fx_catchup_row<4>(tb, row, sub, sc, upto, lg, ser);
        else if (tb.vec == 2) fx_catchup_row<2>(tb, row, sub, sc, upto, lg, ser);
        else fx_catchup_row<1>(tb, row, sub, sc, upto, lg, ser);
    }
}

// ---------------------------------------------------------------------------------------------
// host side: fx_row_state -> FxTableDev
// ---------------------------------------------------------------------------------------------
// group_log2: the lane group of a row = the widest table's lanes, up to 256 (D = 255: one row per workgroup).
// No launch of this file keeps a narrower limit of its own: the per-table branches (fx_update_row,
// fx_catchup_row, fx_owner_one) never talk across lanes, and the one that does — the quad replay, DPP and
// ballots inside a quad — is only chosen for group_log2 == 2 (fx_quad_mode).
static int fx_fill_tables(const fx_row_state* tables_host, int32_t n_tables, FxTableDev* out,
                          int* group_log2, const char* who, bool need_state) {
    int gl = 0;
    for (int t = 0; t < n_tables; ++t) {
        const fx_row_state& h = tables_host[t];
        if (h.D < 1 || h.D > 256) {
            fx_set_error("%s: table %d has D=%d outside [1,256]", who, t, h.D);
            return FX_ERR_INVALID;
        }
        if (!h.table || (need_state && (!h.m || !h.v || !h.last_step))) {
            fx_set_error("%s: table %d has a null pointer", who, t);
            return FX_ERR_INVALID;
        }
        const FxRowGeom g = fx_row_geom(h.D);
        int ll = 0;
        while ((1 << ll) < g.lanes) ++ll;
        out[t].table = h.table;
        out[t].m = h.m;
        out[t].v = h.v;
        out[t].last_step = h.last_step;
        out[t].G = h.G;
        out[t].D = h.D;
        out[t].tld = h.table_ld > 0 ? h.table_ld : h.D;
        out[t].mld = h.m_ld > 0 ? h.m_ld : h.D;
        out[t].vld = h.v_ld > 0 ? h.v_ld : h.D;
        out[t].lld = h.last_ld > 0 ? h.last_ld : 1;
        if (out[t].tld < h.D || out[t].mld < h.D || out[t].vld < h.D) {
            fx_set_error("%s: table %d has a row stride below D", who, t);
            return FX_ERR_INVALID;
        }
        out[t].bf16 = h.table_dtype == FX_BF16 ? 1 : 0;
        if (h.table_dtype != FX_F32 && h.table_dtype != FX_BF16) {
            fx_set_error("%s: table %d has table_dtype %d (FX_F32 or FX_BF16)", who, t, h.table_dtype);
            return FX_ERR_INVALID;
        }
        out[t].vec = g.vec;
        out[t].lanes_log2 = ll;
        if (ll > gl) gl = ll;
        // every lane moves `vec` elements of a field in one access (float4 / float2, uint2 / uint32 of a bf16
        // table) at row * ld + sub * vec: the field's base and its row stride must be whole multiples of that
        const struct { const char* name; const void* p; int64_t ld; int eb; } fields[4] = {
            {"table", h.table, out[t].tld, out[t].bf16 ? 2 : 4}, {"m", h.m, out[t].mld, 4},
            {"v", h.v, out[t].vld, 4}, {"G", h.G, h.D, 4}};
        for (const auto& f : fields) {
            if (f.p == nullptr) continue;
            if (reinterpret_cast<uintptr_t>(f.p) % (uintptr_t)(g.vec * f.eb) != 0 || f.ld % g.vec != 0) {
                fx_set_error("%s: table %d field %s (D=%d) is not aligned for %d-element accesses: the pointer "
                             "must be a multiple of %d bytes and the row stride %lld a multiple of %d",
                             who, t, f.name, h.D, g.vec, g.vec * f.eb, (long long)f.ld, g.vec);
                return FX_ERR_INVALID;
            }
        }
    }
    *group_log2 = gl;
    return FX_OK;
}

// the argument errors fx_fill_tables finds, for a caller that launches other work first (fx_dedup_catchup)
int fx_catchup_rows_check(const fx_row_state* tables_host, int32_t n_tables, const char* who) {
    FxTableDev t[FX_MAX_TABLES];
    int gl = 0;
    return fx_fill_tables(tables_host, n_tables, t, &gl, who, true);
}

// which form of fx_catchup_quad a catch-up of these tables takes: 1 the D = 16 + D = 1 pair, 2 a D = 16 table
// alone, 0 the plain replays
static int fx_quad_mode(const FxTableDev* t, int n_tables, int gl) {
    if (!fx_catchup_quad_on || gl != 2 || t[0].vec != 4 || t[0].D != 16) return 0;
    if (n_tables == 2 && t[1].vec == 1 && t[1].D == 1) return 1;
    return n_tables == 1 ? 2 : 0;
}

// ---------------------------------------------------------------------------------------------
// fx_sparse_adam_multi / fx_sparse_sgd_multi: the row update of every table group that shares one
// de-dup result (same uniq_row), one launch.
// ---------------------------------------------------------------------------------------------
struct MultiOptArgs {
    FxTableDev t[FX_MAX_TABLES];
    const uint32_t* uniq_row;
    const int32_t* n_unique;
    const fx_scalars* scal;
    int32_t n_tables, group_log2;
};

// g += r(p) under a regularizer, then one Adam step of a lane's elements
template <int VEC>
__device__ __forceinline__ void fx_add_reg(float (&g)[VEC], const float (&p)[VEC], const fx_scalars& sc) {
    if (sc.reg_l1 == 0.f && sc.reg_l2 == 0.f) return;
#pragma unroll
    for (int k = 0; k < VEC; ++k) g[k] += fx_reg_grad(p[k], sc.reg_l1, sc.reg_l2);
}

template <int VEC>
__device__ __forceinline__ void fx_adam_vec(float (&p)[VEC], float (&m)[VEC], float (&v)[VEC],
                                            const float (&g)[VEC], const fx_scalars& sc) {
    const float w1 = fx_one_minus(sc.beta1), w2 = fx_one_minus(sc.beta2);   // torch's float(1 - beta)
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        fx_adam_elem(p[k], m[k], v[k], g[k] * sc.clip_coef, w1, sc.beta2, w2, sc.bc2_sqrt, sc.eps,
                     sc.step_size);
}

template <int VEC, bool ADAM>
__device__ __forceinline__ void fx_update_row(const FxTableDev& t, int64_t u, int64_t row, int sub,
                                              const fx_scalars& sc) {
    const int lanes = 1 << t.lanes_log2;
    if (sub >= lanes) return;
    const int d0 = sub * VEC;
    if (d0 < t.D) {
        float p[VEC], g[VEC];
        const int64_t o = row * t.tld + d0;
        fx_tab_load<VEC>(t.table, t.bf16, o, p);
        fx_load<VEC>(t.G + u * t.D + d0, g);
        fx_add_reg<VEC>(g, p, sc);
        if constexpr (ADAM) {
            float m[VEC], v[VEC];
            const int64_t om = row * t.mld + d0, ov = row * t.vld + d0;
            fx_load<VEC>(t.m + om, m);
            fx_load<VEC>(t.v + ov, v);
            fx_adam_vec<VEC>(p, m, v, g, sc);
            fx_store<VEC>(t.m + om, m);
            fx_store<VEC>(t.v + ov, v);
        } else {
            const float scale = sc.lr * sc.clip_coef;
#pragma unroll
            for (int k = 0; k < VEC; ++k) p[k] = p[k] - scale * g[k];
        }
        fx_tab_store<VEC>(t.table, t.bf16, o, p);
    }
    if (sub == 0 && t.last_step) t.last_step[row * t.lld] = sc.step;
}

// the Adam half of fx_update_row on registers that are already loaded
template <int VEC>
__device__ __forceinline__ void fx_adam_finish(const FxTableDev& t, int64_t row, int sub,
                                               FxRowRegs<VEC>& r, float (&g)[VEC],
                                               const fx_scalars& sc) {
    if (!r.act) return;
    if (r.on) {
        fx_add_reg<VEC>(g, r.p, sc);
        fx_adam_vec<VEC>(r.p, r.m, r.v, g, sc);
        fx_tab_store<VEC>(t.table, t.bf16, row * t.tld + sub * VEC, r.p);
        fx_store<VEC>(t.m + row * t.mld + sub * VEC, r.m);
        fx_store<VEC>(t.v + row * t.vld + sub * VEC, r.v);
    }
    if (sub == 0 && t.last_step) t.last_step[row * t.lld] = sc.step;
}

template <bool ADAM>
__global__ __launch_bounds__(256) void k_sparse_update_multi(MultiOptArgs a) {
    const int glanes = 1 << a.group_log2;
    const int sub = threadIdx.x & (glanes - 1);
    const int64_t rpb = 256 >> a.group_log2;
    const int nu = *a.n_unique;
    const fx_scalars sc = *a.scal;
    for (int64_t u = (int64_t)blockIdx.x * rpb + (threadIdx.x >> a.group_log2); u < nu;
         u += (int64_t)gridDim.x * rpb) {
        const int64_t row = a.uniq_row[u];
        if (ADAM && a.n_tables == 2 && a.t[0].vec == 4 && a.t[1].vec == 1) {
            FxRowRegs<4> r0;
            FxRowRegs<1> r1;
            float g0[4] = {0.f, 0.f, 0.f, 0.f}, g1[1] = {0.f};
            fx_row_load<4, false>(a.t[0], row, sub, r0);
            fx_row_load<1, false>(a.t[1], row, sub, r1);
            if (r0.on) fx_load<4>(a.t[0].G + u * a.t[0].D + sub * 4, g0);
            if (r1.on) fx_load<1>(a.t[1].G + u * a.t[1].D + sub, g1);
            fx_adam_finish<4>(a.t[0], row, sub, r0, g0, sc);
            fx_adam_finish<1>(a.t[1], row, sub, r1, g1, sc);
            continue;
        }
        for (int t = 0; t < a.n_tables; ++t) {
            const FxTableDev& tb = a.t[t];
            if (tb.vec == 4) fx_update_row<4, ADAM>(tb, u, row, sub, sc);
            else if (tb.vec == 2) fx_update_row<2, ADAM>(tb, u, row, sub, sc);
            else fx_update_row<1, ADAM>(tb, u, row, sub, sc);
        }
    }
}

static int fx_sparse_update_multi(bool adam, const fx_row_state* tables_host, int32_t n_tables,
                                  const uint32_t* uniq_row, const int32_t* n_unique, int64_t n_max,
                                  const fx_scalars* scal, fx_stream_t stream, const char* who) {
    FX_CHECK_ARG(n_tables >= 1 && n_tables <= FX_MAX_TABLES, "%s: n_tables=%d not in [1,%d]", who,
                 n_tables, FX_MAX_TABLES);
    if (n_max <= 0) return FX_OK;
    FX_CHECK_ARG(tables_host && uniq_row && n_unique && scal, "%s: null pointer", who);
    MultiOptArgs a;
    memset(&a, 0, sizeof(a));
    int gl = 0;
    const int st = fx_fill_tables(tables_host, n_tables, a.t, &gl, who, false);
    if (st != FX_OK) return st;
    for (int t = 0; t < n_tables; ++t) {
        FX_CHECK_ARG(a.t[t].G != nullptr, "%s: table %d has no gradient", who, t);
        FX_CHECK_ARG(!adam || (a.t[t].m && a.t[t].v), "%s: table %d has no Adam moments", who, t);
    }
    a.uniq_row = uniq_row;
    a.n_unique = n_unique;
    a.scal = scal;
    a.n_tables = n_tables;
    a.group_log2 = gl;
    int64_t blocks = fx_ceil_div(n_max, 256 >> gl);
    if (blocks > 256 * 64) blocks = 256 * 64;
    dim3 grid((unsigned)blocks);
    hipStream_t s = fx_hip_stream(stream);
    if (adam) hipLaunchKernelGGL(k_sparse_update_multi<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_sparse_update_multi<false>, grid, dim3(256), 0, s, a);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_sparse_adam_multi(const fx_row_state* tables_host, int32_t n_tables,
                                    const uint32_t* uniq_row, const int32_t* n_unique,
                                    int64_t n_max, const fx_scalars* scal, fx_stream_t stream) {
    return fx_sparse_update_multi(true, tables_host, n_tables, uniq_row, n_unique, n_max, scal,
                                  stream, "fx_sparse_adam_multi");
}

extern "C" int fx_sparse_sgd_multi(const fx_row_state* tables_host, int32_t n_tables,
                                   const uint32_t* uniq_row, const int32_t* n_unique, int64_t n_max,
                                   const fx_scalars* scal, fx_stream_t stream) {
    return fx_sparse_update_multi(false, tables_host, n_tables, uniq_row, n_unique, n_max, scal,
                                  stream, "fx_sparse_sgd_multi");
}

// ---------------------------------------------------------------------------------------------
// fx_adam_catchup_all: flush of the exact mode for fp32 or bf16 tables — every row of the table is
// brought up to step + upto_offset (before evaluate / save / a learning-rate change).
// ---------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void k_catchup_all(FxTableDev t, int64_t total_rows,
                                                     const fx_scalars* scal, int upto_offset) {
    const int lanes = 1 << t.lanes_log2;
    const int sub = threadIdx.x & (lanes - 1);
    const int64_t rpb = 256 >> t.lanes_log2;
    const fx_scalars sc = *scal;
    const int upto = sc.step + upto_offset;
    const FxLogs lg = fx_logs_of(sc);
    const FxSeries ser = fx_series_of(scal, sc);
    for (int64_t row = (int64_t)blockIdx.x * rpb + (threadIdx.x >> t.lanes_log2); row < total_rows;
         row += (int64_t)gridDim.x * rpb) {
        if (t.last_step[row * t.lld] >= upto) continue;
        fx_catchup_row<VEC>(t, row, sub, sc, upto, lg, ser);
    }
}

static int fx_catchup_all_launch(const fx_row_state* table_host, int64_t total_rows, int32_t upto_offset,
                                 const fx_scalars* scal, const char* who, hipStream_t s) {
    FX_CHECK_ARG(table_host && scal, "%s: null pointer", who);
    if (total_rows <= 0) return FX_OK;
    FxTableDev t;
    int gl = 0;
    const int st = fx_fill_tables(table_host, 1, &t, &gl, who, true);
    if (st != FX_OK) return st;
    int64_t blocks = fx_ceil_div(total_rows, 256 >> t.lanes_log2);
    if (blocks > 256 * 64) blocks = 256 * 64;
    dim3 grid((unsigned)blocks);
    if (t.vec == 4) hipLaunchKernelGGL(k_catchup_all<4>, grid, dim3(256), 0, s, t, total_rows, scal, (int)upto_offset);
    else if (t.vec == 2) hipLaunchKernelGGL(k_catchup_all<2>, grid, dim3(256), 0, s, t, total_rows, scal, (int)upto_offset);
    else hipLaunchKernelGGL(k_catchup_all<1>, grid, dim3(256), 0, s, t, total_rows, scal, (int)upto_offset);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_adam_catchup_all(const fx_row_state* table_host, int64_t total_rows,
                                   int32_t upto_offset, const fx_scalars* scal,
                                   fx_stream_t stream) {
    return fx_catchup_all_launch(table_host, total_rows, upto_offset, scal, "fx_adam_catchup_all",
                                 fx_hip_stream(stream));
}

// ---------------------------------------------------------------------------------------------
// fx_adam_catchup_rows: the exact-mode catch-up of the unique rows of ANY de-dup result (the generic
// sort path: sequence columns that alias a table, batches beyond the column fast path), for fp32 or
// bf16 tables, every table group that shares the id plan in ONE launch.
// ---------------------------------------------------------------------------------------------
struct CatchRowsArgs {
    FxTableDev t[FX_MAX_TABLES];
    const uint32_t* uniq_row;
    const int32_t* n_unique;
    const fx_scalars* scal;
    int32_t n_tables, group_log2, upto_offset, quad;
};

__global__ __launch_bounds__(256) void k_catchup_rows(CatchRowsArgs a) {
    const int glanes = 1 << a.group_log2;
    const int sub = threadIdx.x & (glanes - 1);
    const int64_t rpb = 256 >> a.group_log2;
    const int nu = *a.n_unique;
    const fx_scalars sc = *a.scal;
    const int upto = sc.step + a.upto_offset;
    const FxLogs lg = fx_logs_of(sc);
    const FxSeries ser = fx_series_of(a.scal, sc);
    if (a.quad) {
        FxRowRegs<4> r0;
        FxRowRegs<1> r1;
        // (the votes inside fx_catchup_quad run over the lanes that are in it: quads past the end of the list
        // simply are not)
        if (a.quad == 1)
            for (int64_t u = (int64_t)blockIdx.x * rpb + (threadIdx.x >> 2); u < nu; u += (int64_t)gridDim.x * rpb)
                fx_catchup_quad<true>(a.t[0], a.t[1], (int64_t)a.uniq_row[u], sub, sc, upto, lg, ser, r0, r1);
        else
            for (int64_t u = (int64_t)blockIdx.x * rpb + (threadIdx.x >> 2); u < nu; u += (int64_t)gridDim.x * rpb)
                fx_catchup_quad<false>(a.t[0], a.t[0], (int64_t)a.uniq_row[u], sub, sc, upto, lg, ser, r0, r1);
        return;
    }
    for (int64_t u = (int64_t)blockIdx.x * rpb + (threadIdx.x >> a.group_log2); u < nu;
         u += (int64_t)gridDim.x * rpb)
        fx_catchup_tables(a.t, a.n_tables, (int64_t)a.uniq_row[u], sub, sc, upto, lg, ser);
}

// the one launch of k_catchup_rows (declared in fx_common.h: fx_dedup_catchup of fx_fused.hip ends with it)
int fx_catchup_rows_launch(const fx_row_state* tables_host, int32_t n_tables, const uint32_t* uniq_row,
                           const int32_t* n_unique, int64_t n_max, int32_t upto_offset,
                           const fx_scalars* scal, const char* who, hipStream_t s) {
    CatchRowsArgs a;
    memset(&a, 0, sizeof(a));
    int gl = 0;
    const int st = fx_fill_tables(tables_host, n_tables, a.t, &gl, who, true);
    if (st != FX_OK) return st;
    a.uniq_row = uniq_row;
    a.n_unique = n_unique;
    a.scal = scal;
    a.n_tables = n_tables;
    a.group_log2 = gl;
    a.upto_offset = upto_offset;
    a.quad = fx_quad_mode(a.t, n_tables, gl);
    int64_t blocks = fx_ceil_div(n_max, 256 >> gl);
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(k_catchup_rows, dim3((unsigned)blocks), dim3(256), 0, s, a);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

extern "C" int fx_adam_catchup_rows(const fx_row_state* tables_host, int32_t n_tables,
                                    const uint32_t* uniq_row, const int32_t* n_unique,
                                    int64_t n_max, int32_t upto_offset, const fx_scalars* scal,
                                    fx_stream_t stream) {
    FX_CHECK_ARG(n_tables >= 1 && n_tables <= FX_MAX_TABLES,
                 "fx_adam_catchup_rows: n_tables=%d not in [1,%d]", n_tables, FX_MAX_TABLES);
    if (n_max <= 0) return FX_OK;
    FX_CHECK_ARG(tables_host && uniq_row && n_unique && scal, "fx_adam_catchup_rows: null pointer");
    return fx_catchup_rows_launch(tables_host, n_tables, uniq_row, n_unique, n_max, upto_offset, scal,
                                  "fx_adam_catchup_rows", fx_hip_stream(stream));
}

// ---------------------------------------------------------------------------------------------
// fx_owner_fetch_rows: owner side of the row-sharded forward, ONE launch for every table group of the
// exchange (round 2: a catch-up launch + a gather launch per group).  A lane group owns one unique
// owned row of the de-dup of what the peers asked for: it brings the row up to date (exact mode: the
// zero-gradient Adam replay of fx_adam_catchup_rows, `catchup` != 0) and writes the row into the send
// block at EVERY position that asked for it (sorted_pos of its run: one entry per requesting rank), each
// group in its own columns [off_t, off_t + D_t) of the [n_total, ld] block; pad columns and the
// entries that asked for nothing (pad ids: the tail of the sorted array) are zeroed.  The rows are read
// once — the round-2 sequence read them in the catch-up and again in the gather.
// ---------------------------------------------------------------------------------------------
struct OwnerFetchArgs {
    FxTableDev t[FX_MAX_TABLES];
    int32_t off[FX_MAX_TABLES];
    const uint32_t* uniq_row;
    const uint32_t* seg_start;
    const uint32_t* sorted_pos;
    const int32_t* n_unique;
    float* send;
    int64_t ld, n_total;
    const fx_scalars* scal;
    float* zero_row;             // zero_w floats cleared on the way (pad row of the block the rows land in)
    int32_t n_tables, group_log2, upto_offset, catchup, used_w, zero_w, quad;
};

template <int VEC>
__device__ __forceinline__ void fx_owner_put(const OwnerFetchArgs& a, int ti, const FxRowRegs<VEC>& r,
                                             int sub, uint32_t beg, uint32_t end) {
    if (!r.on) return;
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        // a bf16 table holds the ROUNDED row: that is what an unsharded gather would read back after the
        // catch-up stored it, so that is what travels (the registers still hold the unrounded fp32 result)
        v[k] = a.t[ti].bf16 ? fx_bf16_to_f32(fx_f32_to_bf16(r.p[k])) : r.p[k];
    for (uint32_t i = beg; i < end; ++i)
        fx_store<VEC>(a.send + (int64_t)a.sorted_pos[i] * a.ld + a.off[ti] + sub * VEC, v);
}

template <int VEC>
__device__ __forceinline__ void fx_owner_one(const OwnerFetchArgs& a, int ti, int64_t row, int sub,
                                             const fx_scalars& sc, int upto, const FxLogs& lg,
                                             const FxSeries& ser, uint32_t beg, uint32_t end) {
    FxRowRegs<VEC> r;
    if (a.catchup) {
        fx_row_load<VEC>(a.t[ti], row, sub, r);
        fx_catchup_finish<VEC>(a.t[ti], row, sub, r, sc, upto, lg, ser);
    } else {                                   // plain gather: only the row itself (no optimizer state)
        const int lanes = 1 << a.t[ti].lanes_log2;
        r.act = sub < lanes;
        r.on = r.act && sub * VEC < a.t[ti].D;
        if (r.on) fx_tab_load<VEC>(a.t[ti].table, a.t[ti].bf16, row * a.t[ti].tld + sub * VEC, r.p);
    }
    fx_owner_put<VEC>(a, ti, r, sub, beg, end);
}

__global__ __launch_bounds__(256) void k_owner_fetch_rows(OwnerFetchArgs a) {
    const int glanes = 1 << a.group_log2;
    const int sub = threadIdx.x & (glanes - 1);
    const int64_t rpb = 256 >> a.group_log2;
    const int nu = *a.n_unique;
    fx_scalars sc;
    int upto = 0;
    FxLogs lg{0.0, 0.0, 0.0, 0.0};
    FxSeries ser{nullptr, 0};
    if (a.catchup) {
        sc = *a.scal;
        upto = sc.step + a.upto_offset;
        lg = fx_logs_of(sc);
        ser = fx_series_of(a.scal, sc);
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < a.zero_w; i += 256) a.zero_row[i] = 0.f;
    const int64_t gid = (int64_t)blockIdx.x * rpb + (threadIdx.x >> a.group_log2);
    const int64_t gstride = (int64_t)gridDim.x * rpb;
    for (int64_t u = gid; u < nu; u += gstride) {
        const int64_t row = a.uniq_row[u];
        const uint32_t beg = a.seg_start[u], end = a.seg_start[u + 1];
        if (a.quad) {
            // the shape of k_catchup_rows' quad replay, by the same function: a row is caught up to the same
            // bits whether its owner is this rank of N or the only rank (round 6; the plain replays below
            // round the k <= FX_SERIES_KDIR steps differently)
            FxRowRegs<4> r0;
            FxRowRegs<1> r1;
            if (a.quad == 1) fx_catchup_quad<true>(a.t[0], a.t[1], row, sub, sc, upto, lg, ser, r0, r1);
            else fx_catchup_quad<false>(a.t[0], a.t[0], row, sub, sc, upto, lg, ser, r0, r1);
            fx_owner_put<4>(a, 0, r0, sub, beg, end);
            if (a.quad == 1) fx_owner_put<1>(a, 1, r1, sub, beg, end);
        } else if (a.catchup && a.n_tables == 2 && a.t[0].vec == 4 && a.t[1].vec == 1) {
            // the D-float tables + the D=1 tables of LogisticRegression: all eight loads in flight
            FxRowRegs<4> r0;
            FxRowRegs<1> r1;
            fx_row_load<4>(a.t[0], row, sub, r0);
            fx_row_load<1>(a.t[1], row, sub, r1);
            fx_catchup_finish<4>(a.t[0], row, sub, r0, sc, upto, lg, ser);
            fx_catchup_finish<1>(a.t[1], row, sub, r1, sc, upto, lg, ser);
            fx_owner_put<4>(a, 0, r0, sub, beg, end);
            fx_owner_put<1>(a, 1, r1, sub, beg, end);
        } else {
            for (int ti = 0; ti < a.n_tables; ++ti) {
                const int vec = a.t[ti].vec;
                if (vec == 4) fx_owner_one<4>(a, ti, row, sub, sc, upto, lg, ser, beg, end);
                else if (vec == 2) fx_owner_one<2>(a, ti, row, sub, sc, upto, lg, ser, beg, end);
                else fx_owner_one<1>(a, ti, row, sub, sc, upto, lg, ser, beg, end);
            }
        }
        if (sub == 0)                                          // pad columns of the block's rows
            for (uint32_t i = beg; i < end; ++i)
                for (int c = a.used_w; c < (int)a.ld; ++c)
                    a.send[(int64_t)a.sorted_pos[i] * a.ld + c] = 0.f;
    }
    // entries that asked for nothing (pad ids sort to the tail): zero rows
    const int64_t n_valid = a.seg_start[nu];
    for (int64_t i = n_valid + (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n_total;
         i += (int64_t)gridDim.x * 256) {
        float* dst = a.send + (int64_t)a.sorted_pos[i] * a.ld;
        for (int c = 0; c < (int)a.ld; ++c) dst[c] = 0.f;
    }
}

extern "C" int fx_owner_fetch_rows(const fx_row_state* tables_host, const int32_t* off_host,
                                   int32_t n_tables, const uint32_t* uniq_row,
                                   const uint32_t* seg_start, const uint32_t* sorted_pos,
                                   const int32_t* n_unique, int64_t n_total, float* send, int64_t ld,
                                   int32_t catchup, int32_t upto_offset, const fx_scalars* scal,
                                   float* zero_row, int32_t zero_w, fx_stream_t stream) {
    FX_CHECK_ARG(n_tables >= 1 && n_tables <= FX_MAX_TABLES,
                 "fx_owner_fetch_rows: n_tables=%d not in [1,%d]", n_tables, FX_MAX_TABLES);
    FX_CHECK_ARG(zero_w >= 0 && (zero_w == 0 || zero_row), "fx_owner_fetch_rows: zero_w without zero_row");
    if (n_total <= 0) return FX_OK;
    FX_CHECK_ARG(tables_host && off_host && uniq_row && seg_start && sorted_pos && n_unique && send,
                 "fx_owner_fetch_rows: null pointer");
    FX_CHECK_ARG(!catchup || scal, "fx_owner_fetch_rows: catch-up without scal");
    OwnerFetchArgs a;
    memset(&a, 0, sizeof(a));
    int gl = 0;
    const int st = fx_fill_tables(tables_host, n_tables, a.t, &gl, "fx_owner_fetch_rows", catchup != 0);
    if (st != FX_OK) return st;
    int used = 0;
    for (int t = 0; t < n_tables; ++t) {
        FX_CHECK_ARG(off_host[t] >= 0 && off_host[t] + a.t[t].D <= ld && off_host[t] % a.t[t].vec == 0 &&
                         ld % a.t[t].vec == 0,
                     "fx_owner_fetch_rows: table %d does not fit / align in the block", t);
        a.off[t] = off_host[t];
        if (off_host[t] + a.t[t].D > used) used = off_host[t] + a.t[t].D;
    }
    a.uniq_row = uniq_row; a.seg_start = seg_start; a.sorted_pos = sorted_pos; a.n_unique = n_unique;
    a.send = send; a.ld = ld; a.n_total = n_total; a.scal = scal; a.n_tables = n_tables;
    a.group_log2 = gl; a.upto_offset = upto_offset; a.catchup = catchup ? 1 : 0; a.used_w = used;
    a.zero_row = zero_row; a.zero_w = zero_w;
    a.quad = catchup ? fx_quad_mode(a.t, n_tables, gl) : 0;
    int64_t blocks = fx_ceil_div(n_total, 256 >> gl);
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(k_owner_fetch_rows, dim3((unsigned)blocks), dim3(256), 0, fx_hip_stream(stream), a);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// ---------------------------------------------------------------------------------------------
// embedding regularizer (rank_model.py:95-112): a dense term over EVERY table row.  Three kernels:
//   k_reg_stats   sum p^2, sum |p|, sum r^2 (r = l1 sign(p) + l2 p) over the whole packed table
//   k_reg_cross   sum 2 G.r over the rows the batch touched: with it
//                 |G + r|^2 summed over all rows = sum r^2 + sum G^2 + sum 2 G.r
//   k_reg_dense   the optimizer step with g = r for the rows the batch did NOT touch
//                 (touched rows: k_sparse_update_multi adds r itself and marks last_step)
// All three read one packed fp32 table.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reg_stats(const float* __restrict__ x, int64_t n,
                                                   const fx_scalars* scal, float* partials) {
    __shared__ float red4[4];
    const float l1 = scal->reg_l1, l2 = scal->reg_l2;
    float s2 = 0.f, s1 = 0.f, sr = 0.f;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? (n >> 2) : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 q = x4[i];
        const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float r = fx_reg_grad(e[k], l1, l2);
            s2 = fmaf(e[k], e[k], s2);
            s1 += fabsf(e[k]);
            sr = fmaf(r, r, sr);
        }
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float e = x[i], r = fx_reg_grad(e, l1, l2);
        s2 = fmaf(e, e, s2);
        s1 += fabsf(e);
        sr = fmaf(r, r, sr);
    }
    const float t2 = fx_block_sum_256(s2, red4);
    __syncthreads();
    const float t1 = fx_block_sum_256(s1, red4);
    __syncthreads();
    const float tr = fx_block_sum_256(sr, red4);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = t2;
        partials[FX_REG_BLOCKS + blockIdx.x] = t1;
        partials[2 * FX_REG_BLOCKS + blockIdx.x] = tr;
    }
}

extern "C" int fx_reg_stats(const float* x, int64_t n, const fx_scalars* scal, float* partials,
                            fx_stream_t stream) {
    FX_CHECK_ARG(n >= 0, "fx_reg_stats: n=%lld", (long long)n);
    FX_CHECK_ARG((x || n == 0) && scal && partials, "fx_reg_stats: null pointer");
    hipLaunchKernelGGL(k_reg_stats, dim3(FX_REG_BLOCKS), dim3(256), 0, fx_hip_stream(stream), x, n,
                       scal, partials);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

// the packed fp32 table that fx_reg_cross / fx_reg_dense_update are given, as the kernels take it
static int fx_reg_table(const float* table, float* m, float* v, const int32_t* last_step, int32_t D,
                        const float* G, FxTableDev* out, int* group_log2, const char* who) {
    fx_row_state h;
    memset(&h, 0, sizeof(h));
    h.table = const_cast<float*>(table); h.m = m; h.v = v; h.last_step = const_cast<int32_t*>(last_step);
    h.G = G; h.D = D;
    h.table_dtype = FX_F32;
    return fx_fill_tables(&h, 1, out, group_log2, who, false);
}

template <int VEC>
__global__ __launch_bounds__(256) void k_reg_cross(FxTableDev a, const uint32_t* uniq_row,
                                                   const int32_t* n_unique, const fx_scalars* scal,
                                                   float* partials) {
    __shared__ float red4[4];
    const float* table = reinterpret_cast<const float*>(a.table);
    const int lanes = 1 << a.lanes_log2;
    const int sub = threadIdx.x & (lanes - 1);
    const int d0 = sub * VEC;
    const int nu = *n_unique;
    const int64_t rpb = 256 >> a.lanes_log2;
    const float l1 = scal->reg_l1, l2 = scal->reg_l2;
    float acc = 0.f;
    for (int64_t u = (int64_t)blockIdx.x * rpb + (threadIdx.x >> a.lanes_log2); u < nu;
         u += (int64_t)gridDim.x * rpb) {
        if (d0 >= a.D) continue;
        const int64_t row = uniq_row[u];
        float p[VEC], g[VEC];
        fx_load<VEC>(table + row * a.D + d0, p);
        fx_load<VEC>(a.G + u * a.D + d0, g);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc = fmaf(2.f * g[k], fx_reg_grad(p[k], l1, l2), acc);
    }
    const float tot = fx_block_sum_256(acc, red4);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

extern "C" int fx_reg_cross(const float* table, int32_t D, const uint32_t* uniq_row,
                            const int32_t* n_unique, int64_t n_max, const float* G,
                            const fx_scalars* scal, float* partials, fx_stream_t stream) {
    FX_CHECK_ARG(D >= 1 && D <= 256, "fx_reg_cross: D=%d not in [1,256]", D);
    FX_CHECK_ARG(table && uniq_row && n_unique && G && scal && partials,
                 "fx_reg_cross: null pointer");
    FxTableDev a;
    int gl = 0;
    const int st = fx_reg_table(table, nullptr, nullptr, nullptr, D, G, &a, &gl, "fx_reg_cross");
    if (st != FX_OK) return st;
    hipStream_t s = fx_hip_stream(stream);
    dim3 grid(FX_REG_CROSS_BLOCKS);       // fixed: every block writes its (possibly zero) partial
    if (a.vec == 4) hipLaunchKernelGGL(k_reg_cross<4>, grid, dim3(256), 0, s, a, uniq_row, n_unique, scal, partials);
    else if (a.vec == 2) hipLaunchKernelGGL(k_reg_cross<2>, grid, dim3(256), 0, s, a, uniq_row, n_unique, scal, partials);
    else hipLaunchKernelGGL(k_reg_cross<1>, grid, dim3(256), 0, s, a, uniq_row, n_unique, scal, partials);
    FX_CHECK_LAUNCH();
    return FX_OK;
}

template <int VEC, bool ADAM>
__global__ __launch_bounds__(256) void k_reg_dense(FxTableDev a, int64_t total_rows,
                                                   const fx_scalars* scal) {
    float* table = reinterpret_cast<float*>(a.table);
    const int lanes = 1 << a.lanes_log2;
    const int sub = threadIdx.x & (lanes - 1);
    const int d0 = sub * VEC;
    const int64_t rpb = 256 >> a.lanes_log2;
    const fx_scalars sc = *scal;
    const float scale = sc.lr * sc.clip_coef;
    for (int64_t row = (int64_t)blockIdx.x * rpb + (threadIdx.x >> a.lanes_log2); row < total_rows;
         row += (int64_t)gridDim.x * rpb) {
        if (d0 >= a.D) continue;
        if (a.last_step[row] == sc.step) continue;       // updated by the sparse kernel this step
        const int64_t o = row * a.D + d0;
        float p[VEC], g[VEC];
        fx_load<VEC>(table + o, p);
#pragma unroll
        for (int k = 0; k < VEC; ++k) g[k] = fx_reg_grad(p[k], sc.reg_l1, sc.reg_l2);
        if constexpr (ADAM) {
            float m[VEC], v[VEC];
            fx_load<VEC>(a.m + o, m);
            fx_load<VEC>(a.v + o, v);
            fx_adam_vec<VEC>(p, m, v, g, sc);
            fx_store<VEC>(a.m + o, m);
            fx_store<VEC>(a.v + o, v);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) p[k] = p[k] - scale * g[k];
        }
        fx_store<VEC>(table + o, p);
    }
}

extern "C" int fx_reg_dense_update(float* table, float* m, float* v, const int32_t* last_step,
                                   int64_t total_rows, int32_t D, int32_t adam,
                                   const fx_scalars* scal, fx_stream_t stream) {
    FX_CHECK_ARG(D >= 1 && D <= 256, "fx_reg_dense_update: D=%d not in [1,256]", D);
    if (total_rows <= 0) return FX_OK;
    FX_CHECK_ARG(table && last_step && scal && (!adam || (m && v)),
                 "fx_reg_dense_update: null pointer");
    FxTableDev a;
    int gl = 0;
    const int st = fx_reg_table(table, m, v, last_step, D, nullptr, &a, &gl, "fx_reg_dense_update");
    if (st != FX_OK) return st;
    int64_t blocks = fx_ceil_div(total_rows, 256 >> gl);
    if (blocks > 256 * 32) blocks = 256 * 32;
    dim3 grid((unsigned)blocks);
    hipStream_t s = fx_hip_stream(stream);
#define FX_REG_DENSE(V)                                                                                   \
    do {                                                                                                  \
        if (adam) hipLaunchKernelGGL((k_reg_dense<V, true>), grid, dim3(256), 0, s, a, total_rows, scal); \
        else hipLaunchKernelGGL((k_reg_dense<V, false>), grid, dim3(256), 0, s, a, total_rows, scal);     \
    } while (0)
    if (a.vec == 4) FX_REG_DENSE(4);
    else if (a.vec == 2) FX_REG_DENSE(2);
    else FX_REG_DENSE(1);
#undef FX_REG_DENSE
    FX_CHECK_LAUNCH();
    return FX_OK;
}
