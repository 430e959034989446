// fx_seq_parts.h — a sample's column parts (struct fx_seq_parts, include/fxctr.h: the address rule is stated there)
// as the kernels of fx_bst.hip and fx_gru.hip walk them, and the entry points' per-part argument tests.
// Column c of a row of n_parts * D floats is column cc = c - part * D of part = c / D.  A description travels by
// value in the kernel's argument block; the loads by a lane's own `part` are vector loads from that block, so a
// caller that can hoist `part` out of a loop does so itself: everything here is a plain inline expression.
// (The struct keeps the fields of one side within 64 bytes; DESIGN.md 4.13.1 has the 46 VGPRs the other order cost.)
#pragma once
#include "fx_common.h"

static inline int64_t fx_al4(int64_t n) { return (n + 3) / 4 * 4; }

// Part i of one side of a description: a null pointer passes only where `nullable` (a gradient nobody wants, then
// its strides are not looked at); the sequence side must hold `rows` positions of D floats, the target side D floats.
// `what` names the description in the message ("part", "gradient of part").
static inline int fx_parts_check_seq(const char* who, const char* what, const fx_seq_parts* d, int i, int D,
                                     int64_t rows, bool nullable) {
    if (d->seq[i] == nullptr) {
        FX_CHECK_ARG(nullable, "%s: null %s %d", who, what, i);
        return FX_OK;
    }
    FX_CHECK_ARG(d->seq_row_ld[i] >= D && d->seq_ld[i] >= rows * d->seq_row_ld[i],
                 "%s: %s %d: strides %lld / %lld below D / %lld rows", who, what, i, (long long)d->seq_row_ld[i],
                 (long long)d->seq_ld[i], (long long)rows);
    return FX_OK;
}

static inline int fx_parts_check_tgt(const char* who, const char* what, const fx_seq_parts* d, int i, int D,
                                     bool nullable) {
    if (d->tgt[i] == nullptr) {
        FX_CHECK_ARG(nullable, "%s: null %s %d", who, what, i);
        return FX_OK;
    }
    FX_CHECK_ARG(d->tgt_ld[i] >= D, "%s: %s %d: target stride %lld < D", who, what, i, (long long)d->tgt_ld[i]);
    return FX_OK;
}

#ifdef __HIPCC__
// column cc of part `part`, as an offset from seq[part] / tgt[part]: position t of sample b's history / its target
__device__ __forceinline__ int64_t fx_parts_seq_off(const fx_seq_parts& d, int part, int64_t b, int t, int cc) {
    return b * d.seq_ld[part] + (int64_t)t * d.seq_row_ld[part] + cc;
}
// ... of column c of the whole row: -> its part, and the offset inside that part
__device__ __forceinline__ int64_t fx_parts_seq_off(const fx_seq_parts& d, int D, int64_t b, int t, int c, int& part) {
    part = c / D;
    return fx_parts_seq_off(d, part, b, t, c - part * D);
}
__device__ __forceinline__ int64_t fx_parts_tgt_off(const fx_seq_parts& d, int part, int64_t b, int cc) {
    return b * d.tgt_ld[part] + cc;
}

// a gradient through a description: a null destination is skipped, `acc` adds to what is there
__device__ __forceinline__ void fx_parts_put(const float* base, int64_t off, float v, bool acc) {
    if (base == nullptr) return;
    float* dst = const_cast<float*>(base) + off;
    *dst = acc ? *dst + v : v;
}
#endif
