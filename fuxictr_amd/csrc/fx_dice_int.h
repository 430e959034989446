// fx_dice_int.h — the finishing steps of a two-stage column reduction, shared by fx_dice.hip (which defines
// them) and fx_din_attn.hip (internal, not part of the C ABI).  Stage 1 of either file leaves per-workgroup
// partial sums partial[(c * nt + k) * H + h] (chunk c, term k, column h); these launchers add the chunks in
// one fixed order and, for Dice, turn [sum z | sum z^2] into [mean | biased variance] and the running update.
// A kernel is launched only from the unit that defines it.  The caller checks the launch.
#pragma once
#include "fx_common.h"

// out[k * H + h] = sum over the chunks c of partial[(c * nt + k) * H + h], for k < nt
void fx_chunks_sum_launch(const float* partial, int chunks, int nt, int64_t H, float* out, hipStream_t s);

// the same for the nt = 2 terms [sum z | sum z^2] over n_total rows, and in the same launch stats[2H] =
// [mean | biased variance] and running = (1 - momentum) running + momentum [mean | unbiased variance] — the
// single-rank case, where nothing (no all-reduce) happens between the sums and the statistics.  sums (the
// 2H column sums) and num_batches_tracked (+= 1) are optional outputs.
void fx_chunks_stats_launch(const float* partial, int chunks, int H, int64_t n_total, float momentum,
                            float* sums, float* stats, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, hipStream_t s);
