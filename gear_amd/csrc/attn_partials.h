// attn_partials.h -- the decode partial dispatch of attention.hip for callers in other translation units (kivi.hip).
#pragma once
#include "common.h"

// where attn_decode_impl(..., keep) left the partial results of a launch: slot s of output row x = b * Hq + hq holds the
// unnormalised sum part_o[(x * pslots + s) * 128 + d] and (max, sum) part_ml[(x * pslots + s) * 2 + {0, 1}] of its chunk's scaled
// scores; an empty chunk has max = -inf
struct gear_attn_partials {
    const float* part_o;
    const float* part_ml;
    int pslots;
};

// Partial results of q [c->B, Hq, 128] over the first T compressed tokens of view c -- codes, scales and minima only: no factors,
// no outliers, no window -- in partials-only mode (one launch, no reduce).  T > 0, T % 64 == 0; workspace as for
// gear_attn_decode_workspace(c->B, Hq, T, c->bits).  Every argument check runs before the launch.
int gear_attn_partials_dense(const gear_cache_view* c, const void* q, int Hq, int T, float qscale, void* workspace,
                             size_t workspace_bytes, void* stream, gear_attn_partials* out);
