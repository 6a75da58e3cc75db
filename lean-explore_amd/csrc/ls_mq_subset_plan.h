// ls_mq_subset_plan.h — the host side of a subset pass (ls_mq_subset.hip: 2..16 queries share one pass over the m
// selected rows of an fp32 index): whether a (subset, k) is served by passes at all, and the launch geometry. Plain
// inline functions over plain numbers; no HIP, so a host program compiles them alone (tests/mq_subset_plan_check.cpp).
//
// ONE predicate per (subset, k), blind to the query count: where it holds, every group of 2..16 queries of a call is one
// pass; a lone query (and a lone rest) stays on the single-query row-list scan - the same bits, so nothing is re-routed.
#pragma once
#include "ls_mq_plan.h"

#define LS_MQ_SUBSET_WAVES 4   // waves per workgroup (one B block)
#define LS_MQ_SUBSET_NQ 16     // queries one pass carries

struct ls_mq_subset_in {
    bool enabled;          // ls_set_subset_small_batch
    bool multi_query, mq;  // debug options 6 and 16: several queries per pass at all, on the matrix cores
    bool f32;              // the index stores fp32 rows
    bool single_device;    // not a sharded / replicated handle
    int32_t n_cu;
    int32_t max_blocks;    // workgroups the handle's candidate blocks have room for (LS_KP_MAX keys each)
    int32_t opt_blocks;    // debug option 7 (0: automatic)
    int32_t opt_kprime;    // debug option 0 (0: automatic)
};
struct ls_mq_subset_plan {
    int blocks, kprime, keys;  // all 0: declined
};

static inline ls_mq_subset_plan ls_mq_subset_make_plan(const ls_mq_subset_in& in, int64_t m, int32_t k) {
    ls_mq_subset_plan p{0, 0, 0};
    if (!(in.enabled && in.multi_query && in.mq && in.f32 && in.single_device && m >= LS_MQ_MIN_ROWS &&
          in.n_cu > 0 && in.max_blocks > 0))
        return p;
    const int keff = (int)std::max<int64_t>(std::min<int64_t>(k, m), 1);
    p.blocks = in.opt_blocks > 0 ? std::min(in.opt_blocks, in.max_blocks)
                                 : std::min(ls_mq_plan_blocks(m, LS_MQ_SUBSET_WAVES, in.n_cu), in.max_blocks);
    if (p.blocks < 1) return ls_mq_subset_plan{0, 0, 0};
    int keys = ls_mq_plan_lane_keys(LS_MQ_SUBSET_WAVES, p.blocks, keff);
    if (keys == 0 && in.opt_blocks <= 0) {
        // k too large for the key lists of so few waves (two tiles per wave: a 10 % subset of 200 k rows runs 157
        // workgroups, and k = 1000 puts 1.6 of a query's top-k into every wave): one workgroup per CU, down to one tile
        // per wave, spreads them over more lists before the call is given up to the single-query launches
        const int64_t one_tile = ((m + 15) / 16 + LS_MQ_SUBSET_WAVES - 1) / LS_MQ_SUBSET_WAVES;
        const int wide = (int)std::min<int64_t>(std::min(in.n_cu, in.max_blocks), one_tile);
        if (wide > p.blocks) {
            p.blocks = wide;
            keys = ls_mq_plan_lane_keys(LS_MQ_SUBSET_WAVES, p.blocks, keff);
        }
    }
    p.kprime = in.opt_kprime > 0 ? std::min(in.opt_kprime, LS_MQ_KP_MAX - 1) : ls_kprime(p.blocks, keff, LS_MQ_KP_MAX);
    p.keys = ls_mq_plan_fit_keys(LS_MQ_SUBSET_WAVES, keys, &p.kprime);
    p.kprime = ls_mq_plan_fit_stride(p.kprime, (int64_t)in.max_blocks * LS_KP_MAX, p.blocks);
    if (p.keys == 0 || p.kprime < 1) return ls_mq_subset_plan{0, 0, 0};
    return p;
}

// queries of the next pass when `left` remain: min(left, 16) while two or more are left; 0 = a lone query, which the
// single-query row-list scan serves
static inline int ls_mq_subset_group(int64_t left) {
    return left >= 2 ? (int)std::min<int64_t>(left, LS_MQ_SUBSET_NQ) : 0;
}
