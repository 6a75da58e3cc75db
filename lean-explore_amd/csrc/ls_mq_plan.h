// ls_mq_plan.h — how a small-batch (ls_mq / ls_mq16 / ls_mq8) launch is planned on the host: workgroups per launch, keys
// per lane, and how k' follows them. Plain C++ (no HIP): ls_mq.hip and ls_api.hip's plans take the rules from here, and
// so does the subset pass's plan (ls_mq_subset_plan.h), which a host program compiles alone.
#pragma once
#include <algorithm>
#include <cstdint>

#include "ls_scan_plan.h"

#define LS_MQ_MIN_ROWS 4096              // shards (and subsets) below this stay on the VALU scan

// workgroups of `wpb` waves for a launch over n rows, `cap` of them at most: one per CU at most, at least two tiles of
// 16 rows per wave
static inline int ls_mq_plan_blocks(int64_t n, int wpb, int64_t cap) {
    const int64_t NT = (n + 15) / 16;
    constexpr int tpw = 2;  // at least this many tiles per wave on small shards
    const int64_t b = (NT + wpb * tpw - 1) / (wpb * tpw);
    // (big shards: ONE workgroup per CU. tools/mq_blocks_sweep.py, N = 200 k, 16 queries, d = 384 / 768 / 1024:
    //  256 workgroups 60.3 / 128.6 / 167.0 us, 448: 67.2 / 140.9 / 179.7, 512: 65.0 / 137.0 / 176.9,
    //  768: 65.9 / 140.3 / 181.0 - four waves per CU with 12-16 KB in flight each already carry the HBM
    //  stream; more streams only add DRAM page conflicts and a longer tail)
    if (b <= cap) return (int)std::max<int64_t>(b, 1);
    // ... and among the counts in [0.92, 1] x CUs the one whose last round of tiles is the fullest (12 500 tiles
    // over 256 x 4 waves are 12.2 rounds: a fifth of the waves then runs a 13th tile alone; 241 workgroups make
    // it 12.97). Same box, 16 queries: 256 -> 241-250 workgroups 61.6 -> 59.4 us (d = 384), 142.3 -> 133.9 (d = 768),
    // 166.8 -> 167.7-170.5 (d = 1024: within the noise).
    int64_t best = cap;
    double best_fill = -1.0;
    for (int64_t c = cap; c >= cap * 92 / 100; --c) {
        const double rounds = (double)NT / (double)(c * wpb);
        double fill = rounds - (double)(int64_t)rounds;
        if (fill == 0.0) fill = 1.0;
        if (fill > best_fill + 0.02) {  // near-ties go to the larger count
            best_fill = fill;
            best = c;
        }
    }
    return (int)best;
}

// keys a lane - and, after the in-register merge of its four lane groups, a WAVE - keeps per query: the smallest
// of {3, 5, 8} for which "some wave of the launch holds more than that many of one query's top-k" is rarer than
// 2e-3 per query (the wave-level list is the binding one: a wave sees n / waves rows of the query, a Poisson(k /
// waves) number of them in the top-k; whatever it drops raises the workgroup's bound past the k-th key and the
// query is served again - 140 us at d = 1024). Round 5 priced the per-lane lists only; with two B blocks at
// k = 1000 (1792 waves, 0.56 top-k rows per wave) that chose 5 keys and 4 % of the queries were served twice.
// 0 = this kernel is the wrong tool (k too large for the shard: the scan path's groups take the call).
static inline int ls_mq_plan_lane_keys(int wpb, int blocks, int keff) {
    const double waves = (double)wpb * blocks;
    const double mu = (double)keff / waves;
    for (int m : {3, 5, 8}) {
        double term = __builtin_exp(-mu), tail = 1.0 - term;  // P(X >= 1)
        for (int j = 1; j <= m; ++j) {
            term *= mu / j;
            tail -= term;  // ... P(X >= m + 1)
        }
        if (tail < 0.0) tail = 0.0;
        if (tail * waves < 2e-3) return m;
    }
    return 0;
}

// A workgroup of `wpb` waves ranks wpb x keys keys and emits k' + 1 of them: the lists grow (3 -> 5 -> 8) until they
// hold that many, and k' gives way where 8 do not. Returns the keys per lane (0 stays 0: declined).
static inline int ls_mq_plan_fit_keys(int wpb, int keys, int* kprime) {
    while (keys > 0 && keys < 8 && *kprime + 1 > wpb * keys) keys = keys == 3 ? 5 : 8;
    if (keys > 0) *kprime = std::min(*kprime, wpb * keys - 1);
    return keys;
}
// ... and k' never runs past a query's candidate block: `stride` keys for `blocks` workgroups (a forced workgroup
// count near the handle's maximum at large k would otherwise)
static inline int ls_mq_plan_fit_stride(int kprime, int64_t stride, int blocks) {
    return (int)std::min<int64_t>(kprime, stride / blocks);
}
