// ls_mq_plan.h — the host side of every small-batch pass (ls_mq / ls_mq16 / ls_mq8 / ls_mq_subset), as plain numbers:
// whether an (index or subset, k) is served by passes at all, the launch geometry (workgroups, k', keys per lane), how
// a call's queries are grouped into passes, and the LDS a workgroup takes. Plain C++ (no HIP): ls_api.hip and
// ls_subset.hip fill ls_mq_in from the handle, the launchers take the LDS sizes, and tests/mq_plan_check.cpp compiles
// this header alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ls_scan_plan.h"

#ifdef __HIPCC__
#define LS_MQ_HD __host__ __device__
#else
#define LS_MQ_HD
#endif

#define LS_MQ_MIN_ROWS 4096              // shards (and subsets) below this stay on the VALU scan
#define LS_MQ_NQ 16                      // query columns of one MFMA block; a pass carries one block or two
#define LS_MQ_WAVES 4                    // waves per workgroup
#define LS_MQ_WAVES2 8                   // ... of ls_mq's two-block kernel
#define LS_FIN_WG_MAX 16                 // selection workgroups riding on one launch: workgroup w runs jobs w, w + 16, ..
// LDS bytes a piggy-backed finalize may use without lowering the scan's occupancy below 2/CU
#define LS_PIGGY_LDS_MAX (72 * 1024)
#define LS_MQ_LDS_MAX2 (136 * 1024)      // ls_mq, two blocks: 32 x (4 KB + 8) of queries (the key lists reuse them)
#define LS_MQ16_LDS_MAX2 (136 * 1024)    // ls_mq16, two blocks: 32 x (4 KB + 16)

// ---- LDS of a pass's workgroup ---------------------------------------------------------------------------------------
// The pitch between two queries (why each avoids bank conflicts: at the kernels) ...
LS_MQ_HD constexpr int mq_pitch(int chunks) { return chunks * 4 + 2; }      // ls_mq: floats, the stored row + 2
LS_MQ_HD constexpr int mq16_pitch(int chunks) { return chunks * 16 + 16; }  // ls_mq16: bytes, the stored row + 16
LS_MQ_HD constexpr int mq8_pitch(int chunks) { return chunks * 16 + 8; }    // ls_mq8: floats, the stored row + 8
LS_MQ_HD constexpr int mq_key_pitch(int tk) { return (tk + 14) / 16 * 16 + 1; }  // u64 between two queries' key lists
// ... and the whole: the queries, followed by (one block) or later overwritten by (two) the waves' key lists + bounds
constexpr size_t ls_mq_lds_layout(size_t query_bytes, int lane_keys, int nb, int wpb) {
    const size_t kb = (size_t)nb * LS_MQ_NQ * (mq_key_pitch(wpb * lane_keys) + wpb + 1) * sizeof(uint64_t);
    return nb == 1 ? query_bytes + kb : (query_bytes > kb ? query_bytes : kb);
}
constexpr size_t mq_lds_bytes(int chunks, int lane_keys, int nb, int wpb) {
    return ls_mq_lds_layout(((size_t)nb * LS_MQ_NQ * mq_pitch(chunks) * sizeof(float) + 15) / 16 * 16, lane_keys, nb, wpb);
}
constexpr size_t mq16_lds_bytes(int chunks, int lane_keys, int nb) {
    return ls_mq_lds_layout((size_t)nb * LS_MQ_NQ * mq16_pitch(chunks), lane_keys, nb, LS_MQ_WAVES);
}
constexpr size_t mq8_lds_bytes(int chunks, int lane_keys) {
    return ls_mq_lds_layout((size_t)LS_MQ_NQ * mq8_pitch(chunks) * sizeof(float), lane_keys, 1, LS_MQ_WAVES);
}

// ---- the plan --------------------------------------------------------------------------------------------------------
enum ls_mq_kind {
    LS_MQ_F32 = 0,  // ls_mq.hip: 2..32 queries, the scan kernel's bits
    LS_MQ_F16,      // ls_mq16.hip (ls_set_f16_small_batch): 1..32 queries
    LS_MQ_SQ8,      // ls_mq8.hip (ls_set_sq8_small_batch): 2..16 queries, the sq8 scan's bits
    LS_MQ_ROWLIST,  // ls_mq_subset.hip (ls_set_subset_small_batch): 2..16 queries over the rows of a subset of an fp32 index
    LS_MQ_IVF,      // ls_ivf_batch.hip (ls_ivf_set_small_batch): 2..16 queries over the union of their probed lists
};
// lists the union step of an IVF pass keeps in LDS (one mask word per list: 16 KB, beside 4 KB of partial sums)
#define LS_IVF_BATCH_MAX_NLIST 4096
struct ls_mq_in {
    int kind;            // ls_mq_kind: what the index stores (LS_MQ_ROWLIST: a subset search)
    bool opt_in;         // the kind's ls_set_*_small_batch (fp32 has none: debug option 16 alone)
    bool multi_query;    // debug option 6: several queries per pass at all
    bool mq;             // debug option 16: on the matrix cores (fp32 and row list)
    bool mq32;           // debug option 22: fp32 passes of 17..32 queries
    bool f32;            // row list: the index stores fp32 rows
    bool single_device;  // row list: not a sharded / replicated handle
    int32_t n_cu;
    int32_t max_blocks;  // workgroups the handle's candidate blocks have room for (LS_KP_MAX keys each)
    int32_t chunks;      // 16-byte chunks per stored row
    int32_t opt_blocks;  // debug option 7 (0: automatic)
    int32_t opt_kprime;  // debug option 0 (0: automatic)
    int32_t nlist;       // IVF: lists of the handle
};
struct ls_mq_plan {
    int blocks, kprime, keys;  // all 0: declined
};

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

// waves per workgroup of the pass that serves nq queries: ls_mq's two-block kernel runs eight (ls_mq.hip). The key-list
// rule counts these waves, so fp16 and sq8 evaluate it with four whatever nq is.
static inline int ls_mq_plan_waves(int kind, int nq) { return kind == LS_MQ_F32 && nq > LS_MQ_NQ ? LS_MQ_WAVES2 : LS_MQ_WAVES; }

// The launch of ONE pass of nq queries over `rows` rows (of the index, or of the subset), or all zeros: declined.
static inline ls_mq_plan ls_mq_plan_pass(const ls_mq_in& in, int64_t rows, int32_t k, int nq) {
    constexpr ls_mq_plan declined{0, 0, 0};
    const int kind = in.kind;
    // what differs between the kinds: the switches that grant the pass ...
    const bool granted = kind == LS_MQ_F32   ? in.mq
                         : kind == LS_MQ_F16 ? in.opt_in
                         // (16 prepared queries of a 64-chunk row: 64.5 KB of LDS; longer rows do not fit - mq8_lds_bytes)
                         : kind == LS_MQ_SQ8 ? in.opt_in && in.chunks <= 64
                         : kind == LS_MQ_IVF ? in.opt_in && in.f32 && in.nlist >= 1 && in.nlist <= LS_IVF_BATCH_MAX_NLIST
                                             : in.opt_in && in.mq && in.f32 && in.single_device;
    if (!(granted && in.multi_query && rows >= LS_MQ_MIN_ROWS && in.n_cu > 0 && in.max_blocks > 0)) return declined;
    // ... the waves per workgroup, and whether the workgroups fill their CU's LDS (two blocks of ls_mq; two blocks of
    // ls_mq16 rows from 3 KB: 99 / 132 KB of queries): such a launch leaves LS_FIN_WG_MAX CUs to the selection workgroups
    // that ride along (they would otherwise wait for a scan workgroup to end - and a same-launch selection for scan
    // workgroups that cannot start before it ends)
    const int waves = ls_mq_plan_waves(kind, nq);
    const bool alone = nq > LS_MQ_NQ && (kind == LS_MQ_F32 || (kind == LS_MQ_F16 && mq16_lds_bytes(in.chunks, 8, 2) +
                                                                                           LS_PIGGY_LDS_MAX > 160 * 1024));
    const int cap = std::min(alone ? std::max(8, in.n_cu - LS_FIN_WG_MAX) : in.n_cu, in.max_blocks);

    const int keff = (int)std::max<int64_t>(std::min<int64_t>(k, rows), 1);
    ls_mq_plan p;
    p.blocks = in.opt_blocks > 0 ? std::min(in.opt_blocks, in.max_blocks) : ls_mq_plan_blocks(rows, waves, cap);
    if (p.blocks < 1) return declined;
    int keys = ls_mq_plan_lane_keys(waves, p.blocks, keff);
    if (kind == LS_MQ_ROWLIST && keys == 0 && in.opt_blocks <= 0) {
        // k too large for the key lists of so few waves (two tiles per wave: a 10 % subset of 200 k rows runs 157
        // workgroups, and k = 1000 puts 1.6 of a query's top-k into every wave): one workgroup per CU, down to one tile
        // per wave, spreads them over more lists before the call is given up to the single-query launches
        const int64_t one_tile = ((rows + 15) / 16 + waves - 1) / waves;
        const int wide = (int)std::min<int64_t>(cap, one_tile);
        if (wide > p.blocks) {
            p.blocks = wide;
            keys = ls_mq_plan_lane_keys(waves, p.blocks, keff);
        }
    }
    // (an ls_mq workgroup ranks waves x keys of them and may emit more than the scan kernel's 15: at k = 1000 over
    // 224-241 workgroups - 4.2-4.5 of a query's top-k each on average - the 15-key cap left the proof unprovable for
    // 1.5e-3..3.6e-3 of the queries, each one a second serve of 140 us; 23 keys: 1e-9)
    p.kprime = in.opt_kprime > 0 ? std::min(in.opt_kprime, LS_MQ_KP_MAX - 1) : ls_kprime(p.blocks, keff, LS_MQ_KP_MAX);
    p.keys = ls_mq_plan_fit_keys(waves, keys, &p.kprime);  // k' + 1 of waves x keys go out
    p.kprime = ls_mq_plan_fit_stride(p.kprime, (int64_t)in.max_blocks * LS_KP_MAX, p.blocks);
    if (p.keys == 0 || p.kprime < 1) return declined;
    return p;
}

// The launch geometry for a group of nq queries of a call. fp16: ONE predicate per (index, k), blind to the query
// count - the 16-query plan. Where it holds every scan-path launch of that (index, k) - a lone query, a group of up to
// 32, a retry, a repair - is an ls_mq16 launch, so a query's bits never depend on its company; 17..32 queries of long
// rows run fewer workgroups, and where the key-list rule then declines what it grants 16 queries, the launch keeps the
// 16-query geometry. sq8 and row list: the plan takes no query count.
static inline ls_mq_plan ls_mq_make_plan(const ls_mq_in& in, int64_t rows, int32_t k, int nq) {
    if (in.kind != LS_MQ_F16 || nq <= LS_MQ_NQ) return ls_mq_plan_pass(in, rows, k, nq);
    const ls_mq_plan p16 = ls_mq_plan_pass(in, rows, k, LS_MQ_NQ);
    if (p16.keys == 0) return p16;
    const ls_mq_plan p = ls_mq_plan_pass(in, rows, k, nq);
    return p.keys > 0 ? p : p16;
}

// Queries one pass may carry for this (index or subset, k); 0: no pass serves it. fp32: 32 (two 16-column MFMA blocks
// per A operand) where the eight-wave plan fits and debug option 22 is on, else 16; fp16: 32; sq8 and row list: 16.
static inline int ls_mq_max_queries(const ls_mq_in& in, int64_t rows, int32_t k) {
    if (in.kind == LS_MQ_F32 && in.mq32 && ls_mq_make_plan(in, rows, k, 2 * LS_MQ_NQ).keys > 0) return 2 * LS_MQ_NQ;
    if (ls_mq_make_plan(in, rows, k, LS_MQ_NQ).keys == 0) return 0;
    return in.kind == LS_MQ_F16 ? 2 * LS_MQ_NQ : LS_MQ_NQ;
}

// Queries of the scan path's next launch when `left` remain and a pass carries mq_max (ls_mq_max_queries): ONE
// definition, shared by the scheduling and by the host API's decision to overlap a call.
static inline int ls_mq_group_size(const ls_mq_in& in, int64_t left, int mq_max) {
    // (sq8: one launch per query - DESIGN.md 4.9 - unless ls_set_sq8_small_batch lets 2..16 share a pass: 4.9b)
    if (in.kind == LS_MQ_SQ8) return mq_max > 0 && left >= 2 ? (int)std::min<int64_t>(left, mq_max) : 1;
    // (an fp16 index served by ls_mq16 sends its lone queries there too: the same bits alone or in company)
    if (mq_max > 0 && (left >= 2 || in.kind == LS_MQ_F16)) return (int)std::min<int64_t>(left, mq_max);
    return !in.multi_query ? 1 : (left >= 5 ? (int)std::min<int64_t>(left, 8) : (left >= 2 ? (int)std::min<int64_t>(left, 4) : 1));
}
// ... and the launches (query groups) a call of nq queries takes
static inline int64_t ls_mq_group_count(const ls_mq_in& in, int64_t rows, int32_t k, int64_t nq) {
    const int mq_max = ls_mq_max_queries(in, rows, k);
    int64_t groups = 0;
    for (int64_t left = nq; left > 0; ++groups) left -= ls_mq_group_size(in, left, mq_max);
    return groups;
}
// Row list: queries of the next pass when `left` remain: min(left, 16) while two or more are left; 0 = a lone query,
// which the single-query row-list scan serves (the same bits, so nothing is re-routed)
static inline int ls_mq_subset_group(int64_t left) { return left >= 2 ? (int)std::min<int64_t>(left, LS_MQ_NQ) : 0; }

// ---- IVF (LS_MQ_IVF): a group of g queries shares one pass over the union of its probed lists -------------------------
// The host never learns the union's size: it plans from the bound min(ntotal, g x rows_q), rows_q = the rows of the
// handle's nprobe largest lists (what ONE query probes at most; k counts against it: a query's top-k lies in its own lists).
static inline int64_t ls_mq_ivf_bound(int64_t ntotal, int64_t rows_q, int g) { return std::min<int64_t>(ntotal, (int64_t)g * rows_q); }
// The launch of a group of g queries, or all zeros. ONE predicate per (handle, k, nprobe), blind to the group size above
// 2: the plan of the smallest group. A larger group's bound is no smaller and mostly runs more workgroups, which only
// eases the key-list rule - but past one workgroup per CU ls_mq_plan_blocks may pick up to 8 % fewer than a smaller
// bound's, and on that edge the rule can decline what it grants two queries: such a group keeps the two-query geometry
// (as ls_mq_make_plan does for fp16), so no group of a served shape is without a plan.
static inline ls_mq_plan ls_mq_ivf_plan(const ls_mq_in& in, int64_t ntotal, int64_t rows_q, int32_t k, int g) {
    const int32_t kq = (int32_t)std::max<int64_t>(std::min<int64_t>(k, rows_q), 1);
    const ls_mq_plan p2 = ls_mq_plan_pass(in, ls_mq_ivf_bound(ntotal, rows_q, 2), kq, LS_MQ_NQ);
    if (g <= 2 || p2.keys == 0) return p2;
    const ls_mq_plan p = ls_mq_plan_pass(in, ls_mq_ivf_bound(ntotal, rows_q, g), kq, LS_MQ_NQ);
    return p.keys > 0 ? p : p2;
}
static inline bool ls_mq_ivf_served(const ls_mq_in& in, int64_t ntotal, int64_t rows_q, int32_t k) {
    return ls_mq_ivf_plan(in, ntotal, rows_q, k, 2).keys > 0;
}
