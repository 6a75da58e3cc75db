// ls_switch_plan.h — the small-batch switches: which (metric, stored dtype, placement) a switch serves and with what words
// it is refused otherwise ("The small-batch switches"). Plain inline functions (no HIP): the one setter of the
// flat handle (ls_switch.hip) and ls_ivf_set_small_batch (ls_ivf.hip) take every refusal from ls_switch_ask, and
// tests/switch_plan_check.cpp holds it, row for row, to what the setters answered before there was a table.
//
//   switch   ls_index field   served by                              settles first   on a group handle
//   f16      opt_mq16         inner product, fp16 rows               yes             every member, row shards' score vectors sized
//   sq8      opt_mq8          inner product, sq8 codes, one device   yes             refused
//   subset   opt_mqs          inner product, fp32 rows, one device   no              refused on enable, LS_OK on disable
//   l2       opt_l2_batch     L2, one device                         yes             refused
//   ivf      (ls_ivf)         inner product, fp32 rows               -               -
// bf16 rows (LS_DTYPE_BF16) are served by none of them: f16 and sq8 refuse such a handle either way, subset and ivf on
// enable, each with words that say "bf16 rows".
//
// (The field column is code in ls_switch.hip's set_switch only - this header cannot name ls_index: a new switch is a row
// here AND a field there.) Every refusal is LS_ERR_INVALID_ARG and comes before any device check. The checks run in the
// order written below: where several apply, the first is the one issued. The subset and IVF rules look at `enable`
// (switching them off is allowed wherever the handle's metric is theirs); the others do not.
#pragma once
#include "../../include/leansearch_l2.h"  // LS_OK, LS_ERR_INVALID_ARG, LS_DTYPE_*, LS_METRIC_*

enum ls_switch { LS_SW_F16, LS_SW_SQ8, LS_SW_SUBSET, LS_SW_L2, LS_SW_IVF, LS_SW_COUNT };
enum ls_switch_place { LS_PLACE_SINGLE, LS_PLACE_SHARDED, LS_PLACE_REPLICATED, LS_PLACE_NA /* an IVF handle */ };

struct ls_switch_facts {  // what the setter needs beside the rule
    const char* setter;  // the extern "C" name: the first word of every message
    bool settles;        // an accepted call finishes what is queued or awaits a repair under the old setting first
    bool forwards;       // on a group handle: to every member (else a group that passes the rule has nothing to switch)
};
static inline ls_switch_facts ls_switch_facts_of(ls_switch sw) {
    switch (sw) {
    case LS_SW_F16: return {"ls_set_f16_small_batch", true, true};
    case LS_SW_SQ8: return {"ls_set_sq8_small_batch", true, false};
    case LS_SW_SUBSET: return {"ls_set_subset_small_batch", false, false};
    case LS_SW_L2: return {"ls_set_l2_small_batch", true, false};
    default: return {"ls_ivf_set_small_batch", false, false};
    }
}

// rc == LS_OK: served. Otherwise the message is printf(fmt, fill) (fill: what the index stores, where fmt has a %s).
struct ls_switch_answer { int rc; const char *fmt, *fill; };

static inline ls_switch_answer ls_switch_ask(ls_switch sw, int32_t metric, int32_t dtype, ls_switch_place place, int32_t enable) {
    const auto refuse = [](const char* fmt, const char* fill = nullptr) { return ls_switch_answer{LS_ERR_INVALID_ARG, fmt, fill}; };
    const bool l2 = metric == LS_METRIC_L2;
    const bool group = place == LS_PLACE_SHARDED || place == LS_PLACE_REPLICATED;
    const char* stores = dtype == LS_DTYPE_F16 ? "fp16 rows" : "sq8 codes";  // (asked for where the dtype is not fp32)
    const bool bf16 = dtype == LS_DTYPE_BF16;  // (include/leansearch_bf16.h: its own words, ahead of the other dtypes')
    switch (sw) {
    case LS_SW_F16:
        if (l2) return refuse("ls_set_f16_small_batch: an L2 index (every L2 query is served alone by the scan)");
        if (bf16) return refuse("ls_set_f16_small_batch: the index stores bf16 rows (every bf16 query is served alone by the scan)");
        if (dtype == LS_DTYPE_SQ8)
            return refuse("ls_set_f16_small_batch: the index stores sq8 codes (every sq8 query is served alone by the scan)");
        if (dtype != LS_DTYPE_F16)
            return refuse("ls_set_f16_small_batch: the index stores fp32 rows (small fp32 batches already share a pass)");
        break;
    case LS_SW_SQ8:
        if (l2) return refuse("ls_set_sq8_small_batch: an L2 index (it stores no sq8 codes; every L2 query is served alone by the scan)");
        if (bf16) return refuse("ls_set_sq8_small_batch: the index stores bf16 rows (every bf16 query is served alone by the scan)");
        if (dtype == LS_DTYPE_F16) return refuse("ls_set_sq8_small_batch: the index stores fp16 rows (ls_set_f16_small_batch is its option)");
        if (group || dtype != LS_DTYPE_SQ8)
            return refuse("ls_set_sq8_small_batch: not an sq8 index (small fp32 batches already share a pass)");
        break;
    case LS_SW_SUBSET:
        if (l2) return refuse("ls_set_subset_small_batch: an L2 index (every L2 query is served alone by the row-list scan)");
        if (enable && group)
            return refuse("ls_set_subset_small_batch: a sharded or replicated handle (its subset searches launch per query)");
        if (enable && bf16)
            return refuse("ls_set_subset_small_batch: the index stores %s (the subset pass serves fp32 rows)", "bf16 rows");
        if (enable && dtype != LS_DTYPE_F32)
            return refuse("ls_set_subset_small_batch: the index stores %s (the subset pass serves fp32 rows)", stores);
        break;
    case LS_SW_L2:
        if (!l2) return refuse("ls_set_l2_small_batch: not an L2 index (an inner-product index has its own small-batch options)");
        if (group) return refuse("ls_set_l2_small_batch: a sharded or replicated handle (the option serves an L2 index on one device)");
        break;
    default:  // LS_SW_IVF
        if (enable && l2)
            return refuse("ls_ivf_set_small_batch: an L2 IVF index (every L2 query is served alone by the probed-list scan)");
        if (enable && bf16)
            return refuse("ls_ivf_set_small_batch: the index stores %s (the IVF pass serves fp32 rows)", "bf16 rows");
        if (enable && dtype != LS_DTYPE_F32)
            return refuse("ls_ivf_set_small_batch: the index stores %s (the IVF pass serves fp32 rows)", stores);
    }
    return {LS_OK, nullptr, nullptr};
}
