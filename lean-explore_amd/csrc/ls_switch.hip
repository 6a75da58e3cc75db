// ls_switch.hip — the flat handle's small-batch switches (ls_switch_plan.h): ONE setter behind the four
// extern "C" names. Every refusal is the table's; this file locks, forwards to a group's members, settles the handle
// where the table says so and stores the flag (set_switch's last statement: the one map from a switch to its field).
#include "ls_index.h"
#include "ls_switch_plan.h"

#include "../../include/leansearch_l2_batch.h"
#include "../../include/leansearch_sq8_batch.h"
#include "../../include/leansearch_subset_batch.h"

// A call the table accepted. size_score_vectors (f16 only): sub-handles of a row-sharded group. Their sub-searches keep
// score vectors (stream-ordered, no repair), and with this option a sub-search carries up to 32 queries: the vectors are
// sized NOW (2 generations x 32 x n floats per shard), so that running out of device memory is this call's error, not a
// later search's.
static int set_switch(ls_index* ix, ls_switch sw, int32_t enable, bool size_score_vectors) {
    const ls_switch_facts f = ls_switch_facts_of(sw);
    ls_quiesce lk(ix);  // (no synchronous host call in flight, then the handle's mutex)
    if (ix->group) return f.forwards ? ls_group_set_f16_small_batch(ix, enable) : LS_OK;  // (LS_OK: the subset switch, off)
    if (f.settles) {  // what is queued or awaits a repair was routed under the old setting: finished under it
        LS_HIP(hipSetDevice(ix->device));
        if (int rc = ls_i_settle(ix)) return rc;
    }  // (subset calls leave nothing queued: that switch touches no device)
    if (sw == LS_SW_F16 && enable && size_score_vectors && ix->d_corpus)
        if (int rc = ls_i_grow_score_vectors(ix, LS_QUERIES_PER_LAUNCH_MAX)) return rc;
    (sw == LS_SW_F16 ? ix->opt_mq16 : sw == LS_SW_SQ8 ? ix->opt_mq8 : sw == LS_SW_SUBSET ? ix->opt_mqs : ix->opt_l2_batch) = enable != 0;
    return LS_OK;
}

int ls_i_set_f16_small_batch(ls_index* ix, int32_t enable, bool ssv) { return set_switch(ix, LS_SW_F16, enable, ssv); }

static int ask_and_set(ls_index* ix, ls_switch sw, int32_t enable) {
    if (!ix) {
        ls_set_error("%s: index is null", ls_switch_facts_of(sw).setter);
        return LS_ERR_INVALID_ARG;
    }
    const ls_switch_place place = !ix->group ? LS_PLACE_SINGLE : ls_group_is_replicated(ix) ? LS_PLACE_REPLICATED : LS_PLACE_SHARDED;
    const ls_switch_answer a = ls_switch_ask(sw, ix->metric, ix->dtype, place, enable);
    if (a.rc != LS_OK) {
        ls_set_error(a.fmt, a.fill);
        return a.rc;
    }
    return set_switch(ix, sw, enable, false);
}

extern "C" {
int ls_set_f16_small_batch(ls_index* ix, int32_t enable) { return ask_and_set(ix, LS_SW_F16, enable); }
int ls_set_sq8_small_batch(ls_index* ix, int32_t enable) { return ask_and_set(ix, LS_SW_SQ8, enable); }
int ls_set_subset_small_batch(ls_index* ix, int32_t enable) { return ask_and_set(ix, LS_SW_SUBSET, enable); }
int ls_set_l2_small_batch(ls_index* ix, int32_t enable) { return ask_and_set(ix, LS_SW_L2, enable); }
int32_t ls_l2_small_batch(const ls_index* ix) { return ix && ix->opt_l2_batch ? 1 : 0; }
}  // extern "C"
