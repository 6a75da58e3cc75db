// ls_scan_call_plan.h — what a scan-path call launches, decided from plain numbers: whether the call takes the two scan
// lanes, and per launch which kernel serves it, how many queries it carries, whether its selection rides in the launch,
// whether it writes score vectors and whether its queries can be served again later. Plain C++ (no HIP):
// scan_search_on_stream (ls_api.hip) fills ls_scan_call_in from the handle, the call's ls_scan_call (ls_index.h) and its
// stream, and does what the answers say; tests/scan_call_plan_check.cpp compiles this header alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ls_mq_plan.h"

#define LS_NSETS 2                       // scan scratch generations of the caller's stream (and of lane 0)
#define LS_LANE_MIN_BYTES (240ll << 20)  // stored corpus bytes (~35 us per pass) from which pipelined launches take two lanes
#define LS_MQ_KEEP_SLOTS 256             // launches without score vectors between two repairs (device-output calls)

// LDS bytes of a selection workgroup that holds keys_cap keys and ranks keff results
static inline size_t ls_fin_lds_bytes_host(int keys_cap, int keff) {
    int rc = 256;
    while (rc < keff) rc <<= 1;
    return ((size_t)keys_cap + (size_t)rc + 256 + 16) * sizeof(uint64_t) + (8 * 256 + 64) * sizeof(uint32_t);
}

// What the call's stream is to the handle (bits: a caller on the null stream is the active lanes' caller AND equal to a
// host slot's stream that was never created)
enum : unsigned {
    LS_STREAM_OWN = 1u,           // the library's own stream or a host slot's
    LS_STREAM_LANE = 2u,          // one of the two lane streams
    LS_STREAM_LANES_CALLER = 4u,  // the stream the active lanes are fed from
};

struct ls_scan_call_in {
    // storage
    int64_t n;
    int elem, chunks;  // bytes per stored element (4 fp32, 2 fp16, 1 sq8), 16-byte chunks per stored row
    int mq_kind;       // ls_mq_kind of the handle's ls_mq_in (ls_i_mq_in)
    int s_vecs;        // score vectors per scratch generation (refreshed after they grow)
    // switches (debug options 24, 3, 6, 19, 19, 9) and ls_set_profiling
    int opt_lanes;
    bool opt_overlap, opt_multi_query, opt_scan_skip_scores, opt_mq_skip_scores, opt_same_launch, profiling;
    // the call's context (ls_scan_call)
    bool has_done, has_retry, gen_forced, reserving, repairable;
    bool pipeline, inorder;  // LS_FLAG_PIPELINE, LS_FLAG_INORDER
    unsigned stream;         // LS_STREAM_* bits
    int32_t k;
    int64_t nq;
    int mq_max;        // ls_mq_max_queries for this (index, k)
    int64_t n_groups;  // ls_mq_group_count: launches the call is cut into
    bool lanes_active;
    // L2 handle with ls_set_l2_small_batch on (include/leansearch_l2_batch.h): its queries go out in VALU scan groups of
    // 8 / 4 / 1, although opt_multi_query is never set for an L2 handle. Off (the default, and for every other handle):
    // every decision below is what it was without the field.
    bool l2_groups;
};

// Queries of an L2 handle's next launch with ls_set_l2_small_batch on, `left` remaining: the VALU groups' rule, and the
// launches a call of nq queries takes (scan_call_in's n_groups, ls_i_scan_group_count). Declined at 8 queries (DESIGN.md
// 4.11b), such a call goes out in groups of 4: fp16 rows of 4-chunk lanes (49..64, 97..128, 193..256 chunks: two launches
// of 4 measured faster than one of 8) and of 16 lanes x 2 chunks (17..32 chunks: the kernel is not built).
static inline bool ls_scan_l2_declines8(int elem, int chunks) {
    const bool v4 = (chunks > 48 && chunks <= 64) || (chunks > 96 && chunks <= 128) || (chunks > 192 && chunks <= 256);
    return elem == 2 && (v4 || (chunks > 16 && chunks <= 32));
}
static inline int ls_scan_l2_group_size(int64_t left, int elem, int chunks) {
    return left >= 5 && !ls_scan_l2_declines8(elem, chunks) ? 8 : (left >= 2 ? 4 : 1);
}
static inline int64_t ls_scan_l2_group_count(int64_t nq, int elem, int chunks) {
    int64_t groups = 0;
    for (int64_t left = nq; left > 0; ++groups) left -= ls_scan_l2_group_size(left, elem, chunks);
    return groups;
}

// A device-output call's results may be repaired after it was queued: pipelined results are final after ls_check,
// synchronous ones when the call returns; LS_FLAG_ASYNC alone promises stream order, LS_FLAG_INORDER the lanes' order
static inline bool ls_scan_call_repairable(bool pipeline, bool async, bool inorder) {
    return !inorder && (pipeline || !async);
}

// ---- per call ------------------------------------------------------------------------------------------------------
struct ls_scan_call_plan {
    bool bad_groups;   // a call that owns one scratch generation must be a single query group
    bool lane_call;    // the call's one launch goes to a scan lane
    bool drain_lanes;  // the lanes run dry first
    bool ride;         // selection jobs may ride on a later launch (else: flushed before and after every call)
    bool leave_pending;  // ... and the last launch's jobs wait for the next call
};
static inline ls_scan_call_plan ls_scan_call_make_plan(const ls_scan_call_in& in) {
    ls_scan_call_plan p{};
    p.bad_groups = in.gen_forced && in.n_groups != 1;
    // Pipelined calls that are ONE launch without score vectors alternate between the two scan lanes (ls_index.h).
    // Everything else - several query groups, VALU groups that keep their score vectors, LS_FLAG_INORDER, a call
    // while ls_set_profiling is on (its event pairs would time a launch's wait for CUs), a repair's own launches -
    // stays on the caller's stream, after the lanes have run dry. So does every launch over a corpus of less than
    // LS_LANE_MIN_BYTES: a lane call costs the host a copy launch, two event records and two waits on top of the
    // scan launch, and a pass shorter than that queueing work is host-bound on two lanes (153.6 MB of fp16 rows:
    // 26.5 us per step on one stream, 27.8 on two; 307 MB and more: 2.4-6.9 us gained - docs/EXPERIMENTS.md).
    // Debug option 24 = 2 lifts the size rule (tests, A/B).
    const bool lane_size = in.opt_lanes == 2 || (int64_t)in.n * in.chunks * 16 >= LS_LANE_MIN_BYTES;
    const bool lane_kind = (in.mq_max > 0 && (in.nq >= 2 || in.elem == 2)) || (in.nq == 1 && in.opt_scan_skip_scores);
    p.lane_call = in.pipeline && in.opt_lanes && in.opt_overlap && !in.profiling && in.repairable &&
                  !in.reserving && !in.has_done && !in.gen_forced && in.opt_mq_skip_scores &&
                  in.n > 0 && in.n_groups == 1 && lane_kind && lane_size &&
                  !(in.stream & LS_STREAM_LANE);
    p.drain_lanes = in.lanes_active && !(p.lane_call && (in.stream & LS_STREAM_LANES_CALLER));  // (a stream switch too: the new caller starts over)
    p.ride = in.opt_overlap;
    p.leave_pending = in.pipeline && in.opt_overlap;
    return p;
}

// ---- per launch ----------------------------------------------------------------------------------------------------
enum ls_scan_kernel { LS_K_SCAN = 0, LS_K_MQ, LS_K_MQ8, LS_K_MQ16 };
// The launch's kernel and queries, `left` queries of the call remaining. keep_full: the ring of kept queries has no slot
// left (or was sized for another d).
struct ls_scan_launch_shape {
    int kind;           // ls_scan_kernel
    int NQ, real;       // query slots of the launch (8 or 4 with the last real query repeated as padding, or 1) and real queries
    bool repair_first;  // the keep ring is full: what is pending becomes final before this launch
};
static inline ls_scan_launch_shape ls_scan_launch_make_shape(const ls_scan_call_in& in, bool lane_call, int64_t left,
                                                             bool keep_full) {
    // (ls_mq_group_size reads the kind and debug option 6 of the handle's ls_mq_in and nothing else: tests/scan_call_plan_check.cpp
    // compares this with the full ls_mq_in over its sweep)
    ls_mq_in mq_in{};
    mq_in.kind = in.mq_kind;
    mq_in.multi_query = in.opt_multi_query;
    const int mq_max = in.mq_max;
    // queries per launch: 8 or 4 with the last real query repeated as padding, or 1
    const bool mq16 = mq_max > 0 && in.elem == 2;
    const bool use_mq = mq_max > 0 && (left >= 2 || mq16);
    const bool mq8 = use_mq && in.elem == 1;  // (sq8 index, ls_set_sq8_small_batch: the same bits as its scan kernel)
    const int gsz = ls_mq_group_size(mq_in, left, mq_max);
    const bool valu_groups = in.opt_multi_query || (in.l2_groups && !use_mq);  // (an L2 handle: no pass serves it, mq_max is 0)
    const int NQ = use_mq ? gsz
                   : (!valu_groups || in.elem == 1 ? 1
                      : (!in.opt_multi_query ? ls_scan_l2_group_size(left, in.elem, in.chunks) : (left >= 5 ? 8 : (left >= 2 ? 4 : 1))));
    ls_scan_launch_shape s{};
    s.kind = mq16 ? LS_K_MQ16 : mq8 ? LS_K_MQ8 : use_mq ? LS_K_MQ : LS_K_SCAN;
    s.NQ = NQ;
    s.real = (int)std::min<int64_t>(NQ, left);
    s.repair_first = !lane_call && (use_mq || NQ == 1) && in.repairable && !in.reserving && keep_full;
    return s;
}

// ... and, with the workgroups and k' of the kernel chosen, what the launch carries
struct ls_scan_launch_plan {
    int own_keys_cap;   // LDS key capacity of the launch's own selection jobs
    bool same_launch;   // the selection jobs ride on their own queries' launch (synchronous host calls)
    bool host_words;    // the jobs answer through completion words the host polls, with a retry list behind them
    bool dev_keep;      // the launch keeps its raw queries: unproven ones are served again (mq_repair)
    bool skip_scores;   // the launch writes no score vectors
    bool grow_scores;   // ... it does, for more queries than the handle keeps vectors for: grow them to NQ first
};
static inline ls_scan_launch_plan ls_scan_launch_make_plan(const ls_scan_call_in& in, const ls_scan_launch_shape& sh,
                                                           int blocks, int kprime) {
    const int64_t keff = std::min<int64_t>(in.k, in.n);
    const bool use_mq = sh.kind != LS_K_SCAN;
    const int NQ = sh.NQ;
    ls_scan_launch_plan p{};
    // Synchronous host-API calls (ls_search: the reference's call, search/engine.py:250): the
    // selection jobs of THIS group ride on its own scan launch and wait inside the kernel for
    // the scan workgroups' keys - one launch per group instead of scan + selection, no kernel
    // boundary and no second launch latency in front of the selection. The hand-off is the
    // data itself (tagged write-through granules, no drain, no counter: ls_fin_params::gran); a job
    // whose emitted keys cannot be proven complete answers LS_DONE_RETRY in its completion word
    // and the host launches the stand-alone finalize behind the scan (host_call_finish).
    // Only on the library's own stream and only with completion words to answer through: a
    // caller's stream may be CU-masked, and device-output calls have no way to ask for a retry.
    p.own_keys_cap = std::max(256, blocks * kprime);
    p.same_launch =
        !in.pipeline && in.n > 0 && in.opt_same_launch != 0 && !in.reserving && in.has_done &&
        in.n_groups <= LS_NSETS &&
        (in.stream & LS_STREAM_OWN) &&  // (the library's own streams)
        keff <= 256 &&  // (k > 256 orders its result on 1024 threads: own launch)
        (int64_t)blocks * (kprime + 1) <= LS_GRAN_MAX &&
        ls_fin_lds_bytes_host(p.own_keys_cap, (int)std::max<int64_t>(keff, 1)) <= LS_PIGGY_LDS_MAX;
    // An ls_mq launch whose selection jobs ride along (synchronous host calls) writes NO score vectors: such
    // a job never reads S inside the launch anyway (it answers LS_DONE_RETRY), and its retry serves the
    // query again, alone, on the single-query path - the same bits: the scan kernel, or ls_mq16 where that serves
    // this (index, k) (host_call_finish). The 16 x n x 4 bytes of
    // stores cost 3 us of 57 (d = 384) and 4..29 us of 140..167 (d = 1024, 2..16 queries) at N = 200 k.
    // (k > 256: the selection has its own launch behind the pass; without S it answers the same way)
    p.host_words = !in.pipeline && in.has_done && in.has_retry && !in.reserving;
    // (device-output calls whose results ls_check may still repair: mq_repair; never a repair's own launch)
    p.dev_keep = (use_mq || (NQ == 1 && in.opt_scan_skip_scores)) && in.repairable &&
                 !in.reserving && !in.has_done && in.opt_mq_skip_scores && in.n > 0;
    // (single queries of synchronous host calls too - the reference's call: 0.5-1 us of 47 / 122)
    p.skip_scores = ((p.same_launch || p.host_words) && in.opt_mq_skip_scores) || p.dev_keep;
    p.grow_scores = !p.skip_scores && NQ > in.s_vecs;  // a wide launch that keeps its score vectors (rare: ls_i_grow_score_vectors)
    return p;
}
