// l2_batch_plan_check.cpp — host check of the L2 query groups in ls_scan_call_plan.h (ls_scan_call_in::l2_groups,
// include/leansearch_l2_batch.h). Plain C++: compiles the plan headers alone.
//   1. an L2 handle (mq_max 0, opt_multi_query off, f32 or fp16 rows) with the field on: left = 1..17 gives
//      5.. -> 8 slots, 2..4 -> 4, 1 -> 1, real = min(slots, left), kind LS_K_SCAN; the call's group count agrees.
//      The declined shapes (fp16 rows of 17..32 chunks and of 4-chunk lanes at 8 queries) go out in groups of 4
//   2. the same with the field off: one query per launch throughout
//   3. every other input of a sweep over storage, switches, k and query counts: the call plan, the launch shape and the
//      launch plan are the same with the field set and clear (the field decides nothing where a handle is not L2:
//      multi-query on, or a pass serving it, or sq8 codes)
// Prints "ok <cases>" and exits 0, or says what differs and exits 1.
#include <cstdio>
#include <cstring>

#include "ls_scan_call_plan.h"

static int fails = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                \
            ++fails;                                   \
        }                                              \
    } while (0)

static ls_scan_call_in l2_handle(int elem, int chunks, int64_t nq, bool groups) {
    ls_scan_call_in in{};
    in.n = 200000, in.elem = elem, in.chunks = chunks, in.mq_kind = elem == 2 ? LS_MQ_F16 : LS_MQ_F32, in.s_vecs = 8;
    in.opt_lanes = 1, in.opt_overlap = true, in.opt_multi_query = false;  // (never set on an L2 handle: ls_i_mq_in)
    in.opt_scan_skip_scores = in.opt_mq_skip_scores = in.opt_same_launch = true;
    in.has_done = in.has_retry = true;
    in.stream = LS_STREAM_OWN;
    in.k = 10, in.nq = nq, in.mq_max = 0;
    in.l2_groups = groups;
    in.n_groups = groups ? ls_scan_l2_group_count(nq, elem, chunks) : nq;
    return in;
}

static bool same_shape(const ls_scan_launch_shape& a, const ls_scan_launch_shape& b) {
    return a.kind == b.kind && a.NQ == b.NQ && a.real == b.real && a.repair_first == b.repair_first;
}
static bool same_call(const ls_scan_call_plan& a, const ls_scan_call_plan& b) {
    return a.bad_groups == b.bad_groups && a.lane_call == b.lane_call && a.drain_lanes == b.drain_lanes && a.ride == b.ride &&
           a.leave_pending == b.leave_pending;
}
static bool same_launch(const ls_scan_launch_plan& a, const ls_scan_launch_plan& b) {
    return a.own_keys_cap == b.own_keys_cap && a.same_launch == b.same_launch && a.host_words == b.host_words &&
           a.dev_keep == b.dev_keep && a.skip_scores == b.skip_scores && a.grow_scores == b.grow_scores;
}

int main() {
    long long cases = 0;
    // ---- 1, 2: the group shapes of an L2 handle ----
    for (int elem : {4, 2})
      for (int chunks : {1, 16, 17, 24, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 256}) {
        // (the table of DESIGN.md 4.11b, restated: fp16 rows of 16 lanes x 2 chunks and of 4-chunk lanes)
        const bool declined8 = elem == 2 && (chunks == 17 || chunks == 24 || chunks == 32 || chunks == 64 || chunks == 128 ||
                                             chunks == 256 || chunks == 49 || chunks == 97 || chunks == 193);
        CHECK(ls_scan_l2_declines8(elem, chunks) == declined8, "declines8(%d, %d)", elem, chunks);
        for (int64_t left = 1; left <= 17; ++left) {
            const int want = left >= 5 && !declined8 ? 8 : (left >= 2 ? 4 : 1);
            for (bool keep_full : {false, true}) {
                const ls_scan_launch_shape on = ls_scan_launch_make_shape(l2_handle(elem, chunks, left, true), false, left, keep_full);
                CHECK(on.kind == LS_K_SCAN && on.NQ == want && on.real == (int)std::min<int64_t>(want, left),
                      "field on, %d-byte rows, left %lld: kind %d NQ %d real %d (want NQ %d)", elem, (long long)left, on.kind, on.NQ,
                      on.real, want);
                const ls_scan_launch_shape off = ls_scan_launch_make_shape(l2_handle(elem, chunks, left, false), false, left, keep_full);
                CHECK(off.kind == LS_K_SCAN && off.NQ == 1 && off.real == 1, "field off, left %lld: kind %d NQ %d real %d",
                      (long long)left, off.kind, off.NQ, off.real);
                cases += 2;
            }
            // the launches of a call of `left` queries: walking the shapes gives the group count the call was planned with
            const ls_scan_call_in in = l2_handle(elem, chunks, left, true);
            int64_t groups = 0, served = 0;
            for (int64_t l = left; l > 0; ++groups) {
                const ls_scan_launch_shape s = ls_scan_launch_make_shape(in, false, l, false);
                CHECK(s.NQ == ls_scan_l2_group_size(l, elem, chunks), "left %lld: NQ %d, ls_scan_l2_group_size %d", (long long)l, s.NQ,
                      ls_scan_l2_group_size(l, elem, chunks));
                l -= s.real, served += s.real;
            }
            CHECK(groups == in.n_groups && served == left, "nq %lld: %lld launches, planned %lld", (long long)left, (long long)groups,
                  (long long)in.n_groups);
            CHECK(!ls_scan_call_make_plan(in).bad_groups, "nq %lld: bad_groups without a forced generation", (long long)left);
        }
    }
    const int64_t counts[18] = {0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3};  // 9 = 8 + 1, 10 = 8 + 4 (2 real), 13 = 8 + 8 (5 real), 17 = 8 + 8 + 1
    for (int64_t nq = 1; nq <= 17; ++nq) {
        CHECK(ls_scan_l2_group_count(nq, 4, 96) == counts[nq], "ls_scan_l2_group_count(%lld) = %lld", (long long)nq,
              (long long)ls_scan_l2_group_count(nq, 4, 96));
        CHECK(ls_scan_l2_group_count(nq, 2, 32) == (nq + 3) / 4, "groups of 4: nq %lld -> %lld",
              (long long)nq, (long long)ls_scan_l2_group_count(nq, 2, 32));
    }

    // ---- 3: where the handle is not an L2 handle with its groups off, the field decides nothing ----
    for (int elem : {4, 2, 1})
        for (int mq_max : {0, 16, 32})
            for (int kind : {(int)LS_MQ_F32, (int)LS_MQ_F16, (int)LS_MQ_SQ8})
                for (int bits = 0; bits < 256; ++bits)
                  for (int chunks : {32, 96})  // (the declined fp16 shape too: the rule is the L2 groups' alone)
                    for (int64_t nq : {1, 2, 4, 5, 8, 9, 16, 17, 40})
                        for (int32_t k : {1, 10, 257, 2048}) {
                            ls_scan_call_in in{};
                            in.n = 200000, in.elem = elem, in.chunks = chunks, in.mq_kind = kind, in.s_vecs = 8;
                            in.opt_lanes = 1, in.opt_overlap = true, in.opt_same_launch = true;
                            in.opt_multi_query = bits & 1;
                            in.opt_scan_skip_scores = bits & 2, in.opt_mq_skip_scores = bits & 4;
                            in.has_done = bits & 8, in.has_retry = bits & 8, in.pipeline = bits & 16;
                            in.repairable = bits & 32, in.reserving = bits & 64, in.profiling = bits & 128;
                            in.stream = LS_STREAM_OWN, in.k = k, in.nq = nq, in.mq_max = mq_max;
                            // (an input the field could touch: multi-query off, no pass, not sq8 - an L2 handle's; 1, 2 above)
                            if (!in.opt_multi_query && elem != 1 && mq_max == 0) continue;
                            ls_mq_in mq{};
                            mq.kind = kind, mq.multi_query = in.opt_multi_query;
                            in.n_groups = 0;
                            for (int64_t l = nq; l > 0; ++in.n_groups) l -= ls_mq_group_size(mq, l, mq_max);
                            ls_scan_call_in set = in;
                            set.l2_groups = true;
                            const ls_scan_call_plan ca = ls_scan_call_make_plan(in), cb = ls_scan_call_make_plan(set);
                            CHECK(same_call(ca, cb), "call plan moves with the field (elem %d mq_max %d bits %d nq %lld)", elem, mq_max,
                                  bits, (long long)nq);
                            for (int64_t left = nq; left > 0;) {
                                const ls_scan_launch_shape a = ls_scan_launch_make_shape(in, ca.lane_call, left, false);
                                const ls_scan_launch_shape b = ls_scan_launch_make_shape(set, cb.lane_call, left, false);
                                CHECK(same_shape(a, b), "shape moves with the field (elem %d mq_max %d bits %d left %lld): NQ %d / %d", elem,
                                      mq_max, bits, (long long)left, a.NQ, b.NQ);
                                CHECK(same_launch(ls_scan_launch_make_plan(in, a, 224, 7), ls_scan_launch_make_plan(set, b, 224, 7)),
                                      "launch plan moves with the field (elem %d mq_max %d bits %d left %lld)", elem, mq_max, bits,
                                      (long long)left);
                                left -= a.real > 0 ? a.real : 1;
                                ++cases;
                            }
                        }
    if (fails) {
        std::fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok %lld\n", cases);
    return 0;
}
