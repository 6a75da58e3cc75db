// Host check of csrc/ls_scan_call_plan.h: a plain program with its own main, built by tests/test_scan_call_plan_cpu.py
// with AddressSanitizer and UndefinedBehaviorSanitizer.
//   scan_call_plan_check <tests/scan_call_plan_parent.txt> [table]      ("table": part 1 only)
// 1. The table holds what the expressions this header replaced (scan_search_on_stream, csrc/ls_api.hip, at the commit the
//    table names) answered, one launch per row: the inputs, then the answers. The header is held to it row for row; no
//    difference is excused.
// 2. Its own sweep - call contexts x storage x nq x k x n x flags x stream x switches x profiling x lanes in flight x
//    keep ring full, every launch of every call - for four implications:
//      same_launch  =>  completion words and not LS_FLAG_PIPELINE
//      dev_keep     =>  no completion words
//      lane_call    =>  one query group and a repairable call
//      reserving    =>  skip_scores is false
//    and that the launch's query count is what ls_mq_group_size answers for the handle's whole ls_mq_in.
// The sweep is addressed by coordinates (point_at), so that the program that wrote the table - the parent's expressions
// pasted in, not committed - could walk it and every point's neighbours; it includes this file with
// LS_SCAN_CALL_PLAN_CHECK_NO_MAIN defined, for the sweep and the row format, and has its own main.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ls_scan_call_plan.h"

static long long fails = 0;
#define CHECK(c, ...)                              \
    do {                                           \
        if (!(c)) {                                \
            if (++fails <= 20) {                   \
                std::fprintf(stderr, "FAIL %s: ", #c); \
                std::fprintf(stderr, __VA_ARGS__); \
                std::fprintf(stderr, "\n");        \
            }                                      \
        }                                          \
    } while (0)

// ---- one launch of one call: a table row ---------------------------------------------------------------------------
#define N_IN 29   // ls_scan_call_in (25), keep_full, left, blocks, kprime
#define N_OUT 15  // call plan (5), launch shape (4), launch plan (6)
struct row {
    long long v[N_IN + N_OUT];
};
static ls_scan_call_in in_of(const row& r) {
    const long long* v = r.v;
    ls_scan_call_in in{};
    in.n = v[0], in.elem = (int)v[1], in.chunks = (int)v[2], in.s_vecs = (int)v[3];
    in.opt_lanes = (int)v[4], in.opt_overlap = v[5], in.opt_multi_query = v[6], in.opt_scan_skip_scores = v[7];
    in.opt_mq_skip_scores = v[8], in.opt_same_launch = v[9], in.profiling = v[10];
    in.has_done = v[11], in.has_retry = v[12], in.gen_forced = v[13], in.reserving = v[14], in.repairable = v[15];
    in.pipeline = v[16], in.inorder = v[17], in.stream = (unsigned)v[18];
    in.k = (int32_t)v[19], in.nq = v[20], in.mq_max = (int)v[21], in.n_groups = v[22], in.lanes_active = v[23];
    in.mq_kind = (int)v[24];
    return in;
}
static void put_in(row& r, const ls_scan_call_in& in, bool keep_full, int64_t left, int blocks, int kprime) {
    const long long v[N_IN] = {in.n, in.elem, in.chunks, in.s_vecs, in.opt_lanes, in.opt_overlap, in.opt_multi_query,
                               in.opt_scan_skip_scores, in.opt_mq_skip_scores, in.opt_same_launch, in.profiling,
                               in.has_done, in.has_retry, in.gen_forced, in.reserving, in.repairable, in.pipeline,
                               in.inorder, in.stream, in.k, in.nq, in.mq_max, in.n_groups, in.lanes_active, in.mq_kind,
                               keep_full, left, blocks, kprime};
    for (int i = 0; i < N_IN; ++i) r.v[i] = v[i];
}
// the header's answers for the row's inputs
static void answer(row& r) {
    const ls_scan_call_in in = in_of(r);
    const ls_scan_call_plan cp = ls_scan_call_make_plan(in);
    const ls_scan_launch_shape sh = ls_scan_launch_make_shape(in, cp.lane_call, r.v[26], r.v[25] != 0);
    const ls_scan_launch_plan lp = ls_scan_launch_make_plan(in, sh, (int)r.v[27], (int)r.v[28]);
    const long long o[N_OUT] = {cp.bad_groups, cp.lane_call, cp.drain_lanes, cp.ride, cp.leave_pending,
                                sh.kind, sh.NQ, sh.real, sh.repair_first,
                                lp.own_keys_cap, lp.same_launch, lp.host_words, lp.dev_keep, lp.skip_scores, lp.grow_scores};
    for (int i = 0; i < N_OUT; ++i) r.v[N_IN + i] = o[i];
}

// ---- the sweep -----------------------------------------------------------------------------------------------------
// The handle the sweep imagines: 256 CUs, candidate blocks for two workgroups per CU, rows of d = 1024.
struct sweep_point {
    ls_scan_call_in in;
    ls_mq_in mq;
    bool keep_full;
    int L, V;
};
static const int64_t NS[] = {0, 1, 4095, 4096, 200000, (LS_LANE_MIN_BYTES + 4095) / 4096};  // (the last: 1024 x fp32 rows past LS_LANE_MIN_BYTES)
static const int64_t NQS[] = {1, 2, 3, 5, 8, 16, 17, 32};
static const int32_t KS[] = {1, 50, 256, 257, 1000};
// call contexts {has_done, has_retry, gen_forced, reserving}: a device-output call (ls_search_device, a shard's
// sub-search, the batched repair), a host call overlapped / exclusive, its retry, mq_repair, and the batched repair
// under a host call (a retry list without completion words)
static const bool CTX[][4] = {{0, 0, 0, 0}, {1, 1, 1, 0}, {1, 1, 0, 0}, {1, 0, 1, 1}, {0, 0, 0, 1}, {0, 1, 0, 0}};
static const unsigned STREAMS[] = {0u, LS_STREAM_OWN, LS_STREAM_LANE, LS_STREAM_LANES_CALLER, LS_STREAM_OWN | LS_STREAM_LANES_CALLER};
#define N_VARIANTS 13  // the defaults, then every switch at its other value(s), alone
// coordinates: context, dtype (fp32, fp16, sq8), variant, n, k, nq, flags (none, LS_FLAG_ASYNC, LS_FLAG_PIPELINE,
// LS_FLAG_PIPELINE | LS_FLAG_INORDER), stream, profiling, lanes in flight, keep ring full
#define N_DIMS 11
static const int DIMS[N_DIMS] = {6, 3, N_VARIANTS, 6, 5, 8, 4, 5, 2, 2, 2};

static sweep_point point_at(const int* c) {
    const bool* ctx = CTX[c[0]];
    const int dtype = c[1], variant = c[2], fl = c[6];
    const int64_t n = NS[c[3]], nq = NQS[c[5]];
    const int32_t k = KS[c[4]];
    sweep_point p{};
    ls_mq_in& mq = p.mq;
    mq.kind = dtype == 0 ? LS_MQ_F32 : dtype == 1 ? LS_MQ_F16 : LS_MQ_SQ8;
    mq.opt_in = dtype == 1 ? variant == 10 : dtype == 2 ? variant == 11 : false;  // ls_set_f16_small_batch / ls_set_sq8_small_batch
    mq.multi_query = variant != 4;
    mq.mq = variant != 8;    // debug option 16
    mq.mq32 = variant != 9;  // debug option 22
    mq.f32 = dtype == 0, mq.single_device = true;
    mq.n_cu = 256, mq.max_blocks = 512, mq.chunks = 1024 * (dtype == 0 ? 4 : dtype == 1 ? 2 : 1) / 16;
    ls_scan_call_in& in = p.in;
    in.n = n;
    in.elem = dtype == 0 ? 4 : dtype == 1 ? 2 : 1;
    in.mq_kind = mq.kind;
    in.chunks = mq.chunks;
    p.L = 64, p.V = in.chunks / 64;
    in.s_vecs = variant == 12 ? 32 : 8;
    in.opt_lanes = variant == 1 ? 0 : variant == 2 ? 2 : 1;
    in.opt_overlap = variant != 3;
    in.opt_multi_query = variant != 4;
    in.opt_scan_skip_scores = variant != 5;
    in.opt_mq_skip_scores = variant != 6;
    in.opt_same_launch = variant != 7;
    in.profiling = c[8];
    in.has_done = ctx[0], in.has_retry = ctx[1], in.gen_forced = ctx[2], in.reserving = ctx[3];
    in.pipeline = fl >= 2, in.inorder = fl == 3;
    // (only ls_search_device makes a call repairable, from its flags)
    in.repairable = !(ctx[0] || ctx[1] || ctx[2] || ctx[3]) && ls_scan_call_repairable(in.pipeline, fl == 1, in.inorder);
    in.stream = STREAMS[c[7]];
    in.k = k, in.nq = nq;
    in.lanes_active = c[9];
    // (the two plan questions depend on five coordinates only: asked once each)
    static int mq_max_of[3][N_VARIANTS][6][5];
    static int64_t n_groups_of[3][N_VARIANTS][6][5][8];
    static bool asked[3][N_VARIANTS][6][5][8];
    if (!asked[dtype][variant][c[3]][c[4]][c[5]]) {
        asked[dtype][variant][c[3]][c[4]][c[5]] = true;
        mq_max_of[dtype][variant][c[3]][c[4]] = ls_mq_max_queries(mq, n, k);
        n_groups_of[dtype][variant][c[3]][c[4]][c[5]] = ls_mq_group_count(mq, n, k, nq);
    }
    in.mq_max = mq_max_of[dtype][variant][c[3]][c[4]];
    in.n_groups = n_groups_of[dtype][variant][c[3]][c[4]][c[5]];
    p.keep_full = c[10];
    return p;
}

template <typename F>
static void sweep(F&& f) {  // f(point, its coordinates), the last coordinate fastest
    int c[N_DIMS] = {};
    for (;;) {
        f(point_at(c), c);
        int d = N_DIMS - 1;
        while (d >= 0 && ++c[d] == DIMS[d]) c[d--] = 0;
        if (d < 0) return;
    }
}

// every launch of the call at p, as the scheduling loop walks them: g(row with the inputs filled in)
template <typename G>
static void launches(const sweep_point& p, G&& g) {
    const ls_scan_call_in& in = p.in;
    const int64_t keff = std::min<int64_t>(in.k, in.n);
    const int scan_blocks = ls_scan_blocks_lv(in.n > 0 ? in.n : 1, p.L, p.V, p.mq.n_cu);
    const int scan_kprime = ls_kprime(scan_blocks, (int)std::max<int64_t>(keff, 1), LS_KP_MAX);
    const ls_scan_call_plan cp = ls_scan_call_make_plan(in);
    for (int64_t left = in.nq; left > 0;) {
        const ls_scan_launch_shape sh = ls_scan_launch_make_shape(in, cp.lane_call, left, p.keep_full);
        const ls_mq_plan mp = sh.kind != LS_K_SCAN ? ls_mq_make_plan(p.mq, in.n, in.k, sh.NQ) : ls_mq_plan{0, 0, 0};
        if (sh.kind != LS_K_SCAN)
            CHECK(sh.NQ == ls_mq_group_size(p.mq, left, in.mq_max), "NQ %d, the handle's ls_mq_in groups %d", sh.NQ,
                  ls_mq_group_size(p.mq, left, in.mq_max));
        row r{};
        put_in(r, in, p.keep_full, left, sh.kind != LS_K_SCAN ? mp.blocks : scan_blocks, sh.kind != LS_K_SCAN ? mp.kprime : scan_kprime);
        g(r);
        if (sh.real < 1) break;
        left -= sh.real;
    }
}

#ifndef LS_SCAN_CALL_PLAN_CHECK_NO_MAIN
int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: scan_call_plan_check <table>\n");
        return 2;
    }
    // 1. the table
    FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    long long table_rows = 0;
    char line[1024];
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        row want{};
        char* s = line;
        int got = 0;
        for (; got < N_IN + N_OUT; ++got) {
            char* e = nullptr;
            want.v[got] = std::strtoll(s, &e, 10);
            if (e == s) break;
            s = e;
        }
        CHECK(got == N_IN + N_OUT, "table row %lld has %d numbers", table_rows + 1, got);
        if (got != N_IN + N_OUT) continue;
        ++table_rows;
        row have = want;
        answer(have);
        for (int i = N_IN; i < N_IN + N_OUT; ++i)
            CHECK(have.v[i] == want.v[i], "table row %lld, answer %d: %lld, the table says %lld", table_rows, i - N_IN,
                  have.v[i], want.v[i]);
    }
    std::fclose(f);
    CHECK(table_rows >= 500, "only %lld table rows", table_rows);
    if (argc > 2 && std::string(argv[2]) == "table") {
        if (fails) std::fprintf(stderr, "%lld failures\n", fails);
        else std::printf("ok %lld table rows\n", table_rows);
        return fails ? 1 : 0;
    }
    // 2. the implications, over every launch of the sweep
    long long calls = 0, rows = 0, n_same = 0, n_keep = 0, n_lane = 0, n_skip = 0;
    sweep([&](const sweep_point& p, const int*) {
        ++calls;
        launches(p, [&](row& r) {
            ++rows;
            answer(r);
            const ls_scan_call_in in = in_of(r);
            const bool lane_call = r.v[N_IN + 1], same_launch = r.v[N_IN + 10], dev_keep = r.v[N_IN + 12], skip_scores = r.v[N_IN + 13];
            n_same += same_launch, n_keep += dev_keep, n_lane += lane_call, n_skip += skip_scores;
            CHECK(!same_launch || (in.has_done && !in.pipeline), "same_launch without completion words or pipelined");
            CHECK(!dev_keep || !in.has_done, "dev_keep with completion words");
            CHECK(!lane_call || (in.n_groups == 1 && in.repairable), "lane_call of %lld groups, repairable %d", (long long)in.n_groups, in.repairable);
            CHECK(!in.reserving || !skip_scores, "a reserving context skips its score vectors");
        });
    });
    CHECK(n_same > 0 && n_keep > 0 && n_lane > 0 && n_skip > 0, "the sweep never reaches an answer (%lld %lld %lld %lld)", n_same,
          n_keep, n_lane, n_skip);
    if (fails) {
        std::fprintf(stderr, "%lld failures\n", fails);
        return 1;
    }
    std::printf("ok %lld table rows, %lld calls, %lld launches\n", table_rows, calls, rows);
    return 0;
}
#endif
