// Host check of csrc/ls_mq_plan.h: a plain program with its own main, built by tests/test_mq_plan_cpu.py with
// AddressSanitizer and UndefinedBehaviorSanitizer.
//   mq_plan_check <tests/mq_plan_parent.txt> [m k n_cu]...
// 1. The table holds what the four plan functions this header replaced answered, input for input; the header is held to it
//    row for row. The one permitted difference: an fp32 plan that declined with workgroups and k' still set is all zeros
//    now - printed as "zeroed ..." and counted.
// 2. Its own sweep, for all four kinds: what every launch relies on (the launchers' argument check and LDS ceilings), all
//    zeros on decline, every switch of a kind's predicate alone declines, the forced workgroup and k' ranges, the group
//    arithmetic, the LDS facts the plan quotes.
// 3. "defect <kind> <rows> <k> <n_cu>" for every (kind, rows, k, n_cu) of the table where a group size the grouping rule produces has
//    no plan although the pass is granted.
// 4. The row-list plan of every "m k n_cu" triple of the command line as "m k n_cu blocks kprime keys", for the
//    restatement in tests/mq_subset_shapes.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>

#include "ls_mq_plan.h"

static int fails = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            ++fails;                           \
            std::fprintf(stderr, "FAIL %s: ", #c); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
        }                                      \
    } while (0)

static const int NQS[] = {1, 2, 16, 17, 32};

static ls_mq_in on(int kind, int n_cu, int chunks = 0) {
    ls_mq_in in{};
    in.kind = kind;
    in.opt_in = in.multi_query = in.mq = in.mq32 = in.f32 = in.single_device = true;
    in.n_cu = n_cu;
    in.max_blocks = 4 * n_cu;
    in.chunks = chunks ? chunks : (kind == LS_MQ_SQ8 ? 24 : 96);
    return in;
}

// the workgroup's LDS and its ceiling, as the kind's launcher computes them
static size_t lds_bytes(const ls_mq_in& in, int keys, int nq) {
    const int nb = nq > LS_MQ_NQ ? 2 : 1;
    return in.kind == LS_MQ_F16   ? mq16_lds_bytes(in.chunks, keys, nb)
           : in.kind == LS_MQ_SQ8 ? mq8_lds_bytes(in.chunks, keys)
                                  : mq_lds_bytes(in.chunks, keys, nb, ls_mq_plan_waves(in.kind, nq));
}
static size_t lds_max(const ls_mq_in& in, int nq) {
    if (nq <= LS_MQ_NQ) return LS_PIGGY_LDS_MAX;
    return in.kind == LS_MQ_F16 ? LS_MQ16_LDS_MAX2 : LS_MQ_LDS_MAX2;
}

static void check_plan(const ls_mq_in& in, int64_t m, int32_t k, int nq) {
    const ls_mq_plan p = ls_mq_make_plan(in, m, k, nq);
    const long long mm = (long long)m;
    if (p.keys == 0) {
        CHECK(p.blocks == 0 && p.kprime == 0, "declined plan not all zeros (kind %d m %lld k %d)", in.kind, mm, k);
        return;
    }
    const int waves = ls_mq_plan_waves(in.kind, nq);
    const int64_t c_stride = (int64_t)in.max_blocks * LS_KP_MAX, b_stride = in.max_blocks;  // (the handle's strides)
    CHECK(m >= LS_MQ_MIN_ROWS, "served below the row threshold (m %lld)", mm);
    CHECK(p.keys == 3 || p.keys == 5 || p.keys == 8, "keys %d", p.keys);
    CHECK(p.blocks >= 1 && p.blocks <= b_stride, "blocks %d of %d (m %lld k %d)", p.blocks, in.max_blocks, mm, k);
    CHECK((m + 15) / 16 >= 1, "no tile (m %lld)", mm);
    CHECK(p.kprime >= 1 && p.kprime + 1 <= LS_MQ_KP_MAX, "kprime %d", p.kprime);
    CHECK(p.kprime + 1 <= waves * p.keys, "kprime %d + 1 of %d x %d keys", p.kprime, waves, p.keys);
    CHECK((int64_t)p.blocks * p.kprime <= c_stride, "kprime %d x %d blocks past the stride %lld", p.kprime, p.blocks,
          (long long)c_stride);
    CHECK(lds_bytes(in, p.keys, nq) <= lds_max(in, nq), "kind %d: %zu bytes of LDS for %d-chunk rows, %d queries", in.kind,
          lds_bytes(in, p.keys, nq), in.chunks, nq);
    if (in.opt_blocks > 0)
        CHECK(p.blocks == std::min(in.opt_blocks, in.max_blocks), "forced blocks %d -> %d", in.opt_blocks, p.blocks);
    else  // automatic workgroups: at most one per CU, a quarter of the stride's room - the stride clamp cannot bind
        CHECK(p.blocks <= in.n_cu && c_stride / p.blocks >= LS_MQ_KP_MAX - 1, "the stride clamp binds at %d blocks", p.blocks);
    if (in.opt_kprime > 0) CHECK(p.kprime <= in.opt_kprime, "forced kprime %d -> %d", in.opt_kprime, p.kprime);
}

// the switches of ls_mq_in, and whether kind `kind`'s predicate reads them
static bool* switch_of(ls_mq_in& x, int i) {
    return i == 0 ? &x.opt_in : i == 1 ? &x.multi_query : i == 2 ? &x.mq : i == 3 ? &x.f32 : &x.single_device;
}
static bool switch_read(int kind, int i) {
    return i == 1 || kind == LS_MQ_ROWLIST || (i == 0 && kind != LS_MQ_F32) || (i == 2 && kind == LS_MQ_F32);
}

static int table_rows = 0, zeroed = 0;
static std::set<std::tuple<int, long long, int, int>> defects;

static void check_table(const char* path) {
    FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr, "cannot open %s", path);
    if (!f) return;
    char line[512];
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        int kind, k, cu, chunks, mq32, qpp, old[5][3];
        long long rows;
        const int got = std::sscanf(line, "%d %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &kind, &rows, &k,
                                    &cu, &chunks, &mq32, &qpp, &old[0][0], &old[0][1], &old[0][2], &old[1][0], &old[1][1],
                                    &old[1][2], &old[2][0], &old[2][1], &old[2][2], &old[3][0], &old[3][1], &old[3][2],
                                    &old[4][0], &old[4][1], &old[4][2]);
        CHECK(got == 22 && kind >= 0 && kind <= LS_MQ_ROWLIST, "table line: %s", line);
        if (got != 22) continue;
        ++table_rows;
        ls_mq_in in = on(kind, cu, chunks);
        in.mq32 = mq32 != 0;
        const int mq_max = ls_mq_max_queries(in, rows, k);
        CHECK(mq_max == qpp, "queries per pass %d, the parent's %d: %s", mq_max, qpp, line);
        for (int i = 0; i < 5; ++i) {
            const ls_mq_plan p = ls_mq_make_plan(in, rows, k, NQS[i]);
            const int* o = old[i];
            // the table sweeps the row length for fp16 and sq8 and debug option 22 for fp32: no other kind's rule reads them
            ls_mq_in y = in;
            if (kind == LS_MQ_F32 || kind == LS_MQ_ROWLIST) y.chunks = in.chunks == 16 ? 256 : 16;
            if (kind != LS_MQ_F32) y.mq32 = !in.mq32;
            const ls_mq_plan py = ls_mq_make_plan(y, rows, k, NQS[i]);
            CHECK(py.blocks == p.blocks && py.kprime == p.kprime && py.keys == p.keys, "kind %d reads chunks / option 22: %s", kind, line);
            if (kind == LS_MQ_F32 && o[2] == 0 && (o[0] != 0 || o[1] != 0)) {  // declined with workgroups and k' set
                CHECK(p.blocks == 0 && p.kprime == 0 && p.keys == 0, "not zeroed: %s", line);
                ++zeroed;
                std::printf("zeroed %d %lld %d %d %d %d nq %d (was %d %d 0)\n", kind, rows, k, cu, chunks, mq32, NQS[i], o[0], o[1]);
            } else {
                CHECK(p.blocks == o[0] && p.kprime == o[1] && p.keys == o[2], "nq %d: %d %d %d, the parent's: %s", NQS[i],
                      p.blocks, p.kprime, p.keys, line);
            }
            check_plan(in, rows, k, NQS[i]);
        }
        // every group size the grouping rule produces for this (index, k) where a pass is granted needs a plan
        for (int64_t left = 1; left <= 2 * mq_max + 2; ++left) {
            const int g = kind == LS_MQ_ROWLIST ? ls_mq_subset_group(left) : ls_mq_group_size(in, left, mq_max);
            const bool pass = mq_max > 0 && (kind == LS_MQ_ROWLIST ? g > 0 : left >= 2 || kind == LS_MQ_F16);
            if (pass && ls_mq_make_plan(in, rows, k, g).keys == 0) defects.insert({kind, rows, k, cu});
        }
    }
    std::fclose(f);
}

int main(int argc, char** argv) {
    CHECK(argc >= 2, "usage: mq_plan_check <parent table> [m k n_cu]...");
    if (argc >= 2) check_table(argv[1]);
    CHECK(table_rows > 700, "the table has %d rows", table_rows);
    for (const auto& d : defects)
        std::printf("defect %d %lld %d %d\n", std::get<0>(d), std::get<1>(d), std::get<2>(d), std::get<3>(d));

    const int64_t ms[] = {1, 4095, 4096, 4097, 6000, 200000, 12500000};
    const int32_t ks[] = {1, 10, 50, 150, 1000, 2048};
    const int cus[] = {8, 256};
    int served = 0, declined = 0;
    for (int kind = 0; kind <= LS_MQ_ROWLIST; ++kind)
        for (int cu : cus)
            for (int64_t m : ms)
                for (int32_t k : ks)
                    for (int nq : {16, 32}) {
                        const ls_mq_in in = on(kind, cu);
                        check_plan(in, m, k, nq);
                        const ls_mq_plan base = ls_mq_make_plan(in, m, k, nq);
                        (base.keys ? served : declined)++;
                        if (m < LS_MQ_MIN_ROWS) CHECK(base.keys == 0, "m %lld is below the threshold", (long long)m);
                        // every switch of the kind's predicate, alone, declines - and leaves all zeros; the others are not read
                        for (int off = 0; off < 5; ++off) {
                            ls_mq_in x = in;
                            *switch_of(x, off) = false;
                            const ls_mq_plan p = ls_mq_make_plan(x, m, k, nq);
                            if (switch_read(kind, off))
                                CHECK(p.blocks == 0 && p.kprime == 0 && p.keys == 0, "kind %d: switch %d off still serves (m %lld k %d)",
                                      kind, off, (long long)m, k);
                            else
                                CHECK(p.blocks == base.blocks && p.kprime == base.kprime && p.keys == base.keys,
                                      "kind %d reads switch %d (m %lld k %d)", kind, off, (long long)m, k);
                        }
                        // debug option 7 (workgroups) and 0 (k'), in range and past it
                        for (int ob : {1, 3, 4 * cu, 4 * cu + 100})
                            for (int ok : {0, 1, 100}) {
                                ls_mq_in x = in;
                                x.opt_blocks = ob;
                                x.opt_kprime = ok;
                                check_plan(x, m, k, nq);
                            }
                    }
    CHECK(served > 0 && declined > 0, "the sweep must see both outcomes (%d served, %d declined)", served, declined);
    // the row-list plan takes no query count: a call's groups all launch with it. The groups: min(left, 16) while two or
    // more queries are left, a lone rest is not a pass
    for (int64_t nq = 1; nq <= 40; ++nq) {
        int passes = 0;
        int64_t left = nq;
        while (const int g = ls_mq_subset_group(left)) {
            CHECK(g >= 2 && g <= LS_MQ_NQ && g <= left, "group %d of %lld", g, (long long)left);
            left -= g;
            ++passes;
        }
        CHECK(left == 0 || left == 1, "rest %lld", (long long)left);
        const int want = (int)(nq / 16) + ((nq % 16) >= 2 ? 1 : 0);
        CHECK(passes == want, "nq %lld: %d passes, %d expected", (long long)nq, passes, want);
    }
    // the scan path's groups: they use up the call, a pass carries at most mq_max, and the count is their number
    for (int kind = 0; kind < LS_MQ_ROWLIST; ++kind)
        for (int mq_max : {0, 16, 32})
            for (int64_t nq = 1; nq <= 70; ++nq) {
                const ls_mq_in in = on(kind, 256);
                int64_t left = nq;
                while (left > 0) {
                    const int g = ls_mq_group_size(in, left, mq_max);
                    CHECK(g >= 1 && g <= left && g <= std::max(mq_max, kind == LS_MQ_SQ8 ? 1 : 8), "kind %d: group %d of %lld", kind,
                          g, (long long)left);
                    left -= g;
                }
            }
    CHECK(ls_mq_group_count(on(LS_MQ_F32, 256), 200000, 10, 70) == 3, "70 queries: 32 + 32 + 6");
    CHECK(ls_mq_group_count(on(LS_MQ_SQ8, 256), 200000, 10, 18) == 2, "18 queries on sq8: 16 + 2");
    CHECK(ls_mq_group_count(on(LS_MQ_F32, 256), 1000, 10, 13) == 2, "13 queries on the VALU scan: 8 + 5");

    // the LDS facts the plan quotes. Two blocks of fp16 queries fill their CU exactly for the 3 KB and 4 KB rows ...
    for (int ch : {16, 32, 48, 64, 96, 128, 192, 256})
        CHECK((mq16_lds_bytes(ch, 8, 2) + LS_PIGGY_LDS_MAX > 160 * 1024) == (ch >= 192), "fp16 rows of %d chunks", ch);
    // ... and 16 prepared sq8 queries fit for rows of 64 chunks, the plan's limit, and not for the next length
    CHECK(mq8_lds_bytes(64, 8) <= LS_PIGGY_LDS_MAX && mq8_lds_bytes(96, 8) > LS_PIGGY_LDS_MAX, "sq8 rows: %zu / %zu bytes",
          mq8_lds_bytes(64, 8), mq8_lds_bytes(96, 8));
    CHECK(ls_mq_make_plan(on(LS_MQ_SQ8, 256, 64), 200000, 10, 16).keys == 3 && ls_mq_make_plan(on(LS_MQ_SQ8, 256, 96), 200000, 10, 16).keys == 0,
          "the sq8 row limit");

    // 4100 rows on 256 CUs (the GPU tests' dispatch sweeps): k = 10, 30, 100 select 3, 5 and 8 keys per lane for every
    // kind, with four waves (33 workgroups) and with eight (17); k = 300 declines - but for the row list, which widens
    // to 65 workgroups of one tile per wave and serves it with 8
    for (int kind = 0; kind <= LS_MQ_ROWLIST; ++kind)
        for (int nq : {16, 32}) {
            const int32_t k4[] = {10, 30, 100, 300};
            const int want[] = {3, 5, 8, kind == LS_MQ_ROWLIST ? 8 : 0};
            for (int i = 0; i < 4; ++i) {
                const ls_mq_plan p = ls_mq_make_plan(on(kind, 256), 4100, k4[i], nq);
                CHECK(p.keys == want[i], "kind %d nq %d k %d: %d keys", kind, nq, k4[i], p.keys);
                if (i < 3) CHECK(p.blocks == (ls_mq_plan_waves(kind, nq) == 8 ? 17 : 33), "kind %d nq %d: %d workgroups", kind, nq, p.blocks);
            }
        }

    for (int i = 2; i + 2 < argc; i += 3) {
        const int64_t m = std::atoll(argv[i]);
        const int32_t k = std::atoi(argv[i + 1]);
        const int cu = std::atoi(argv[i + 2]);
        const ls_mq_plan p = ls_mq_make_plan(on(LS_MQ_ROWLIST, cu), m, k, LS_MQ_NQ);
        std::printf("%lld %d %d %d %d %d\n", (long long)m, k, cu, p.blocks, p.kprime, p.keys);
    }
    if (fails) {
        std::fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok %d served %d declined %d table rows %d zeroed\n", served, declined, table_rows, zeroed);
    return 0;
}
