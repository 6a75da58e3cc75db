// Host check of csrc/ls_mq_subset_plan.h: a plain program with its own main, built by tests/test_mq_subset_cpu.py with
// AddressSanitizer and UndefinedBehaviorSanitizer. It sweeps subset sizes x k x CU counts (and the debug options that
// force the workgroup count and k') and checks what every launch of a subset pass relies on; then it prints the plan of
// every "m k n_cu" triple given on the command line as "m k n_cu blocks kprime keys", for the test's restatement.
#include <cstdio>
#include <cstdlib>

#include "ls_mq_subset_plan.h"

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

static ls_mq_subset_in on(int n_cu) {
    ls_mq_subset_in in{};
    in.enabled = in.multi_query = in.mq = in.f32 = in.single_device = true;
    in.n_cu = n_cu;
    in.max_blocks = 4 * n_cu;
    return in;
}

static void check_plan(const ls_mq_subset_in& in, int64_t m, int32_t k) {
    const ls_mq_subset_plan p = ls_mq_subset_make_plan(in, m, k);
    const long long mm = (long long)m;
    if (p.keys == 0) {
        CHECK(p.blocks == 0 && p.kprime == 0, "declined plan not all zeros (m %lld k %d)", mm, k);
        return;
    }
    const int64_t stride = (int64_t)in.max_blocks * LS_KP_MAX;
    CHECK(m >= LS_MQ_MIN_ROWS, "served below the row threshold (m %lld)", mm);
    CHECK(p.keys == 3 || p.keys == 5 || p.keys == 8, "keys %d", p.keys);
    CHECK(p.blocks >= 1 && p.blocks <= in.max_blocks, "blocks %d of %d (m %lld k %d)", p.blocks, in.max_blocks, mm, k);
    CHECK((m + 15) / 16 >= 1, "no tile (m %lld)", mm);
    CHECK(p.kprime >= 1 && p.kprime + 1 <= LS_MQ_KP_MAX, "kprime %d", p.kprime);
    CHECK(p.kprime + 1 <= LS_MQ_SUBSET_WAVES * p.keys, "kprime %d + 1 of %d x %d keys", p.kprime, LS_MQ_SUBSET_WAVES, p.keys);
    CHECK(p.kprime <= stride / p.blocks, "kprime %d x %d blocks past the stride %lld", p.kprime, p.blocks, (long long)stride);
    if (in.opt_blocks > 0)
        CHECK(p.blocks == std::min(in.opt_blocks, in.max_blocks), "forced blocks %d -> %d", in.opt_blocks, p.blocks);
    if (in.opt_kprime > 0) CHECK(p.kprime <= in.opt_kprime, "forced kprime %d -> %d", in.opt_kprime, p.kprime);
}

int main(int argc, char** argv) {
    const int64_t ms[] = {1, 4095, 4096, 4097, 6000, 200000, 12500000};
    const int32_t ks[] = {1, 10, 50, 150, 1000, 2048};
    const int cus[] = {8, 256};
    int served = 0, declined = 0;
    for (int cu : cus)
        for (int64_t m : ms)
            for (int32_t k : ks) {
                ls_mq_subset_in in = on(cu);
                check_plan(in, m, k);
                const ls_mq_subset_plan base = ls_mq_subset_make_plan(in, m, k);
                (base.keys ? served : declined)++;
                if (m < LS_MQ_MIN_ROWS) CHECK(base.keys == 0, "m %lld is below the threshold", (long long)m);
                // every switch of the predicate, alone, declines - and leaves all zeros
                for (int off = 0; off < 5; ++off) {
                    ls_mq_subset_in x = in;
                    (off == 0 ? x.enabled : off == 1 ? x.multi_query : off == 2 ? x.mq : off == 3 ? x.f32 : x.single_device) = false;
                    const ls_mq_subset_plan p = ls_mq_subset_make_plan(x, m, k);
                    CHECK(p.blocks == 0 && p.kprime == 0 && p.keys == 0, "switch %d off still serves (m %lld k %d)", off, (long long)m, k);
                }
                // debug option 7 (workgroups) and 0 (k'), in range and past it
                for (int ob : {1, 3, 4 * cu, 4 * cu + 100})
                    for (int ok : {0, 1, 100}) {
                        ls_mq_subset_in x = in;
                        x.opt_blocks = ob;
                        x.opt_kprime = ok;
                        check_plan(x, m, k);
                    }
                // the plan takes no query count: a call's groups all launch with it. The groups: min(left, 16) while two
                // or more queries are left, a lone rest is not a pass
                for (int64_t nq = 1; nq <= 40; ++nq) {
                    int passes = 0;
                    int64_t left = nq;
                    while (const int g = ls_mq_subset_group(left)) {
                        CHECK(g >= 2 && g <= LS_MQ_SUBSET_NQ && g <= left, "group %d of %lld", g, (long long)left);
                        left -= g;
                        ++passes;
                    }
                    CHECK(left == 0 || left == 1, "rest %lld", (long long)left);
                    const int want = (int)(nq / 16) + ((nq % 16) >= 2 ? 1 : 0);
                    CHECK(passes == want, "nq %lld: %d passes, %d expected", (long long)nq, passes, want);
                }
            }
    CHECK(served > 0 && declined > 0, "the sweep must see both outcomes (%d served, %d declined)", served, declined);
    for (int i = 1; i + 2 < argc; i += 3) {
        const int64_t m = std::atoll(argv[i]);
        const int32_t k = std::atoi(argv[i + 1]);
        const int cu = std::atoi(argv[i + 2]);
        const ls_mq_subset_plan p = ls_mq_subset_make_plan(on(cu), m, k);
        std::printf("%lld %d %d %d %d %d\n", (long long)m, k, cu, p.blocks, p.kprime, p.keys);
    }
    if (fails) {
        std::fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok %d served %d declined\n", served, declined);
    return 0;
}
