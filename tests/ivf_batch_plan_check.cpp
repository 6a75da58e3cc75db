// Host check of the IVF kind of csrc/ls_mq_plan.h (LS_MQ_IVF): a plain program with its own main, built by
// tests/test_ivf_batch_cpu.py with AddressSanitizer and UndefinedBehaviorSanitizer.
//   ivf_batch_plan_check [ntotal rows_q k nlist group n_cu]...
// 1. Its own sweep over rows / k / CU counts / group sizes: what the launcher's argument check and the LDS ceiling
//    rely on, all zeros on decline; declined below LS_MQ_MIN_ROWS, with the option off, for fp16 / sq8 rows and past
//    LS_IVF_BATCH_MAX_NLIST; the predicate is the plan of a group of two, and no larger group of a served shape declines.
// 2. The new kind moved nothing: the other kinds' plans do not read the new field, and their enum values stand.
// 3. The plan of every sextuple of the command line as "ntotal rows_q k nlist group n_cu served blocks kprime keys".
#include <cstdio>
#include <cstdlib>

#include "ls_mq_plan.h"

static int fails = 0;
#define CHECK(c, ...)                              \
    do {                                           \
        if (!(c)) {                                \
            ++fails;                               \
            std::fprintf(stderr, "FAIL %s: ", #c); \
            std::fprintf(stderr, __VA_ARGS__);     \
            std::fprintf(stderr, "\n");            \
        }                                          \
    } while (0)

static ls_mq_in on(int kind, int n_cu, int nlist) {
    ls_mq_in in{};
    in.kind = kind;
    in.opt_in = in.multi_query = in.mq = in.mq32 = in.f32 = in.single_device = true;
    in.n_cu = n_cu;
    in.max_blocks = 2 * n_cu;  // (the IVF handle's candidate blocks)
    in.chunks = 96;
    in.nlist = nlist;
    return in;
}

static void check_plan(const ls_mq_in& in, int64_t ntotal, int64_t rows_q, int32_t k, int g) {
    const ls_mq_plan p = ls_mq_ivf_plan(in, ntotal, rows_q, k, g);
    const long long bound = (long long)ls_mq_ivf_bound(ntotal, rows_q, g);
    CHECK(bound <= ntotal && bound <= (long long)g * rows_q && bound >= std::min<int64_t>(ntotal, rows_q), "bound %lld", bound);
    if (p.keys == 0) {
        CHECK(p.blocks == 0 && p.kprime == 0, "declined plan not all zeros (bound %lld k %d)", bound, k);
        return;
    }
    const int64_t c_stride = (int64_t)in.max_blocks * LS_KP_MAX, b_stride = in.max_blocks;
    CHECK(bound >= LS_MQ_MIN_ROWS, "served below the row threshold (bound %lld)", bound);
    CHECK(in.nlist <= LS_IVF_BATCH_MAX_NLIST, "served with %d lists", in.nlist);
    CHECK(p.keys == 3 || p.keys == 5 || p.keys == 8, "keys %d", p.keys);
    CHECK(p.blocks >= 1 && p.blocks <= b_stride && p.blocks <= in.n_cu, "blocks %d", p.blocks);
    CHECK(p.kprime >= 1 && p.kprime + 1 <= LS_MQ_KP_MAX && p.kprime + 1 <= LS_MQ_WAVES * p.keys, "kprime %d keys %d", p.kprime, p.keys);
    CHECK((int64_t)p.blocks * p.kprime <= c_stride, "kprime %d x %d blocks past the stride", p.kprime, p.blocks);
    // the selection's fast path needs blocks x k' >= min(k, rows_q) keys
    CHECK((int64_t)p.blocks * p.kprime >= std::min<int64_t>(k, rows_q), "%d x %d keys for k %d", p.blocks, p.kprime, k);
    CHECK(ls_mq_plan_lane_keys(LS_MQ_WAVES, p.blocks, (int)std::max<int64_t>(std::min<int64_t>(k, rows_q), 1)) > 0, "key rule");
    for (int ch : {16, 96, 256})
        CHECK(mq_lds_bytes(ch, p.keys, 1, LS_MQ_WAVES) <= LS_PIGGY_LDS_MAX, "%zu bytes of LDS", mq_lds_bytes(ch, p.keys, 1, LS_MQ_WAVES));
}

int main(int argc, char** argv) {
    static_assert(LS_MQ_F32 == 0 && LS_MQ_F16 == 1 && LS_MQ_SQ8 == 2 && LS_MQ_ROWLIST == 3 && LS_MQ_IVF == 4, "the kinds' values");
    const int64_t ns[] = {0, 1, 4095, 4096, 4097, 10000, 200000, 12500000};
    const int32_t ks[] = {1, 10, 50, 150, 1000, 2048};
    int served = 0, declined = 0, group_declines = 0;
    for (int cu : {8, 256})
        for (int64_t n : ns)
            for (int frac : {1, 7, 40})  // one query probes n / frac rows at most
                for (int32_t k : ks) {
                    const int64_t rq = n / frac;
                    const ls_mq_in in = on(LS_MQ_IVF, cu, 447);
                    const bool ok = ls_mq_ivf_served(in, n, rq, k);
                    CHECK(ok == (ls_mq_ivf_plan(in, n, rq, k, 2).keys > 0), "the predicate is the plan of two queries");
                    (ok ? served : declined)++;
                    if (ls_mq_ivf_bound(n, rq, 2) < LS_MQ_MIN_ROWS) CHECK(!ok, "served below the threshold (n %lld)", (long long)n);
                    for (int g = 2; g <= LS_MQ_NQ; ++g) {
                        check_plan(in, n, rq, k, g);
                        if (ok && ls_mq_ivf_plan(in, n, rq, k, g).keys == 0) ++group_declines;
                    }
                    // every switch of the predicate, alone, declines - and leaves all zeros
                    for (int off = 0; off < 4; ++off) {
                        ls_mq_in x = in;
                        if (off == 0) x.opt_in = false;
                        if (off == 1) x.f32 = false;
                        if (off == 2) x.nlist = LS_IVF_BATCH_MAX_NLIST + 1;
                        if (off == 3) x.nlist = 0;
                        const ls_mq_plan p = ls_mq_ivf_plan(x, n, rq, k, LS_MQ_NQ);
                        CHECK(p.blocks == 0 && p.kprime == 0 && p.keys == 0, "switch %d off still serves (n %lld k %d)", off, (long long)n, k);
                        CHECK(!ls_mq_ivf_served(x, n, rq, k), "switch %d off: predicate", off);
                    }
                    ls_mq_in edge = in;
                    edge.nlist = LS_IVF_BATCH_MAX_NLIST;
                    CHECK(ls_mq_ivf_served(edge, n, rq, k) == ok, "the nlist cap itself is served");
                    // the other kinds do not read nlist, and answer as they did with it unset
                    for (int kind = 0; kind <= LS_MQ_ROWLIST; ++kind)
                        for (int nq : {2, 16, 32}) {
                            ls_mq_in a = on(kind, cu, 0), b = on(kind, cu, 5000);
                            const ls_mq_plan pa = ls_mq_make_plan(a, n, k, nq), pb = ls_mq_make_plan(b, n, k, nq);
                            CHECK(pa.blocks == pb.blocks && pa.kprime == pb.kprime && pa.keys == pb.keys, "kind %d reads nlist", kind);
                        }
                }
    CHECK(served > 0 && declined > 0, "the sweep must see both outcomes (%d served, %d declined)", served, declined);
    CHECK(group_declines == 0, "%d groups of a served shape have no plan", group_declines);
    for (int i = 1; i + 5 < argc; i += 6) {
        const int64_t n = std::atoll(argv[i]), rq = std::atoll(argv[i + 1]);
        const int32_t k = std::atoi(argv[i + 2]);
        const int nlist = std::atoi(argv[i + 3]), g = std::atoi(argv[i + 4]), cu = std::atoi(argv[i + 5]);
        const ls_mq_in in = on(LS_MQ_IVF, cu, nlist);
        const ls_mq_plan p = ls_mq_ivf_plan(in, n, rq, k, g);
        std::printf("%lld %lld %d %d %d %d %d %d %d %d\n", (long long)n, (long long)rq, k, nlist, g, cu,
                    ls_mq_ivf_served(in, n, rq, k) ? 1 : 0, p.blocks, p.kprime, p.keys);
    }
    if (fails) {
        std::fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok %d served %d declined\n", served, declined);
    return 0;
}
