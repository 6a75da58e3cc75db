// Host check of csrc/ls_range_plan.h (built with -fsanitize=address,undefined by tests/test_range_cpu.py): a model of
// ls_range.hip's three launches - count, offsets, emit - that takes every index from the plan header, thread by thread,
// against a sequential threshold scan. For every (n, G, hit mask): every hit lands in exactly one slot, a query's slots
// are dense and ascending in the row, the totals match, no load starts at a row >= n or ends outside the allocation.
#include "ls_range_plan.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            std::printf("FAIL %s:%d: %s (case %s)\n", __FILE__, __LINE__, #c, g_case); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static char g_case[128] = "";

struct Out {
    std::vector<long long> lims, rows;
    std::vector<float> scores;
};

// ballots of wave `wave` of the workgroup of (slab, q): exactly what ls_range_look + __ballot give
static void wave_ballots(const std::vector<float>& S, long long stride, long long n, long long q, long long slab,
                         int wave, float radius, unsigned long long* b) {
    for (int c = 0; c < LS_RANGE_VEC; ++c) b[c] = 0;
    for (int lane = 0; lane < LS_RANGE_WAVE; ++lane) {
        const int tid = wave * LS_RANGE_WAVE + lane;
        const long long r0 = ls_range_row0(slab, tid);
        if (r0 >= n) continue;
        CHECK(r0 % LS_RANGE_VEC == 0 && r0 + LS_RANGE_VEC <= stride);  // the 16-byte load stays inside the vector
        for (int c = 0; c < LS_RANGE_VEC; ++c)
            if (r0 + c < n && ls_range_hit(S[(size_t)(q * stride + r0 + c)], radius)) b[c] |= 1ull << lane;
    }
}

static Out model(const std::vector<float>& S, long long stride, long long n, int G, float radius) {
    const long long nslab = ls_range_slabs(n);
    std::vector<uint32_t> cnt((size_t)(G * nslab), 0xdeadbeefu);
    // ---- count: one workgroup per (slab, query)
    for (long long q = 0; q < G; ++q)
        for (long long slab = 0; slab < nslab; ++slab) {
            uint32_t wt[LS_RANGE_WAVES];
            for (int w = 0; w < LS_RANGE_WAVES; ++w) {
                unsigned long long b[LS_RANGE_VEC];
                wave_ballots(S, stride, n, q, slab, w, radius, b);
                wt[w] = ls_range_wave_total(b);
            }
            cnt[(size_t)(q * nslab + slab)] = ls_range_slab_total(wt);
        }
    // ---- offsets: one workgroup per query, thread t owns slabs [seg_begin, seg_end)
    std::vector<long long> off((size_t)(G * nslab), -1), total((size_t)G, -1);
    for (long long q = 0; q < G; ++q) {
        long long part[LS_RANGE_OFF_THREADS];
        long long covered = 0;
        for (int t = 0; t < LS_RANGE_OFF_THREADS; ++t) {
            const long long b = ls_range_seg_begin(nslab, t), e = ls_range_seg_end(nslab, t);
            CHECK(b == covered && e >= b && e <= nslab);  // contiguous, in order, inside
            covered = e;
            part[t] = 0;
            for (long long i = b; i < e; ++i) part[t] += cnt[(size_t)(q * nslab + i)];
        }
        CHECK(covered == nslab);
        for (int o = 1; o < LS_RANGE_OFF_THREADS; o <<= 1) {  // the kernel's inclusive scan, step by step
            long long x[LS_RANGE_OFF_THREADS];
            for (int t = 0; t < LS_RANGE_OFF_THREADS; ++t) x[t] = t >= o ? part[t - o] : 0;
            for (int t = 0; t < LS_RANGE_OFF_THREADS; ++t) part[t] += x[t];
        }
        for (int t = 0; t < LS_RANGE_OFF_THREADS; ++t) {
            long long run = t ? part[t - 1] : 0;
            for (long long i = ls_range_seg_begin(nslab, t); i < ls_range_seg_end(nslab, t); ++i) {
                off[(size_t)(q * nslab + i)] = run;
                run += cnt[(size_t)(q * nslab + i)];
            }
        }
        total[(size_t)q] = part[LS_RANGE_OFF_THREADS - 1];
    }
    // ---- the host between the waits: the queries' bases in the group's buffers, lims
    Out o;
    o.lims.assign((size_t)G + 1, 0);
    std::vector<long long> base((size_t)G);
    for (int q = 0; q < G; ++q) {
        base[(size_t)q] = o.lims[(size_t)q];
        o.lims[(size_t)q + 1] = o.lims[(size_t)q] + total[(size_t)q];
    }
    const long long all = o.lims[(size_t)G];
    o.rows.assign((size_t)all, -1);
    o.scores.assign((size_t)all, 0.0f);
    std::vector<int> written((size_t)all, 0);
    // ---- emit
    for (long long q = 0; q < G; ++q)
        for (long long slab = 0; slab < nslab; ++slab) {
            unsigned long long b[LS_RANGE_WAVES][LS_RANGE_VEC];
            uint32_t wt[LS_RANGE_WAVES];
            for (int w = 0; w < LS_RANGE_WAVES; ++w) {
                wave_ballots(S, stride, n, q, slab, w, radius, b[w]);
                wt[w] = ls_range_wave_total(b[w]);
            }
            for (int tid = 0; tid < LS_RANGE_THREADS; ++tid) {
                const int w = tid / LS_RANGE_WAVE, lane = tid % LS_RANGE_WAVE;
                const long long slot0 = base[(size_t)q] + off[(size_t)(q * nslab + slab)] + ls_range_wave_base(wt, w) +
                                        ls_range_lane_rank(b[w], lane);
                for (int c = 0; c < LS_RANGE_VEC; ++c) {
                    if (!((b[w][c] >> lane) & 1ull)) continue;
                    const long long slot = slot0 + ls_range_comp_rank(b[w], lane, c);
                    CHECK(slot >= o.lims[(size_t)q] && slot < o.lims[(size_t)q + 1]);  // inside its query's segment
                    written[(size_t)slot]++;
                    o.rows[(size_t)slot] = ls_range_row0(slab, tid) + c;
                    o.scores[(size_t)slot] = S[(size_t)(q * stride + ls_range_row0(slab, tid) + c)];
                }
            }
        }
    for (long long i = 0; i < all; ++i) CHECK(written[(size_t)i] == 1);  // dense, nothing twice
    return o;
}

static void check(const std::vector<float>& S, long long stride, long long n, int G, float radius) {
    const Out o = model(S, stride, n, G, radius);
    long long at = 0;
    for (int q = 0; q < G; ++q) {
        CHECK(o.lims[(size_t)q] == at);
        for (long long r = 0; r < n; ++r) {  // the sequential scan: rows ascending
            const float s = S[(size_t)(q * stride + r)];
            if (!(s > radius) || std::isnan(s) || !(s > -FLT_MAX)) continue;
            CHECK(at < o.lims[(size_t)q + 1]);
            CHECK(o.rows[(size_t)at] == r);
            CHECK(o.scores[(size_t)at] == s);
            ++at;
        }
        CHECK(o.lims[(size_t)q + 1] == at);  // totals match
    }
}

int main() {
    const long long slab = LS_RANGE_SLAB;
    const long long ns[] = {0, 1, 63, 64, 65, slab - 1, slab, slab + 1, 3 * slab + 17};
    const int gs[] = {1, 3, 8};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::mt19937 rng(20240607);
    int cases = 0;
    static_assert(LS_RANGE_SLAB == LS_RANGE_THREADS * LS_RANGE_VEC && LS_RANGE_THREADS % LS_RANGE_WAVE == 0, "deal");
    for (long long n : ns)
        for (int G : gs) {
            const long long stride = ls_range_stride(n);
            CHECK(stride >= n && stride % 64 == 0);
            // the vectors hold 7.0f where a row must never be read as a hit: behind n
            auto blank = [&](float v) {
                std::vector<float> S((size_t)(G * stride), 7.0f);
                for (int q = 0; q < G; ++q)
                    for (long long r = 0; r < n; ++r) S[(size_t)(q * stride + r)] = v;
                return S;
            };
            auto run = [&](const char* name, const std::vector<float>& S, float radius) {
                std::snprintf(g_case, sizeof g_case, "%s n=%lld G=%d radius=%g", name, n, G, (double)radius);
                check(S, stride, n, G, radius);
                ++cases;
            };
            run("none (all equal to the radius)", blank(1.0f), 1.0f);
            run("all", blank(2.0f), 1.0f);
            run("all, radius -inf", blank(-3.0f), -inf);
            run("radius +inf", blank(inf), inf);
            run("radius NaN", blank(2.0f), nan);
            {  // only slab edges
                std::vector<float> S = blank(0.0f);
                for (int q = 0; q < G; ++q)
                    for (long long r : {0ll, 63ll, 64ll, slab - 1, slab, slab + 1, 2 * slab - 1, 2 * slab, n - 1})
                        if (r >= 0 && r < n && (r + q) % 2 == 0) S[(size_t)(q * stride + r)] = 1.0f;
                run("slab edges", S, 0.5f);
            }
            {  // every other row; NaN, -FLT_MAX and +inf rows under radius -inf
                std::vector<float> S = blank(0.0f);
                for (int q = 0; q < G; ++q)
                    for (long long r = 0; r < n; ++r) S[(size_t)(q * stride + r)] = (r + q) % 2 ? 1.0f : -1.0f;
                run("every other row", S, 0.0f);
                for (int q = 0; q < G; ++q)
                    for (long long r = q; r < n; r += 5)
                        S[(size_t)(q * stride + r)] = r % 3 == 0 ? nan : (r % 3 == 1 ? -FLT_MAX : inf);
                run("NaN / -FLT_MAX / +inf rows", S, -inf);
                run("NaN / -FLT_MAX / +inf rows, finite radius", S, 0.0f);
            }
            {  // one slab full and the rest empty (a different slab per query)
                std::vector<float> S = blank(0.0f);
                const long long nslab = ls_range_slabs(n);
                for (int q = 0; q < G && nslab > 0; ++q)
                    for (long long r = (q % nslab) * slab; r < n && r < (q % nslab + 1) * slab; ++r)
                        S[(size_t)(q * stride + r)] = 1.0f;
                run("one slab full", S, 0.0f);
            }
            for (int rep = 0; rep < 6; ++rep) {  // random masks of several densities, radius equal to a present score
                std::vector<float> S = blank(0.0f);
                const unsigned dens[] = {1, 2, 8, 64, 1000, 3};
                for (auto& v : S) v = (float)(rng() % dens[rep]);
                run("random", S, 0.0f);
                run("random, radius just below a present score", S, std::nextafter(1.0f, 0.0f));
            }
        }
    // the split of a call's queries into groups
    for (long long nq = 0; nq <= 40; ++nq) {
        long long covered = 0;
        for (long long g = 0; g < ls_range_groups(nq); ++g) {
            const int sz = ls_range_group_size(nq, g);
            std::snprintf(g_case, sizeof g_case, "groups nq=%lld", nq);
            CHECK(sz >= 1 && sz <= LS_RANGE_GROUP && g * LS_RANGE_GROUP == covered);
            covered += sz;
        }
        CHECK(covered == nq);
        ++cases;
    }
    std::printf("OK %d cases\n", cases);
    return 0;
}
