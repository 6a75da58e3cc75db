// Host check of csrc/ls_ivf_subset_plan.h (compiled with -fsanitize=address,undefined and run by
// tests/test_ivf_subset_cpu.py): the compaction of an IVF subset over n = 3001 rows in 37 lists - two of them empty,
// one of a single row, one holding a third of the rows - against a brute-force restatement, for seven selections.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ls_ivf_subset_plan.h"

static const int64_t N = 3001;
static const int32_t NLIST = 37;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*: any fixed sequence will do
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static void set_bit(std::vector<uint8_t>& bm, int64_t r) { bm[(size_t)(r >> 3)] |= (uint8_t)(1u << (r & 7)); }

static int fail(const std::string& what, const char* msg, long long a = 0, long long b = 0) {
    std::printf("%s: %s (%lld, %lld)\n", what.c_str(), msg, a, b);
    return 1;
}

static int check(const std::string& what, const std::vector<int32_t>& assign, const std::vector<uint32_t>& off,
                 const std::vector<uint8_t>& bm, int64_t nbytes, int64_t want_m) {
    ls_ivf_subset_plan plan;
    ls_ivf_subset_compact(assign.data(), N, NLIST, off.data(), nbytes ? bm.data() : nullptr, nbytes, plan);
    // the restatement: list after list, original rows ascending; the storage row of a row is its list's first storage
    // row plus the rows of the list before it
    std::vector<uint32_t> srow, sid, soff(1, 0);
    std::vector<int64_t> counts;
    for (int32_t l = 0; l < NLIST; ++l) {
        uint32_t s = off[(size_t)l];
        int64_t c = 0;
        for (int64_t r = 0; r < N; ++r) {
            if (assign[(size_t)r] != l) continue;
            const bool sel = (r >> 3) < nbytes && ((bm[(size_t)(r >> 3)] >> (r & 7)) & 1);
            if (sel) {
                srow.push_back(s);
                sid.push_back((uint32_t)r);
                ++c;
            }
            ++s;
        }
        if (s != off[(size_t)l + 1]) return fail(what, "the test's own storage offsets are off", l, s);
        counts.push_back(c);
        soff.push_back((uint32_t)srow.size());
    }
    if (plan.m != (int64_t)srow.size() || plan.m != want_m) return fail(what, "m", plan.m, want_m);
    if (plan.soff != soff) return fail(what, "soff is not the prefix of the per-list counts");
    if (plan.srow != srow) return fail(what, "srow differs");
    if (plan.sid != sid) return fail(what, "sid differs");
    for (int32_t l = 0; l < NLIST; ++l)
        for (uint32_t x = plan.soff[(size_t)l] + 1; x < plan.soff[(size_t)l + 1]; ++x)
            if (plan.sid[x - 1] >= plan.sid[x] || plan.srow[x - 1] >= plan.srow[x])
                return fail(what, "a list is not ascending", l, x);
    if (plan.top_rows.size() != (size_t)NLIST + 1 || plan.top_rows[0] != 0) return fail(what, "top_rows shape");
    std::vector<int64_t> left(counts);
    int64_t sum = 0;
    for (int32_t p = 1; p <= NLIST; ++p) {  // the p-th largest by repeated extraction
        size_t best = 0;
        for (size_t i = 1; i < left.size(); ++i)
            if (left[i] > left[best]) best = i;
        sum += left[best];
        left[best] = -1;
        if (plan.top_rows[(size_t)p] != sum) return fail(what, "top_rows", p, sum);
    }
    if (plan.top_rows[(size_t)NLIST] != plan.m) return fail(what, "top_rows[nlist] != m");
    return 0;
}

int main() {
    // lists 0 and 20 empty, list 36 one row, list 7 a third of the rows, the rest spread over the other lists
    std::vector<int32_t> assign((size_t)N);
    std::vector<int32_t> others;
    for (int32_t l = 0; l < NLIST; ++l)
        if (l != 0 && l != 7 && l != 20 && l != 36) others.push_back(l);
    for (int64_t r = 0; r < N; ++r) assign[(size_t)r] = others[rnd() % others.size()];
    int64_t in7 = 0;
    while (in7 < N / 3) {
        const size_t r = rnd() % N;
        if (assign[r] != 7) {
            assign[r] = 7;
            ++in7;
        }
    }
    for (;;) {
        const size_t r = rnd() % N;
        if (assign[r] != 7) {
            assign[r] = 36;
            break;
        }
    }
    std::vector<uint32_t> off((size_t)NLIST + 1, 0);
    for (int64_t r = 0; r < N; ++r) off[(size_t)assign[(size_t)r] + 1]++;
    for (int32_t l = 0; l < NLIST; ++l) off[(size_t)l + 1] += off[(size_t)l];
    if (off[1] != 0 || off[21] != off[20] || off[37] - off[36] != 1 || off[8] - off[7] != N / 3 || off[37] != N) {
        std::printf("the assignment does not have the intended shape\n");
        return 1;
    }

    const int64_t full = (N + 7) / 8;
    int cases = 0;
    {  // all: every byte 0xFF and four bytes more - bits at r >= n are ignored
        std::vector<uint8_t> bm((size_t)full + 4, 0xFF);
        if (check("all", assign, off, bm, full + 4, N)) return 1;
        ++cases;
    }
    {  // none: an empty bitmap, and a bitmap of zeros
        std::vector<uint8_t> bm((size_t)full, 0);
        if (check("none (no bytes)", assign, off, bm, 0, 0)) return 1;
        if (check("none (zeros)", assign, off, bm, full, 0)) return 1;
        ++cases;
    }
    {  // one row
        std::vector<uint8_t> bm((size_t)full, 0);
        set_bit(bm, 1234);
        if (check("one", assign, off, bm, full, 1)) return 1;
        ++cases;
    }
    {  // 10 % random
        std::vector<uint8_t> bm((size_t)full, 0);
        int64_t m = 0;
        for (int64_t r = 0; r < N; ++r)
            if (rnd() % 10 == 0) {
                set_bit(bm, r);
                ++m;
            }
        if (check("ten percent", assign, off, bm, full, m)) return 1;
        ++cases;
    }
    {  // all of one list, and everything but that list
        std::vector<uint8_t> in((size_t)full, 0), out((size_t)full, 0);
        for (int64_t r = 0; r < N; ++r) set_bit(assign[(size_t)r] == 7 ? in : out, r);
        if (check("list 7", assign, off, in, full, N / 3)) return 1;
        if (check("all but list 7", assign, off, out, full, N - N / 3)) return 1;
        cases += 2;
    }
    {  // a bitmap shorter than n: rows past it are not selected
        std::vector<uint8_t> bm(100, 0xFF);
        if (check("short", assign, off, bm, 100, 800)) return 1;
        ++cases;
    }
    std::printf("OK %d selections\n", cases);
    return 0;
}
