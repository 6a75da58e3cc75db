// Host check of csrc/ls_ivf_add_plan.h and csrc/ls_rows_plan.h (compiled with AddressSanitizer + UndefinedBehaviorSanitizer and run by
// tests/test_ivf_add_cpu.py). For every case the plan of "old index + one add" is compared with a from-scratch counting
// sort of the concatenated assignment - what ivf_build makes of all rows at once:
//   off_new == the counting sort's offsets;
//   ids (ls_ivf_add_id over src and the old ids) == the counting sort's ids;
//   src maps every destination to the right source: an old destination to the old STORAGE row that held the same
//       original row, a new destination to the new row with that original number;
//   shift[l] == off_new[l] - off_old[l].
// Then the row mover's deal: every (row, chunk) of the destination is moved by exactly one lane of one tile.
#include <cstdio>
#include <random>
#include <vector>

#include "ls_ivf_add_plan.h"

#define FAIL(...)                 \
    do {                          \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
        return 1;                 \
    } while (0)

struct sorted_index {  // ivf_build's counting sort
    std::vector<uint32_t> off, ids;
};

static sorted_index sort_from_scratch(const std::vector<int32_t>& assign, int nlist) {
    sorted_index s;
    s.off.assign((size_t)nlist + 1, 0);
    for (int32_t a : assign) s.off[(size_t)a + 1]++;
    for (int l = 0; l < nlist; ++l) s.off[(size_t)l + 1] += s.off[(size_t)l];
    s.ids.resize(assign.size());
    std::vector<uint32_t> at(s.off.begin(), s.off.end() - 1);
    for (size_t r = 0; r < assign.size(); ++r) s.ids[at[(size_t)assign[r]]++] = (uint32_t)r;
    return s;
}

// one add of `add` onto the index of `old`: 0, or 1 after printing what differs
static int check_add(const char* name, const std::vector<int32_t>& old, const std::vector<int32_t>& add, int nlist) {
    const sorted_index before = sort_from_scratch(old, nlist);
    std::vector<int32_t> all(old);
    all.insert(all.end(), add.begin(), add.end());
    const sorted_index want = sort_from_scratch(all, nlist);
    ls_ivf_add_plan p;
    ls_ivf_add_plan_make(before.off.data(), nlist, add.data(), (int64_t)add.size(), p);
    const uint32_t n_old = (uint32_t)old.size();
    const size_t n_new = all.size();
    if (p.off_new != want.off) FAIL("%s: off_new differs", name);
    if (p.src.size() != n_new || p.sizes.size() != (size_t)nlist || p.shift.size() != (size_t)nlist)
        FAIL("%s: table sizes", name);
    for (int l = 0; l < nlist; ++l) {
        if (p.shift[(size_t)l] != p.off_new[(size_t)l] - before.off[(size_t)l]) FAIL("%s: shift[%d]", name, l);
        if (p.off_new[(size_t)l] < before.off[(size_t)l]) FAIL("%s: list %d moves down", name, l);
        if (p.sizes[(size_t)l] != (int64_t)want.off[(size_t)l + 1] - want.off[(size_t)l]) FAIL("%s: sizes[%d]", name, l);
    }
    std::vector<int> used(n_new, 0);
    for (size_t s = 0; s < n_new; ++s) {
        const uint32_t from = p.src[s];
        if (from >= n_new) FAIL("%s: src[%zu] = %u names no row", name, s, from);
        used[from]++;
        const uint32_t id = ls_ivf_add_id(from, n_old, before.ids.data());
        if (id != want.ids[s]) FAIL("%s: ids[%zu] = %u, want %u", name, s, id, want.ids[s]);
        if (from < n_old) {  // an old storage row: it held the same original row, in the same list, shifted
            if (before.ids[from] != want.ids[s]) FAIL("%s: src[%zu] names the wrong old storage row", name, s);
            const int l = old[before.ids[from]];
            if (s != (size_t)from + p.shift[(size_t)l]) FAIL("%s: old row %u of list %d lands at %zu", name, from, l, s);
        } else if (all[from] != add[from - n_old] || want.ids[s] != from) {
            FAIL("%s: src[%zu] names the wrong new row", name, s);
        }
    }
    for (size_t r = 0; r < n_new; ++r)
        if (used[r] != 1) FAIL("%s: source %zu used %d times", name, r, used[r]);
    return 0;
}

// the row mover's enumeration: W waves, wave gw takes tiles gw, gw + W, ...
static int check_deal(long long rows, int chunks, int n_cu) {
    const int TR = ls_rows_tile_rows(chunks);
    const int blocks = ls_rows_blocks(rows, chunks, n_cu);
    if (TR < 1 || TR * (chunks < LS_ROWS_WAVE ? chunks : 1) > LS_ROWS_WAVE) FAIL("chunks=%d: %d rows per tile", chunks, TR);
    if (blocks < 1 || blocks > n_cu * LS_ROWS_WG_PER_CU) FAIL("rows=%lld chunks=%d: %d workgroups", rows, chunks, blocks);
    const long long W = (long long)blocks * (LS_ROWS_THREADS / LS_ROWS_WAVE), NT = ls_rows_tiles(rows, chunks);
    std::vector<unsigned char> seen((size_t)(rows * chunks), 0);
    for (long long gw = 0; gw < W; ++gw)
        for (long long t = gw; t < NT; t += W)
            for (int lane = 0; lane < LS_ROWS_WAVE; ++lane) {
                const int lr = ls_rows_lane_row(lane, chunks), c0 = ls_rows_lane_chunk(lane, chunks);
                if (lr >= TR) continue;
                const long long s = t * TR + lr;
                if (s >= rows) continue;
                for (int c = c0; c < chunks; c += LS_ROWS_WAVE) {
                    if (c < 0 || c >= chunks) FAIL("chunks=%d: lane %d moves chunk %d", chunks, lane, c);
                    if (seen[(size_t)(s * chunks + c)]++) FAIL("rows=%lld chunks=%d: (%lld, %d) moved twice", rows, chunks, s, c);
                }
            }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) FAIL("rows=%lld chunks=%d: chunk %zu moved %d times", rows, chunks, i, (int)seen[i]);
    return 0;
}

static std::vector<int32_t> draw(std::mt19937& rng, size_t n, int nlist) {
    std::vector<int32_t> a(n);
    for (auto& x : a) x = (int32_t)(rng() % (unsigned)nlist);
    return a;
}

int main() {
    std::mt19937 rng(20240611);
    long long cases = 0;
    // ---- the named edge cases
    {
        if (check_add("empty old index", {}, draw(rng, 50, 7), 7)) return 1;
        if (check_add("nothing and nothing", {}, {}, 3)) return 1;
        // lists 4..7 are empty before and filled by the add; lists 0..3 keep their old rows and get no new ones
        std::vector<int32_t> old = draw(rng, 40, 4), add = draw(rng, 30, 4);
        for (auto& x : add) x += 4;
        if (check_add("lists empty before, filled by the add / old rows and no new ones", old, add, 9)) return 1;
        if (check_add("every new row in one list", draw(rng, 60, 5), std::vector<int32_t>(25, 3), 5)) return 1;
        if (check_add("n_add = 1", draw(rng, 33, 6), {2}, 6)) return 1;
        if (check_add("n_add = 1, first list", draw(rng, 33, 6), {0}, 6)) return 1;
        if (check_add("n_add = 1, last list", draw(rng, 33, 6), {5}, 6)) return 1;
        if (check_add("nlist = 1", std::vector<int32_t>(17, 0), std::vector<int32_t>(9, 0), 1)) return 1;
        // two adds in a row: the second add's old index is the first add's result
        std::vector<int32_t> a = draw(rng, 45, 8), b1 = draw(rng, 20, 8), b2 = draw(rng, 31, 8);
        if (check_add("two adds in a row (first)", a, b1, 8)) return 1;
        a.insert(a.end(), b1.begin(), b1.end());
        if (check_add("two adds in a row (second)", a, b2, 8)) return 1;
        cases += 11;
    }
    // ---- random cases
    for (int it = 0; it < 400; ++it) {
        const int nlist = 1 + (int)(rng() % 40);
        const size_t n_old = rng() % 300, n_add = rng() % 200;
        std::vector<int32_t> old = draw(rng, n_old, nlist), add = draw(rng, n_add, nlist);
        if (it % 3 == 0 && nlist > 2)  // some lists stay empty on either side
            for (auto& x : add) x = x % (nlist / 2);
        if (check_add("random", old, add, nlist)) {
            std::printf("(case %d: nlist %d n_old %zu n_add %zu)\n", it, nlist, n_old, n_add);
            return 1;
        }
        ++cases;
    }
    // ---- the row mover's deal: every row geometry's chunk count, row counts around the tile and the launch size
    for (int chunks : {1, 2, 8, 24, 25, 32, 48, 63, 64, 65, 96, 256})
        for (long long rows : {0ll, 1ll, 7ll, 64ll, 1000ll, 4501ll})
            for (int n_cu : {1, 256}) {
                if (check_deal(rows, chunks, n_cu)) return 1;
                ++cases;
            }
    std::printf("OK %lld cases\n", cases);
    return 0;
}
