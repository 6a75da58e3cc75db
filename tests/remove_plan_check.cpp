// Host check of csrc/ls_remove_plan.h and csrc/ls_rows_plan.h (compiled with AddressSanitizer + UndefinedBehaviorSanitizer and run by
// tests/test_remove_cpu.py). Every case is (n rows, a bitmap, slab rows, a shard split); the plan is held to a
// sequential model:
//   - the in-place slab schedule, executed on a host array in the plan's order (gather into a staging array, write
//     back), yields the survivors in their order - np.delete's result - and NEVER reads a row after a write to it: the
//     model marks written rows and fails on such a read;
//   - r0, the slice at the shard's bit offset (plain and complemented) and the counts equal a bit-by-bit reading;
//   - the gather deal visits every (row, chunk) of a slab exactly once;
//   - the subset kernels' (segment, step, lane) walk with its ballots, wave totals and bases, emulated thread by
//     thread, equals a sequential compaction of the list;
//   - the shards' slices and the new lo[] equal a from-scratch split of the survivors.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ls_remove_plan.h"

#define FAIL(...)                 \
    do {                          \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
        return 1;                 \
    } while (0)

// the bitmap (ls_subset_create's layout) that selects the rows r with gone[r], nbytes bytes long
static std::vector<uint8_t> bitmap_of(const std::vector<char>& gone, size_t nbytes) {
    std::vector<uint8_t> bm(nbytes, 0);
    for (size_t r = 0; r < gone.size(); ++r)
        if (gone[r] && (r >> 3) < nbytes) bm[r >> 3] |= (uint8_t)(1u << (r & 7));
    return bm;
}

// One single-device handle: rows [bit0, bit0 + n) of the bitmap, slab rows `want` (0: automatic for `row_bytes`).
static int check_handle(const char* name, const uint8_t* bm, int64_t nbytes, int64_t bit0, int64_t n, int64_t want,
                        int64_t row_bytes, int64_t* n_new_out) {
    std::vector<char> gone((size_t)n, 0);
    std::vector<uint32_t> src;  // what the device compaction of the complemented slice yields
    int64_t first = n;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t b = bit0 + r;
        gone[(size_t)r] = (b >> 3) < nbytes && ((bm[b >> 3] >> (b & 7)) & 1);
        if (gone[(size_t)r] && first == n) first = r;
        if (!gone[(size_t)r]) src.push_back((uint32_t)r);
    }
    const int64_t n_new = (int64_t)src.size();
    *n_new_out = n_new;
    // r0, counts, the slice
    const int64_t r0 = ls_remove_first(bm, nbytes, bit0, n);
    if (r0 != first) FAIL("%s: r0 = %lld, want %lld", name, (long long)r0, (long long)first);
    if (ls_remove_count(bm, nbytes, bit0, n) != n - n_new) FAIL("%s: ls_remove_count", name);
    for (int comp = 0; comp < 2; ++comp) {
        std::vector<uint8_t> slice;
        ls_remove_slice(bm, nbytes, bit0, n, comp != 0, slice);
        if ((int64_t)slice.size() != ls_remove_slice_bytes(bit0, n)) FAIL("%s: slice size", name);
        const int64_t off = bit0 & 7;
        for (int64_t r = 0; r < n; ++r) {
            const bool bit = (slice[(size_t)((off + r) >> 3)] >> ((off + r) & 7)) & 1;
            if (bit != (comp ? !gone[(size_t)r] : (bool)gone[(size_t)r])) FAIL("%s: slice bit %lld (complement %d)", name, (long long)r, comp);
        }
    }
    for (int64_t s = 0; s < n_new; ++s)
        if ((int64_t)src[(size_t)s] < s || (s < r0 && (int64_t)src[(size_t)s] != s)) FAIL("%s: src[%lld] < its place", name, (long long)s);
    // the slab schedule on a host array: row r holds the value r + 1; written rows are marked
    const int64_t moved = ls_remove_moved(r0, n_new);
    if (moved != (n_new > r0 ? n_new - r0 : 0)) FAIL("%s: moved", name);
    const int64_t R = ls_remove_slab_rows(want, row_bytes, moved);
    if (moved == 0 ? R != 0 : (R < 1 || R > moved)) FAIL("%s: slab rows %lld for %lld moved", name, (long long)R, (long long)moved);
    if (moved > 0 && want > 0 && R != (want < moved ? want : moved)) FAIL("%s: forced slab rows", name);
    if (moved > 0 && want == 0) {
        int64_t fit = LS_RM_STAGE_BYTES / row_bytes;
        if (fit < 1) fit = 1;
        if (R != (fit < moved ? fit : moved)) FAIL("%s: automatic slab rows", name);
    }
    const int64_t slabs = ls_remove_slabs(r0, n_new, R);
    if (moved == 0 ? slabs != 0 : slabs != (moved + R - 1) / R) FAIL("%s: slabs", name);
    std::vector<int64_t> rows((size_t)n), stage((size_t)(R > 0 ? R : 1), -1);
    std::vector<char> written((size_t)n, 0);
    for (int64_t r = 0; r < n; ++r) rows[(size_t)r] = r + 1;
    int64_t next = r0;
    for (int64_t j = 0; j < slabs; ++j) {
        const int64_t a = ls_remove_slab_begin(r0, R, j), c = ls_remove_slab_count(r0, n_new, R, j);
        if (a != next || c < 1 || c > R || a + c > n_new) FAIL("%s: slab %lld = [%lld, +%lld)", name, (long long)j, (long long)a, (long long)c);
        next = a + c;
        // the gather, dealt as the kernel deals it, for a few row widths: every (row, chunk) exactly once
        for (int chunks : {1, 5, 24, 64, 100}) {
            std::vector<int> hit((size_t)c * chunks, 0);
            const int TR = ls_rows_tile_rows(chunks);
            const long long NT = ls_rows_tiles(c, chunks);
            for (long long t = 0; t < NT; ++t)
                for (int lane = 0; lane < LS_ROWS_WAVE; ++lane) {
                    const int lr = ls_rows_lane_row(lane, chunks);
                    if (lr >= TR) continue;
                    const long long i = t * TR + lr;
                    if (i >= c) continue;
                    for (int ch = ls_rows_lane_chunk(lane, chunks); ch < chunks; ch += LS_ROWS_WAVE) hit[(size_t)(i * chunks + ch)]++;
                }
            for (int h : hit)
                if (h != 1) FAIL("%s: gather deal (%d chunks) misses or repeats a chunk", name, chunks);
            if (ls_rows_blocks(c, chunks, 256) < 1) FAIL("%s: gather blocks", name);
        }
        for (int64_t i = 0; i < c; ++i) {
            const int64_t from = src[(size_t)(a + i)];
            if (from < a) FAIL("%s: slab %lld reads row %lld below its first row", name, (long long)j, (long long)from);
            if (written[(size_t)from]) FAIL("%s: slab %lld reads row %lld after a write to it", name, (long long)j, (long long)from);
            stage[(size_t)i] = rows[(size_t)from];
        }
        for (int64_t i = 0; i < c; ++i) {
            rows[(size_t)(a + i)] = stage[(size_t)i];
            written[(size_t)(a + i)] = 1;
        }
    }
    if (moved > 0 && next != n_new) FAIL("%s: the slabs end at %lld, not %lld", name, (long long)next, (long long)n_new);
    for (int64_t s = 0; s < n_new; ++s)
        if (rows[(size_t)s] != (int64_t)src[(size_t)s] + 1) FAIL("%s: new row %lld holds old row %lld", name, (long long)s, (long long)rows[(size_t)s] - 1);
    return 0;
}

// The subset kernels' walk over `list` (ascending rows) with dst_of, emulated thread by thread.
static int check_subset(const char* name, const std::vector<uint32_t>& list, const std::vector<uint32_t>& dst_of) {
    std::vector<uint32_t> want;
    for (uint32_t r : list)
        if (dst_of[r] != LS_ROWS_GONE) want.push_back(dst_of[r]);
    const long long m = (long long)list.size(), groups = ls_remove_segs(m);
    if (groups < 1 || groups * LS_RM_SEG < m || (m > 0 && (groups - 1) * LS_RM_SEG >= m)) FAIL("%s: groups", name);
    if (ls_list_groups(groups) < 1 || ls_list_groups(groups) > groups) FAIL("%s: workgroups", name);
    // segment g: [g * LS_RM_SEG, min(m, (g + 1) * LS_RM_SEG)), walked through the shared steps / pos
    auto begin = [&](long long g) { return (uint32_t)(g * LS_RM_SEG); };
    auto end = [&](long long g) { return (uint32_t)(m < (g + 1) * LS_RM_SEG ? m : (g + 1) * LS_RM_SEG); };
    auto to = [&](long long j, uint32_t e) { return j < (long long)e ? dst_of[list[(size_t)j]] : LS_ROWS_GONE; };
    std::vector<uint32_t> counts((size_t)groups, 0), offs((size_t)groups + 1, 0);
    std::vector<char> seen((size_t)(m > 0 ? m : 1), 0);
    for (long long g = 0; g < groups; ++g)
        for (uint32_t i = 0; i < ls_list_steps(end(g) - begin(g)); ++i)
            for (int tid = 0; tid < LS_LIST_THREADS; ++tid) {
                const long long j = ls_list_pos(begin(g), i, tid);
                if (j < (long long)end(g)) {
                    if (seen[(size_t)j]++) FAIL("%s: position %lld dealt twice", name, j);
                    counts[(size_t)g] += to(j, end(g)) != LS_ROWS_GONE;
                }
            }
    for (long long j = 0; j < m; ++j)
        if (!seen[(size_t)j]) FAIL("%s: position %lld never dealt", name, j);
    for (long long g = 0; g < groups; ++g) offs[(size_t)g + 1] = offs[(size_t)g] + counts[(size_t)g];  // (the scan: total in [groups])
    std::vector<uint32_t> got(want.size(), LS_ROWS_GONE);
    for (long long g = 0; g < groups; ++g) {
        const uint32_t b = begin(g), e = end(g), room = offs[(size_t)g + 1] - offs[(size_t)g];
        uint32_t done = 0;
        for (uint32_t i = 0; i < ls_list_steps(e - b); ++i) {
            unsigned long long ballot[LS_LIST_WAVES];
            uint32_t totals[LS_LIST_WAVES];
            for (int w = 0; w < LS_LIST_WAVES; ++w) {
                ballot[w] = 0;
                for (int lane = 0; lane < LS_ROWS_WAVE; ++lane)
                    if (to(ls_list_pos(b, i, w * LS_ROWS_WAVE + lane), e) != LS_ROWS_GONE) ballot[w] |= 1ull << lane;
                totals[w] = (uint32_t)__builtin_popcountll(ballot[w]);
            }
            for (int tid = 0; tid < LS_LIST_THREADS; ++tid) {
                const int w = tid / LS_ROWS_WAVE, lane = tid % LS_ROWS_WAVE;
                const uint32_t t = to(ls_list_pos(b, i, tid), e);
                if (t == LS_ROWS_GONE) continue;
                const uint32_t rank = done + ls_list_wave_base(totals, w) + ls_list_lane_rank(ballot[w], lane);
                if (rank >= room) FAIL("%s: segment %lld rank %u of %u", name, g, rank, room);
                const long long at = (long long)offs[(size_t)g] + rank;
                if (at < 0 || at >= (long long)got.size()) FAIL("%s: scatter past the new list", name);
                if (got[(size_t)at] != LS_ROWS_GONE) FAIL("%s: scatter writes a slot twice", name);
                got[(size_t)at] = t;
            }
            done += ls_list_step_total(totals);
        }
    }
    if (got != want) FAIL("%s: the subset walk differs from a sequential compaction", name);
    return 0;
}

// One case: the whole index on one handle, then split into shards at `cuts` (ascending first rows, cuts[0] == 0).
static int check_case(const char* name, int64_t n, const std::vector<uint8_t>& bm, int64_t want, int64_t row_bytes,
                      const std::vector<int64_t>& cuts, std::mt19937& rng) {
    const uint8_t* p = bm.empty() ? nullptr : bm.data();
    const int64_t nbytes = (int64_t)bm.size();
    int64_t n_new = 0;
    if (check_handle(name, p, nbytes, 0, n, want, row_bytes, &n_new)) return 1;
    // shards: each takes its own bits; afterwards the blocks are contiguous and their rows are the survivors' split
    const int G = (int)cuts.size();
    std::vector<int64_t> rows((size_t)G), lo((size_t)G), lo_want((size_t)G);
    int64_t at = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t b = cuts[(size_t)g], e = g + 1 < G ? cuts[(size_t)g + 1] : n;
        if (check_handle(name, p, nbytes, b, e - b, want, row_bytes, &rows[(size_t)g])) return 1;
        int64_t kept = 0;
        for (int64_t r = b; r < e; ++r) kept += !ls_rows_bit(p, nbytes, r);
        if (kept != rows[(size_t)g]) FAIL("%s: shard %d keeps %lld rows, want %lld", name, g, (long long)rows[(size_t)g], (long long)kept);
        lo_want[(size_t)g] = at;
        at += kept;
    }
    if (ls_remove_new_lo(rows.data(), G, lo.data()) != n_new || lo != lo_want) FAIL("%s: new lo[]", name);
    // an existing subset: a random selection of the old rows
    std::vector<uint32_t> dst_of((size_t)n, LS_ROWS_GONE), list;
    uint32_t s = 0;
    for (int64_t r = 0; r < n; ++r)
        if (!ls_rows_bit(p, nbytes, r)) dst_of[(size_t)r] = s++;
    const unsigned keep = rng() % 5;  // 0: empty subset, 4: every row
    for (int64_t r = 0; r < n; ++r)
        if (keep == 4 || (keep > 0 && rng() % 4 < keep)) list.push_back((uint32_t)r);
    return check_subset(name, list, dst_of);
}

int main() {
    std::mt19937 rng(20260);
    int cases = 0;
    auto mask = [](int64_t n, auto pred) {
        std::vector<char> g((size_t)n, 0);
        for (int64_t r = 0; r < n; ++r) g[(size_t)r] = pred(r) ? 1 : 0;
        return g;
    };
    struct named {
        const char* name;
        int64_t n;
        std::vector<uint8_t> bm;
        int64_t want;
        std::vector<int64_t> cuts;
    };
    const int64_t N = 1000;
    std::vector<named> edge = {
        {"empty index", 0, {}, 0, {0}},
        {"no bitmap", N, {}, 0, {0, 333}},
        {"nothing selected", N, bitmap_of(mask(N, [](int64_t) { return false; }), 125), 7, {0, 500}},
        {"everything selected", N, bitmap_of(mask(N, [](int64_t) { return true; }), 125), 7, {0, 3, 997}},
        {"only the tail", N, bitmap_of(mask(N, [](int64_t r) { return r >= 900; }), 125), 0, {0, 901}},
        {"only the head, slab below the shift", N, bitmap_of(mask(N, [](int64_t r) { return r < 100; }), 125), 30, {0, 50, 100}},
        {"only the head, slab above the shift", N, bitmap_of(mask(N, [](int64_t r) { return r < 100; }), 125), 400, {0, 101}},
        {"one row left", N, bitmap_of(mask(N, [](int64_t r) { return r != 617; }), 125), 1, {0, 617, 618}},
        {"first row only", N, bitmap_of(mask(N, [](int64_t r) { return r == 0; }), 125), 64, {0, 1}},
        {"last row only", N, bitmap_of(mask(N, [](int64_t r) { return r == 999; }), 125), 64, {0, 999}},
        {"every other row", N, bitmap_of(mask(N, [](int64_t r) { return (r & 1) == 0; }), 125), 1, {0, 7, 15, 16}},
        {"short bitmap", N, bitmap_of(mask(N, [](int64_t r) { return r % 3 == 0; }), 40), 17, {0, 319, 321}},
        {"long bitmap", N, bitmap_of(mask(N + 64, [](int64_t r) { return r % 5 == 0 || r >= 1000; }), 133), 0, {0, 512}},
        {"an emptied middle shard", N, bitmap_of(mask(N, [](int64_t r) { return r >= 301 && r < 707; }), 125), 100, {0, 301, 707}},
    };
    for (const named& c : edge) {
        if (check_case(c.name, c.n, c.bm, c.want, 1536, c.cuts, rng)) return 1;
        ++cases;
    }
    // shard slices at every bit offset 0..7
    for (int off = 0; off < 8; ++off) {
        const std::vector<uint8_t> bm = bitmap_of(mask(N, [](int64_t r) { return r % 7 < 3; }), 125);
        char name[64];
        std::snprintf(name, sizeof name, "bit offset %d", off);
        if (check_case(name, N, bm, 13, 400, {0, 64 + off, 512 + off}, rng)) return 1;
        ++cases;
    }
    // random (n, bitmap, slab rows, shard split) pairs; n spans several subset-kernel workgroups now and then
    for (int it = 0; it < 400; ++it) {
        const int64_t n = it % 40 == 0 ? (int64_t)(LS_RM_SEG * 2 + rng() % 5000) : (int64_t)(rng() % 3000);
        const unsigned density = rng() % 6;  // 0: none ... 5: all
        std::vector<char> gone = mask(n, [&](int64_t) { return density == 5 || rng() % 5 < density; });
        if (n > 0 && rng() % 3 == 0) {  // a block removed, a block kept
            const int64_t a = (int64_t)(rng() % n), b = a + (int64_t)(rng() % (n - a + 1));
            for (int64_t r = a; r < b; ++r) gone[(size_t)r] = rng() % 2 ? gone[(size_t)r] : (char)(it & 1);
        }
        const size_t full = (size_t)(n + 7) / 8;
        const size_t nbytes = rng() % 4 == 0 ? (size_t)(rng() % (full + 1)) : (rng() % 4 == 1 ? full + rng() % 9 : full);
        std::vector<uint8_t> bm = bitmap_of(gone, nbytes);
        if (nbytes > full)
            for (size_t i = full; i < nbytes; ++i) bm[i] = (uint8_t)rng();  // bits at r >= n are ignored
        if (n % 8 && nbytes >= full && full > 0) bm[full - 1] |= (uint8_t)(0xffu << (n % 8));
        const int64_t want = rng() % 3 == 0 ? 0 : (int64_t)(1 + rng() % (n + 5));
        const int64_t row_bytes = rng() % 2 ? 16 * (int64_t)(1 + rng() % 256) : (LS_RM_STAGE_BYTES / (int64_t)(1 + rng() % 50));
        std::vector<int64_t> cuts = {0};
        const int G = 1 + (int)(rng() % 4);
        for (int g = 1; g < G; ++g) cuts.push_back(cuts.back() + (n > cuts.back() ? (int64_t)(rng() % (n - cuts.back() + 1)) : 0));
        char name[64];
        std::snprintf(name, sizeof name, "random %d", it);
        if (check_case(name, n, bm, want, row_bytes, cuts, rng)) return 1;
        ++cases;
    }
    std::printf("OK %d cases\n", cases);
    return 0;
}
