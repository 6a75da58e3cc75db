// Host check of csrc/ls_ivf_remove_plan.h and csrc/ls_rows_plan.h (compiled with AddressSanitizer + UndefinedBehaviorSanitizer and run by
// tests/test_ivf_remove_cpu.py). For every case the plan of "old index - the rows a bitmap selects" is compared with a
// from-scratch counting sort of the surviving assignment - what ivf_build makes of the survivors alone:
//   n_new, assign_new, sizes, off_new == the counting sort's;
//   ids_new == the counting sort's ids (the NEW original row of every destination storage row);
//   src[s] names the old STORAGE row that held the row which is now new original row ids_new[s];
//   dst_of and src are mutual inverses on survivors, and dst_of is LS_ROWS_GONE exactly on the removed rows.
// Then the row kernel's deal (every (row, chunk) of the destination is moved by exactly one lane of one tile) and the
// subset kernels' deal: the (list, step, lane) walk with its ballots, wave totals and bases, emulated thread by thread,
// against a sequential compaction of the same segments.
#include <cstdio>
#include <random>
#include <vector>

#include "ls_ivf_remove_plan.h"

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

// the bitmap (ls_subset_create's layout) that selects the rows r with gone[r], nbytes bytes long
static std::vector<uint8_t> bitmap_of(const std::vector<char>& gone, size_t nbytes) {
    std::vector<uint8_t> bm(nbytes, 0);
    for (size_t r = 0; r < gone.size(); ++r)
        if (gone[r] && (r >> 3) < nbytes) bm[r >> 3] |= (uint8_t)(1u << (r & 7));
    return bm;
}

// the removal `bm` from the index of `assign`: 0, or 1 after printing what differs
static int check_remove(const char* name, const std::vector<int32_t>& assign, const std::vector<uint8_t>& bm, int nlist) {
    const size_t n = assign.size();
    const int64_t nbytes = (int64_t)bm.size();
    const sorted_index before = sort_from_scratch(assign, nlist);
    std::vector<char> gone(n, 0);
    std::vector<uint32_t> renum(n, LS_ROWS_GONE);  // old original row -> new original row
    std::vector<int32_t> surv;
    for (size_t r = 0; r < n; ++r) {
        gone[r] = (r >> 3) < bm.size() && ((bm[r >> 3] >> (r & 7)) & 1);
        if (!gone[r]) {
            renum[r] = (uint32_t)surv.size();
            surv.push_back(assign[r]);
        }
    }
    const sorted_index want = sort_from_scratch(surv, nlist);
    ls_ivf_remove_plan p;
    ls_ivf_remove_plan_make(assign.data(), (int64_t)n, nlist, before.off.data(), bm.empty() ? nullptr : bm.data(), nbytes, p);
    if (ls_ivf_remove_count(bm.empty() ? nullptr : bm.data(), nbytes, (int64_t)n) != (int64_t)(n - surv.size()))
        FAIL("%s: ls_ivf_remove_count", name);
    if (p.n_new != (int64_t)surv.size()) FAIL("%s: n_new = %lld, want %zu", name, (long long)p.n_new, surv.size());
    if (p.assign_new != surv) FAIL("%s: assign_new differs", name);
    if (p.off_new != want.off) FAIL("%s: off_new differs", name);
    if (p.ids_new != want.ids) FAIL("%s: ids_new differs", name);
    if (p.sizes.size() != (size_t)nlist || p.src.size() != surv.size() || p.dst_of.size() != n) FAIL("%s: table sizes", name);
    for (int l = 0; l < nlist; ++l)
        if (p.sizes[(size_t)l] != (int64_t)want.off[(size_t)l + 1] - want.off[(size_t)l]) FAIL("%s: sizes[%d]", name, l);
    for (size_t s = 0; s < surv.size(); ++s) {
        const uint32_t t = p.src[s];
        if (t >= n) FAIL("%s: src[%zu] = %u names no old storage row", name, s, t);
        const uint32_t r_old = before.ids[t];
        if (gone[r_old]) FAIL("%s: src[%zu] names a removed row", name, s);
        if (renum[r_old] != want.ids[s]) FAIL("%s: src[%zu] holds old row %u = new row %u, want %u", name, s, r_old, renum[r_old], want.ids[s]);
        if (p.dst_of[t] != s) FAIL("%s: dst_of[src[%zu]] = %u", name, s, p.dst_of[t]);
        if (s > 0 && surv[want.ids[s]] == surv[want.ids[s - 1]] && p.src[s] <= p.src[s - 1]) FAIL("%s: order inside a list", name);
    }
    for (size_t t = 0; t < n; ++t) {
        const bool g = gone[before.ids[t]] != 0;
        if (g != (p.dst_of[t] == LS_ROWS_GONE)) FAIL("%s: dst_of[%zu] = %u for a %s row", name, t, p.dst_of[t], g ? "removed" : "kept");
        if (!g && (p.dst_of[t] >= surv.size() || p.src[p.dst_of[t]] != t)) FAIL("%s: src[dst_of[%zu]]", name, t);
    }
    return 0;
}

// the row kernel's enumeration (ls_rows_plan.h's deal): W waves, wave gw takes tiles gw, gw + W, ...
static int check_row_deal(long long rows, int chunks, int n_cu) {
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

// The subset kernels, thread by thread. A subset with the given selected rows per list over an index whose list l has
// 2 * sel[l] + 3 rows (every other row selected); `keep(old storage row)` says whether the row survives. G workgroups.
template <class Keep>
static int check_subset_deal(const char* name, const std::vector<uint32_t>& sel, int G, Keep keep) {
    const int nlist = (int)sel.size();
    std::vector<uint32_t> off((size_t)nlist + 1, 0), soff((size_t)nlist + 1, 0), srow;
    for (int l = 0; l < nlist; ++l) {
        off[(size_t)l + 1] = off[(size_t)l] + 2 * sel[(size_t)l] + 3;
        soff[(size_t)l + 1] = soff[(size_t)l] + sel[(size_t)l];
        for (uint32_t j = 0; j < sel[(size_t)l]; ++j) srow.push_back(off[(size_t)l] + 1 + 2 * j);
    }
    const uint32_t n_old = off[(size_t)nlist];
    // dst_of / ids_new as the plan makes them: survivors keep their order inside a list
    std::vector<uint32_t> dst_of(n_old, LS_ROWS_GONE), ids_new;
    for (uint32_t t = 0; t < n_old; ++t)
        if (keep(t)) {
            dst_of[t] = (uint32_t)ids_new.size();
            ids_new.push_back(1000000u + t);  // (any table: the kernel copies ids_new[destination])
        }
    // sequential compaction: the reference
    std::vector<uint32_t> want_soff((size_t)nlist + 1, 0), want_srow, want_sid;
    for (int l = 0; l < nlist; ++l) {
        for (uint32_t j = soff[(size_t)l]; j < soff[(size_t)l + 1]; ++j)
            if (dst_of[srow[j]] != LS_ROWS_GONE) {
                want_srow.push_back(dst_of[srow[j]]);
                want_sid.push_back(ids_new[dst_of[srow[j]]]);
            }
        want_soff[(size_t)l + 1] = (uint32_t)want_srow.size();
    }
    // ---- the count kernel
    std::vector<uint32_t> counts((size_t)nlist, 0xdeadbeefu);
    std::vector<int> looked(srow.size(), 0);
    for (int g = 0; g < G; ++g)
        for (int l = g; l < nlist; l += G) {
            const uint32_t b = soff[(size_t)l], e = soff[(size_t)l + 1];
            uint32_t mine[LS_LIST_WAVES] = {};
            for (uint32_t i = 0; i < ls_list_steps(e - b); ++i)
                for (int w = 0; w < LS_LIST_WAVES; ++w) {
                    unsigned long long ballot = 0;
                    for (int lane = 0; lane < LS_ROWS_WAVE; ++lane) {
                        const long long j = ls_list_pos(b, i, w * LS_ROWS_WAVE + lane);
                        if (j < b) FAIL("%s: position below the segment", name);
                        if (j >= (long long)e) continue;
                        looked[(size_t)j]++;
                        if (dst_of[srow[(size_t)j]] != LS_ROWS_GONE) ballot |= 1ull << lane;
                    }
                    mine[w] += (uint32_t)__builtin_popcountll(ballot);
                }
            counts[(size_t)l] = ls_list_step_total(mine);
        }
    for (size_t j = 0; j < looked.size(); ++j)
        if (looked[j] != 1) FAIL("%s: position %zu looked at %d times", name, j, looked[j]);
    for (int l = 0; l < nlist; ++l)
        if (counts[(size_t)l] != want_soff[(size_t)l + 1] - want_soff[(size_t)l])
            FAIL("%s: counts[%d] = %u, want %u", name, l, counts[(size_t)l], want_soff[(size_t)l + 1] - want_soff[(size_t)l]);
    // ---- the host's part: new offsets from the counts; then the scatter kernel
    std::vector<uint32_t> soff_new((size_t)nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) soff_new[(size_t)l + 1] = soff_new[(size_t)l] + counts[(size_t)l];
    const size_t m_new = soff_new[(size_t)nlist];
    std::vector<uint32_t> srow_new(m_new, LS_ROWS_GONE), sid_new(m_new, LS_ROWS_GONE);
    std::vector<int> written(m_new, 0);
    for (int g = 0; g < G; ++g)
        for (int l = g; l < nlist; l += G) {
            const uint32_t b = soff[(size_t)l], e = soff[(size_t)l + 1];
            const uint32_t room = soff_new[(size_t)l + 1] - soff_new[(size_t)l];
            const long long base = soff_new[(size_t)l];
            uint32_t done = 0;
            for (uint32_t i = 0; i < ls_list_steps(e - b); ++i) {
                unsigned long long ballot[LS_LIST_WAVES] = {};
                uint32_t totals[LS_LIST_WAVES] = {};
                for (int tid = 0; tid < LS_LIST_THREADS; ++tid) {
                    const long long j = ls_list_pos(b, i, tid);
                    if (j < (long long)e && dst_of[srow[(size_t)j]] != LS_ROWS_GONE) ballot[tid / LS_ROWS_WAVE] |= 1ull << (tid % LS_ROWS_WAVE);
                }
                for (int w = 0; w < LS_LIST_WAVES; ++w) totals[w] = (uint32_t)__builtin_popcountll(ballot[w]);
                for (int tid = 0; tid < LS_LIST_THREADS; ++tid) {
                    const int w = tid / LS_ROWS_WAVE, lane = tid % LS_ROWS_WAVE;
                    if (!((ballot[w] >> lane) & 1)) continue;
                    const long long j = ls_list_pos(b, i, tid);
                    const uint32_t rank = done + ls_list_wave_base(totals, w) + ls_list_lane_rank(ballot[w], lane);
                    if (rank >= room) FAIL("%s: list %d rank %u of %u", name, l, rank, room);
                    const uint32_t to = dst_of[srow[(size_t)j]];
                    written[(size_t)(base + rank)]++;
                    srow_new[(size_t)(base + rank)] = to;
                    sid_new[(size_t)(base + rank)] = ids_new[to];
                }
                done += ls_list_step_total(totals);
            }
            if (done != room) FAIL("%s: list %d wrote %u of %u", name, l, done, room);
        }
    for (size_t x = 0; x < m_new; ++x)
        if (written[x] != 1) FAIL("%s: slot %zu written %d times", name, x, written[x]);
    if (soff_new != want_soff || srow_new != want_srow || sid_new != want_sid) FAIL("%s: differs from the sequential compaction", name);
    for (int l = 0; l < nlist; ++l)
        for (uint32_t x = soff_new[(size_t)l] + 1; x < soff_new[(size_t)l + 1]; ++x)
            if (srow_new[x] <= srow_new[x - 1]) FAIL("%s: list %d is not ascending", name, l);
    return 0;
}

static std::vector<int32_t> draw(std::mt19937& rng, size_t n, int nlist) {
    std::vector<int32_t> a(n);
    for (auto& x : a) x = (int32_t)(rng() % (unsigned)nlist);
    return a;
}

int main() {
    std::mt19937 rng(20240702);
    long long cases = 0;
    // ---- the named edge cases
    {
        if (check_remove("n = 0", {}, {0xff, 0xff}, 3)) return 1;
        const std::vector<int32_t> a = draw(rng, 61, 6);
        const size_t n = a.size(), full = (n + 7) / 8;
        if (check_remove("nothing removed", a, std::vector<uint8_t>(full, 0), 6)) return 1;
        if (check_remove("everything removed", a, std::vector<uint8_t>(full, 0xff), 6)) return 1;
        std::vector<char> gone(n, 0);
        for (size_t r = 0; r < n; ++r) gone[r] = a[r] == 2;
        if (check_remove("a whole list removed", a, bitmap_of(gone, full), 6)) return 1;
        size_t first = n, last = n;  // the first and the last row of list 3
        for (size_t r = 0; r < n; ++r)
            if (a[r] == 3) {
                if (first == n) first = r;
                last = r;
            }
        if (first == n || first == last) FAIL("the drawn assignment has fewer than two rows in list 3");
        gone.assign(n, 0);
        gone[first] = 1;
        if (check_remove("first row of a list", a, bitmap_of(gone, full), 6)) return 1;
        gone.assign(n, 0);
        gone[last] = 1;
        if (check_remove("last row of a list", a, bitmap_of(gone, full), 6)) return 1;
        gone.assign(n, 0);
        gone[0] = 1;
        if (check_remove("first row overall", a, bitmap_of(gone, full), 6)) return 1;
        gone.assign(n, 0);
        gone[n - 1] = 1;
        if (check_remove("last row overall", a, bitmap_of(gone, full), 6)) return 1;
        for (size_t r = 0; r < n; ++r) gone[r] = (char)(rng() & 1);
        if (check_remove("a short bitmap (rows past it are kept)", a, bitmap_of(gone, 3), 6)) return 1;
        std::vector<uint8_t> bm = bitmap_of(gone, full);
        bm.back() |= 0xe0;  // (n = 61: bits 61..63 of the last byte)
        bm.push_back(0xff);
        bm.push_back(0xff);
        if (check_remove("bits past n", a, bm, 6)) return 1;
        cases += 10;
    }
    // ---- random cases
    for (int it = 0; it < 400; ++it) {
        const int nlist = 1 + (int)(rng() % 40);
        const size_t n = rng() % 400;
        std::vector<int32_t> a = draw(rng, n, nlist);
        if (it % 3 == 0 && nlist > 2)  // some lists are empty before the removal
            for (auto& x : a) x = x % (nlist / 2);
        const unsigned pct = rng() % 101;
        std::vector<char> gone(n, 0);
        for (auto& g : gone) g = (char)(rng() % 100 < pct);
        const size_t nbytes = it % 5 == 0 ? rng() % ((n + 7) / 8 + 3) : (n + 7) / 8;
        if (check_remove("random", a, bitmap_of(gone, nbytes), nlist)) {
            std::printf("(case %d: nlist %d n %zu nbytes %zu)\n", it, nlist, n, nbytes);
            return 1;
        }
        ++cases;
    }
    // ---- the row kernel's deal: every row geometry's chunk count, row counts around the tile and the launch size
    for (int chunks : {1, 2, 8, 24, 25, 32, 48, 63, 64, 65, 96, 256})
        for (long long rows : {0ll, 1ll, 7ll, 64ll, 1000ll, 4501ll})
            for (int n_cu : {1, 256}) {
                if (check_row_deal(rows, chunks, n_cu)) return 1;
                ++cases;
            }
    // ---- the subset kernels' deal: lists of 0, 1, 63, 64, 65, 255, 256, 257 and 1000 selected rows
    {
        const std::vector<uint32_t> sel = {0, 1, 63, 64, 65, 255, 256, 257, 1000, 0, 513};
        std::vector<char> coin(5000);
        for (auto& c : coin) c = (char)(rng() % 100);
        for (int G : {1, 3, ls_list_groups((int)sel.size())}) {
            if (check_subset_deal("every row kept", sel, G, [](uint32_t) { return true; })) return 1;
            if (check_subset_deal("no row kept", sel, G, [](uint32_t) { return false; })) return 1;
            if (check_subset_deal("half kept", sel, G, [&](uint32_t t) { return coin[t] < 50; })) return 1;
            if (check_subset_deal("a tenth removed", sel, G, [&](uint32_t t) { return coin[t] >= 10; })) return 1;
            if (check_subset_deal("every fourth row kept", sel, G, [](uint32_t t) { return t % 4 == 1; })) return 1;
            cases += 5;
        }
    }
    std::printf("OK %lld cases\n", cases);
    return 0;
}
