// Host check of csrc/ls_ivf_add_plan.h and csrc/ls_ivf_remove_plan.h CHAINED (compiled with AddressSanitizer +
// UndefinedBehaviorSanitizer and run by tests/test_mutation_scripts_cpu.py). tests/ivf_add_plan_check.cpp and
// tests/ivf_remove_plan_check.cpp hold one plan each to a counting sort; here 200 random histories of 12 steps interleave
// the two, every step working on the tables the previous one left - what an ls_ivf handle does between its build and
// its destruction. Carried from step to step:
//   off, assign        the handle's host tables
//   tok[s]             a unique token per row ever added, permuted through each plan's src (what the row kernels do to
//                      the stored rows)
//   ids[s]             storage row -> original row: ls_ivf_add_id on an add, the plan's ids_new on a removal (d_ids)
//   two subsets        created at different steps by ls_ivf_subset_compact, as (soff, srow, sid); updated as the
//                      kernels update them: srow += shift[l] on an add (ls_ivf_subset_shift_kernel), and on a removal the
//                      count / scatter walk through dst_of with ls_list_pos / lane_rank / wave_base
// The model beside them is a list of (token, list) in original-row order - add appends, a removal erases - and a set
// of tokens per subset. After EVERY step: off / assign / ids / tok equal a from-scratch counting sort of the model, and
// every subset's srow names, list after list and ascending inside a list, exactly the storage rows that hold its live
// tokens, with sid == ids[srow].
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "ls_ivf_add_plan.h"
#include "ls_ivf_remove_plan.h"
#include "ls_ivf_subset_plan.h"

#define FAIL(...)                 \
    do {                          \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
        return 1;                 \
    } while (0)

struct subset {
    bool live = false;
    std::vector<uint32_t> soff, srow, sid;
    std::set<uint64_t> members;  // the model: the tokens selected at creation
};

struct history {
    int nlist = 0;
    // the handle
    std::vector<uint32_t> off, ids;
    std::vector<int32_t> assign;
    std::vector<uint64_t> tok;
    subset subs[2];
    // the model
    std::vector<uint64_t> m_tok;
    std::vector<int32_t> m_list;
    uint64_t issued = 0;
};

static std::vector<uint8_t> bitmap_of(const std::vector<char>& sel) {
    std::vector<uint8_t> bm((sel.size() + 7) / 8, 0);
    for (size_t r = 0; r < sel.size(); ++r)
        if (sel[r]) bm[r >> 3] |= (uint8_t)(1u << (r & 7));
    return bm;
}

static void add_step(history& h, const std::vector<int32_t>& lists) {
    const uint32_t n_old = h.off[(size_t)h.nlist];
    ls_ivf_add_plan p;
    ls_ivf_add_plan_make(h.off.data(), h.nlist, lists.data(), (int64_t)lists.size(), p);
    std::vector<uint64_t> tok(p.src.size());
    std::vector<uint32_t> ids(p.src.size());
    for (size_t s = 0; s < p.src.size(); ++s) {
        tok[s] = p.src[s] < n_old ? h.tok[p.src[s]] : h.issued + (p.src[s] - n_old);
        ids[s] = ls_ivf_add_id(p.src[s], n_old, h.ids.data());
    }
    for (subset& u : h.subs)
        if (u.live)
            for (int l = 0; l < h.nlist; ++l)
                for (uint32_t j = u.soff[(size_t)l]; j < u.soff[(size_t)l + 1]; ++j) u.srow[j] += p.shift[(size_t)l];
    h.tok.swap(tok);
    h.ids.swap(ids);
    h.off.swap(p.off_new);
    h.assign.insert(h.assign.end(), lists.begin(), lists.end());
    for (size_t j = 0; j < lists.size(); ++j) {
        h.m_tok.push_back(h.issued + j);
        h.m_list.push_back(lists[j]);
    }
    h.issued += lists.size();
}

// the count and scatter kernels of ls_rows.hip over one IVF subset, thread by thread; 0, or 1 after printing
static int compact_subset(subset& u, int nlist, const ls_ivf_remove_plan& p) {
    const int G = ls_list_groups(nlist);
    std::vector<uint32_t> counts((size_t)nlist, 0);
    for (int g = 0; g < G; ++g)
        for (int l = g; l < nlist; l += G) {
            const uint32_t b = u.soff[(size_t)l], e = u.soff[(size_t)l + 1];
            uint32_t mine[LS_LIST_WAVES] = {};
            for (uint32_t i = 0; i < ls_list_steps(e - b); ++i)
                for (int tid = 0; tid < LS_LIST_THREADS; ++tid) {
                    const long long j = ls_list_pos(b, i, tid);
                    if (j < (long long)e && p.dst_of[u.srow[(size_t)j]] != LS_ROWS_GONE) mine[tid / LS_ROWS_WAVE]++;
                }
            counts[(size_t)l] = ls_list_step_total(mine);
        }
    std::vector<uint32_t> soff((size_t)nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) soff[(size_t)l + 1] = soff[(size_t)l] + counts[(size_t)l];
    std::vector<uint32_t> srow(soff[(size_t)nlist], LS_ROWS_GONE), sid(soff[(size_t)nlist], LS_ROWS_GONE);
    for (int g = 0; g < G; ++g)
        for (int l = g; l < nlist; l += G) {
            const uint32_t b = u.soff[(size_t)l], e = u.soff[(size_t)l + 1];
            const uint32_t room = counts[(size_t)l], base = soff[(size_t)l];
            uint32_t done = 0;
            for (uint32_t i = 0; i < ls_list_steps(e - b); ++i) {
                unsigned long long ballot[LS_LIST_WAVES] = {};
                uint32_t totals[LS_LIST_WAVES] = {};
                for (int tid = 0; tid < LS_LIST_THREADS; ++tid) {
                    const long long j = ls_list_pos(b, i, tid);
                    if (j < (long long)e && p.dst_of[u.srow[(size_t)j]] != LS_ROWS_GONE)
                        ballot[tid / LS_ROWS_WAVE] |= 1ull << (tid % LS_ROWS_WAVE);
                }
                for (int w = 0; w < LS_LIST_WAVES; ++w) totals[w] = (uint32_t)__builtin_popcountll(ballot[w]);
                for (int tid = 0; tid < LS_LIST_THREADS; ++tid) {
                    const int w = tid / LS_ROWS_WAVE, lane = tid % LS_ROWS_WAVE;
                    if (!((ballot[w] >> lane) & 1)) continue;
                    const uint32_t rank = done + ls_list_wave_base(totals, w) + ls_list_lane_rank(ballot[w], lane);
                    if (rank >= room) FAIL("list %d: rank %u of %u", l, rank, room);
                    const uint32_t to = p.dst_of[u.srow[(size_t)ls_list_pos(b, i, tid)]];
                    srow[base + rank] = to;
                    sid[base + rank] = p.ids_new[to];
                }
                done += ls_list_step_total(totals);
            }
            if (done != room) FAIL("list %d: wrote %u of %u", l, done, room);
        }
    u.soff.swap(soff);
    u.srow.swap(srow);
    u.sid.swap(sid);
    return 0;
}

static int remove_step(history& h, const std::vector<char>& sel) {
    const std::vector<uint8_t> bm = bitmap_of(sel);
    const int64_t n = (int64_t)h.assign.size();
    ls_ivf_remove_plan p;
    ls_ivf_remove_plan_make(h.assign.data(), n, h.nlist, h.off.data(), bm.empty() ? nullptr : bm.data(), (int64_t)bm.size(), p);
    std::vector<uint64_t> tok((size_t)p.n_new);
    for (size_t s = 0; s < tok.size(); ++s) tok[s] = h.tok[p.src[s]];
    for (subset& u : h.subs)
        if (u.live && compact_subset(u, h.nlist, p)) return 1;
    h.tok.swap(tok);
    h.ids = p.ids_new;
    h.off.swap(p.off_new);
    h.assign.swap(p.assign_new);
    std::vector<uint64_t> m_tok;
    std::vector<int32_t> m_list;
    for (size_t r = 0; r < h.m_tok.size(); ++r)
        if (!sel[r]) {
            m_tok.push_back(h.m_tok[r]);
            m_list.push_back(h.m_list[r]);
        }
    h.m_tok.swap(m_tok);
    h.m_list.swap(m_list);
    return 0;
}

static void subset_new(history& h, subset& u, const std::vector<char>& sel) {
    const std::vector<uint8_t> bm = bitmap_of(sel);
    ls_ivf_subset_plan p;
    ls_ivf_subset_compact(h.assign.data(), (int64_t)h.assign.size(), h.nlist, h.off.data(), bm.empty() ? nullptr : bm.data(),
                          (int64_t)bm.size(), p);
    u.live = true;
    u.soff.swap(p.soff);
    u.srow.swap(p.srow);
    u.sid.swap(p.sid);
    u.members.clear();
    for (size_t r = 0; r < sel.size(); ++r)
        if (sel[r]) u.members.insert(h.m_tok[r]);
}

// the handle's tables against the model, from scratch
static int check(const history& h) {
    const size_t n = h.m_tok.size();
    if (h.assign != h.m_list) FAIL("assign differs from the model's lists");
    std::vector<uint32_t> off((size_t)h.nlist + 1, 0);
    for (int32_t a : h.m_list) off[(size_t)a + 1]++;
    for (int l = 0; l < h.nlist; ++l) off[(size_t)l + 1] += off[(size_t)l];
    if (h.off != off) FAIL("off differs from the counting sort");
    std::vector<uint32_t> at(off.begin(), off.end() - 1), ids(n);
    std::vector<uint64_t> tok(n);
    for (size_t r = 0; r < n; ++r) {
        const uint32_t s = at[(size_t)h.m_list[r]]++;
        ids[s] = (uint32_t)r;
        tok[s] = h.m_tok[r];
    }
    if (h.ids != ids) FAIL("ids differs from the counting sort");
    if (h.tok != tok) FAIL("the stored rows (tokens) differ from the counting sort");
    for (int x = 0; x < 2; ++x) {
        const subset& u = h.subs[x];
        if (!u.live) continue;
        if (u.soff.size() != (size_t)h.nlist + 1 || u.soff[0] != 0) FAIL("subset %d: soff", x);
        std::vector<uint32_t> srow;
        for (int l = 0; l < h.nlist; ++l) {
            for (uint32_t s = off[(size_t)l]; s < off[(size_t)l + 1]; ++s)
                if (u.members.count(tok[s])) srow.push_back(s);
            if (u.soff[(size_t)l + 1] != srow.size()) FAIL("subset %d: soff[%d] = %u, want %zu", x, l + 1, u.soff[(size_t)l + 1], srow.size());
        }
        if (u.srow != srow) FAIL("subset %d: srow does not name the storage rows of its live tokens", x);
        if (u.sid.size() != srow.size()) FAIL("subset %d: sid size", x);
        for (size_t j = 0; j < srow.size(); ++j)
            if (u.sid[j] != h.ids[srow[j]]) FAIL("subset %d: sid[%zu] = %u, ids[srow] = %u", x, j, u.sid[j], h.ids[srow[j]]);
    }
    return 0;
}

int main() {
    std::mt19937 rng(20250311);
    const int HISTORIES = 200, STEPS = 12;
    long long steps = 0, refills = 0, zeros = 0, recoveries = 0, shrunk_subsets = 0;
    for (int it = 0; it < HISTORIES; ++it) {
        history h;
        h.nlist = 1 + (int)(rng() % 20);
        h.off.assign((size_t)h.nlist + 1, 0);
        const int lists_used = it % 3 == 0 && h.nlist > 2 ? h.nlist / 2 : h.nlist;  // (some lists never hold a row)
        const int new_at[2] = {(int)(rng() % 4), 5 + (int)(rng() % 4)};                // the subsets' creation steps
        std::vector<char> was_empty((size_t)h.nlist, 0), had_rows((size_t)h.nlist, 0);
        bool was_zero = false;
        for (int st = 0; st < STEPS; ++st) {
            const size_t n = h.assign.size();
            const unsigned what = n == 0 ? 0u : rng() % 10;
            if (st == 0 || what < 4) {  // an add: 0, 1, 63 or up to 300 rows, now and then all into one list
                const unsigned pick = rng() % 8;
                const size_t m = st == 0 ? 100 + rng() % 300 : (pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? 63 : rng() % 300);
                std::vector<int32_t> lists(m);
                const int one = rng() % 4 == 0 ? (int)(rng() % (unsigned)lists_used) : -1;
                for (auto& a : lists) a = one >= 0 ? one : (int32_t)(rng() % (unsigned)lists_used);
                add_step(h, lists);
            } else {  // a removal: a share, one whole list, everything, nothing
                std::vector<char> sel(n, 0);
                const unsigned kind = rng() % 8;
                const unsigned pct = rng() % 101;
                const int32_t list = (int32_t)(rng() % (unsigned)lists_used);
                for (size_t r = 0; r < n; ++r)
                    sel[r] = kind == 0 ? h.assign[r] == list : kind == 1 ? 1 : kind == 2 ? 0 : (char)(rng() % 100 < pct);
                size_t before[2] = {h.subs[0].srow.size(), h.subs[1].srow.size()};
                if (remove_step(h, sel)) {
                    std::printf("(history %d step %d: removal)\n", it, st);
                    return 1;
                }
                for (int x = 0; x < 2; ++x) shrunk_subsets += h.subs[x].live && h.subs[x].srow.size() < before[x];
            }
            for (int x = 0; x < 2; ++x)
                if (st == new_at[x]) {
                    std::vector<char> sel(h.assign.size());
                    for (auto& c : sel) c = (char)(rng() & 1);
                    subset_new(h, h.subs[x], sel);
                }
            if (check(h)) {
                std::printf("(history %d step %d, nlist %d, n %zu)\n", it, st, h.nlist, h.assign.size());
                return 1;
            }
            for (int l = 0; l < h.nlist; ++l) {
                const bool rows = h.off[(size_t)l + 1] > h.off[(size_t)l];
                if (rows && was_empty[(size_t)l]) ++refills, was_empty[(size_t)l] = 0;
                if (!rows && had_rows[(size_t)l]) was_empty[(size_t)l] = 1;
                had_rows[(size_t)l] = (char)rows;
            }
            if (h.assign.empty() && !was_zero) ++zeros, was_zero = true;
            if (!h.assign.empty() && was_zero) ++recoveries, was_zero = false;
            ++steps;
        }
    }
    // the histories are random: say what they reached, so that a change which hollows them out fails here
    if (refills < 50 || zeros < 10 || recoveries < 10 || shrunk_subsets < 200)
        FAIL("the histories reach too little: %lld refills, %lld zeros, %lld recoveries, %lld subset compactions", refills, zeros,
             recoveries, shrunk_subsets);
    std::printf("OK %d histories %lld steps\n", HISTORIES, steps);
    return 0;
}
