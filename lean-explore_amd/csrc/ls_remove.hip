// ls_remove.hip — ls_remove (include/leansearch_remove.h): rows leave a built flat handle and the corpus is compacted
// IN PLACE in HBM, through a bounded staging buffer. Everything runs on the handle's own stream.
//
//   survivors  the handle's slice of the bitmap, complemented, goes through ls_subset_create's own compaction
//              (ls_i_subset_compact, ls_subset.hip): src[s], the old row of new row s, ascending.
//   rows       slab after slab of destination rows from the first removed row r0 upwards (ls_remove_plan.h): the row
//              mover (ls_rows.hip) copies the old rows src[a .. a + c) into the staging buffer in STORED format and a
//              device-to-device copy writes the staging buffer back to rows [a, a + c). Then the LS_CORPUS_PAD_ROWS
//              rows behind the last row are zeroed.
//   subsets    src is scattered into dst_of[old row] = new row (LS_ROWS_GONE elsewhere); per existing subset the list
//              compaction (ls_rows.hip) counts, per segment of LS_RM_SEG positions, the positions whose row survives,
//              ls_subset.hip's scan kernel turns the counts into offsets, and the scatter writes dst_of[row] at offset
//              + rank. The list stays ascending (the renumbering is monotone).
//
// Two phases: ls_i_remove_prepare makes the plan and every allocation, the subsets' new lists included, and changes
// nothing; ls_i_remove_commit moves the rows and swaps the lists and the row count in. A group handle (ls_shard.hip)
// prepares every member before it commits one. Every index comes from ls_remove_plan.h.
#include "ls_subset_state.h"
#include "ls_remove_plan.h"
#include "../../include/leansearch_remove.h"

#include <memory>

// ---- the two phases ---------------------------------------------------------------------------------------------------
struct ls_remove_prep {
    ls_index* ix = nullptr;
    int64_t n_old = 0, n_new = 0, r0 = 0, R = 0;
    u32* d_src = nullptr;     // [n_new]
    void* d_stage = nullptr;  // [R] stored rows
    struct sub {
        ls_subset* ss = nullptr;
        u32* d_new = nullptr;
        std::vector<u32> h_new;
        int64_t m_new = 0;
    };
    std::vector<sub> subs;
    hipEvent_t ev[2] = {nullptr, nullptr};  // ls_set_profiling: around the row moves
};

void ls_i_remove_discard(ls_remove_prep* p) {
    if (!p) return;
    (void)hipSetDevice(p->ix->device);
    (void)hipFree(p->d_src);
    (void)hipFree(p->d_stage);
    for (auto& s : p->subs) (void)hipFree(s.d_new);
    for (hipEvent_t e : p->ev)
        if (e) (void)hipEventDestroy(e);
    delete p;
}

int64_t ls_i_remove_prepared_rows(const ls_remove_prep* p) { return p->n_new; }

// the new list of one existing subset, beside the old one: device and host copies
static int prep_subset(ls_remove_prep* p, ls_remove_prep::sub& u, const u32* d_dst_of, hipStream_t s) {
    const ls_subset* ss = u.ss;
    if (ss->m <= 0) return LS_OK;
    const long long groups = ls_remove_segs(ss->m);
    u32* d_counts = nullptr;
    u32 total = 0;
    auto body = [&]() -> int {
        LS_HIP(hipMalloc((void**)&d_counts, sizeof(u32) * (size_t)(groups + 1)));
        if (int rc = ls_launch_list_count(nullptr, ss->d_list, ss->m, d_dst_of, d_counts, groups, s)) return rc;
        if (int rc = ls_launch_subset_scan(d_counts, groups, d_counts + groups, s)) return rc;
        LS_HIP(hipMemcpyAsync(&total, d_counts + groups, sizeof(u32), hipMemcpyDeviceToHost, s));
        LS_HIP(hipStreamSynchronize(s));
        u.m_new = total;
        if (total > 0) {
            LS_HIP(hipMalloc((void**)&u.d_new, sizeof(u32) * (size_t)total));
            // (the scan left the segments' exclusive offsets in d_counts and the total in slot [groups])
            if (int rc = ls_launch_list_scatter(nullptr, ss->d_list, ss->m, d_dst_of, nullptr, d_counts, u.d_new, nullptr,
                                                groups, s))
                return rc;
            u.h_new.resize((size_t)total);
            LS_HIP(hipMemcpyAsync(u.h_new.data(), u.d_new, sizeof(u32) * (size_t)total, hipMemcpyDeviceToHost, s));
            LS_HIP(hipStreamSynchronize(s));
        }
        return LS_OK;
    };
    const int rc = body();
    (void)hipFree(d_counts);
    return rc;
}

int ls_i_remove_prepare(ls_index* ix, const uint8_t* bitmap, int64_t nbytes, int64_t bit0, ls_remove_prep** out) {
    *out = nullptr;
    int rc = ls_i_drain_for_move(ix);  // nothing queued on any stream may still read the rows that move
    if (rc != LS_OK) return rc;
    std::unique_ptr<ls_remove_prep, void (*)(ls_remove_prep*)> p(new ls_remove_prep(), ls_i_remove_discard);
    p->ix = ix;
    p->n_old = p->n_new = ix->n;
    p->r0 = ls_remove_first(bitmap, nbytes, bit0, ix->n);
    if (p->r0 < ix->n) {
        hipStream_t s = ix->own_stream;
        std::vector<uint8_t> slice;
        ls_remove_slice(bitmap, nbytes, bit0, ix->n, true, slice);
        if ((rc = ls_i_subset_compact(slice.data(), (int64_t)slice.size(), bit0 & 7, ix->n, s, &p->d_src, &p->n_new)))
            return rc;
        const int64_t row_bytes = (int64_t)ix->g.chunks * 16;
        p->R = ls_remove_slab_rows(ix->rm_slab_rows, row_bytes, ls_remove_moved(p->r0, p->n_new));
        if (p->R > 0) LS_HIP(hipMalloc(&p->d_stage, (size_t)p->R * (size_t)row_bytes));
        if (ix->profiling && p->R > 0)
            for (hipEvent_t& e : p->ev) LS_HIP(hipEventCreate(&e));
        if (ix->subsets && !ix->subsets->by_id.empty()) {
            u32* d_dst_of = nullptr;
            auto body = [&]() -> int {
                LS_HIP(hipMalloc((void**)&d_dst_of, sizeof(u32) * (size_t)p->n_old));
                LS_HIP(hipMemsetAsync(d_dst_of, 0xff, sizeof(u32) * (size_t)p->n_old, s));
                if (p->n_new > 0)
                    if (int r = ls_launch_remove_dst(p->d_src, p->n_new, d_dst_of, s)) return r;
                p->subs.reserve(ix->subsets->by_id.size());
                for (auto& kv : ix->subsets->by_id) {
                    p->subs.emplace_back();
                    p->subs.back().ss = kv.second;
                    if (int r = prep_subset(p.get(), p->subs.back(), d_dst_of, s)) return r;
                }
                return LS_OK;
            };
            rc = body();
            (void)hipFree(d_dst_of);
            if (rc != LS_OK) return rc;
        }
    }
    *out = p.release();
    return LS_OK;
}

int ls_i_remove_commit(ls_remove_prep* raw) {
    std::unique_ptr<ls_remove_prep, void (*)(ls_remove_prep*)> p(raw, ls_i_remove_discard);
    ls_index* ix = p->ix;
    ix->rm_moved = ix->rm_slabs = ix->rm_bytes = 0;
    ix->rm_ms = 0.0f;
    if (p->r0 >= p->n_old) return LS_OK;  // nothing selected: nothing touched
    hipStream_t s = ix->own_stream;
    const ls_geom& g = ix->g;
    const size_t row_bytes = (size_t)g.chunks * 16;
    char* corpus = (char*)ix->d_corpus;
    const int64_t slabs = ls_remove_slabs(p->r0, p->n_new, p->R);
    if (p->ev[0]) LS_HIP(hipEventRecord(p->ev[0], s));
    for (int64_t j = 0; j < slabs; ++j) {
        const int64_t a = ls_remove_slab_begin(p->r0, p->R, j), c = ls_remove_slab_count(p->r0, p->n_new, p->R, j);
        if (int rc = ls_launch_rows_move(corpus, nullptr, p->d_stage, p->d_src + a, nullptr, nullptr, 0xffffffffll, c, g,
                                         ix->n_cu, s))
            return rc;
        LS_HIP(hipMemcpyAsync(corpus + (size_t)a * row_bytes, p->d_stage, (size_t)c * row_bytes, hipMemcpyDeviceToDevice, s));
    }
    if (p->ev[1]) LS_HIP(hipEventRecord(p->ev[1], s));
    // the batched path reads whole tiles: LS_CORPUS_PAD_ROWS zero rows follow the last row
    LS_HIP(hipMemsetAsync(corpus + (size_t)p->n_new * row_bytes, 0, (size_t)LS_CORPUS_PAD_ROWS * row_bytes, s));
    LS_HIP(hipStreamSynchronize(s));
    for (auto& u : p->subs) {
        (void)hipFree(u.ss->d_list);
        u.ss->d_list = u.d_new;
        u.d_new = nullptr;
        u.ss->h_list.swap(u.h_new);
        u.ss->m = u.m_new;
    }
    ix->n = p->n_new;
    ix->rm_moved = ls_remove_moved(p->r0, p->n_new);
    ix->rm_slabs = slabs;
    if (p->ev[1]) {
        LS_HIP(hipEventElapsedTime(&ix->rm_ms, p->ev[0], p->ev[1]));
        ix->rm_bytes = 4 * ix->rm_moved * (int64_t)row_bytes;  // gather and write-back: each row read and written twice
    }
    return LS_OK;
}

static ls_subset* rm_find_subset(ls_index* ix, int32_t id) {
    if (!ix->subsets) return nullptr;
    auto it = ix->subsets->by_id.find(id);
    return it == ix->subsets->by_id.end() ? nullptr : it->second;
}

void ls_i_remove_group_subsets(ls_index* ix) {
    if (!ix->subsets) return;
    const bool repl = ls_group_is_replicated(ix);
    for (auto& kv : ix->subsets->by_id) {
        ls_subset* gs = kv.second;
        gs->m = 0;
        for (int g = 0; g < (int)gs->member.size(); ++g) {
            const ls_subset* ms = rm_find_subset(ls_group_member(ix, g), gs->member[g]);
            if (ms && (!repl || g == 0)) gs->m += ms->m;
        }
    }
}

extern "C" {

int ls_remove(ls_index* ix, const uint8_t* bitmap, int64_t nbytes, int64_t* out_removed) {
    if (!ix || nbytes < 0 || (nbytes > 0 && !bitmap)) {
        if (!ix)
            ls_set_error("ls_remove: bad argument (handle null)");
        else if (nbytes < 0)
            ls_set_error("ls_remove: bad argument (nbytes=%lld)", (long long)nbytes);
        else
            ls_set_error("ls_remove: bad argument (bitmap null with nbytes=%lld)", (long long)nbytes);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(ix->device)) return rc;
    ls_quiesce lk(ix);  // (no synchronous host call in flight, then the handle's mutex)
    ls_device_guard guard;
    if (ix->group) return ls_group_remove(ix, bitmap, nbytes, out_removed);
    LS_HIP(hipSetDevice(ix->device));
    ls_remove_prep* p = nullptr;
    if (int rc = ls_i_remove_prepare(ix, bitmap, nbytes, 0, &p)) return rc;
    const int64_t removed = ix->n - ls_i_remove_prepared_rows(p);
    if (int rc = ls_i_remove_commit(p)) return rc;
    if (out_removed) *out_removed = removed;
    return LS_OK;
}

int ls_subset_rows(ls_index* ix, int32_t subset, int64_t* out_rows) {
    if (!ix || !out_rows) {
        ls_set_error("ls_subset_rows: bad argument (%s)", !ix ? "handle null" : "out_rows null");
        return LS_ERR_INVALID_ARG;
    }
    ls_quiesce lk(ix);
    const ls_subset* ss = rm_find_subset(ix, subset);
    if (!ss) {
        ls_set_error("ls_subset_rows: no subset %d on this handle", subset);
        return LS_ERR_INVALID_ARG;
    }
    *out_rows = ss->m;
    return LS_OK;
}

int ls_remove_set_slab_rows(ls_index* ix, int64_t rows) {
    if (!ix || rows < 0) {
        ls_set_error("ls_remove_set_slab_rows: bad argument (%s)", !ix ? "handle null" : "rows < 0");
        return LS_ERR_INVALID_ARG;
    }
    ls_quiesce lk(ix);
    ix->rm_slab_rows = rows;
    for (int g = 0; g < ls_shard_count(ix); ++g) {
        ls_index* sub = ls_group_member(ix, g);
        std::lock_guard<std::mutex> lks(sub->mu);
        sub->rm_slab_rows = rows;
    }
    return LS_OK;
}

int ls_remove_last(ls_index* ix, int64_t* moved_rows, int64_t* slabs, float* move_ms, int64_t* move_bytes) {
    if (!ix) {
        ls_set_error("ls_remove_last: bad argument (handle null)");
        return LS_ERR_INVALID_ARG;
    }
    ls_quiesce lk(ix);
    int64_t moved = ix->rm_moved, ns = ix->rm_slabs, bytes = ix->rm_bytes;
    float ms = ix->rm_ms;
    for (int g = 0; g < ls_shard_count(ix); ++g) {
        ls_index* sub = ls_group_member(ix, g);
        std::lock_guard<std::mutex> lks(sub->mu);
        moved += sub->rm_moved;
        ns += sub->rm_slabs;
        bytes += sub->rm_bytes;
        ms += sub->rm_ms;
    }
    if (moved_rows) *moved_rows = moved;
    if (slabs) *slabs = ns;
    if (move_ms) *move_ms = ms;
    if (move_bytes) *move_bytes = bytes;
    return LS_OK;
}

}  // extern "C"
