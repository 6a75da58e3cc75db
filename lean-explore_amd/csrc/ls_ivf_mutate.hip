// ls_ivf_mutate.hip — rows join and leave a built IVF handle (include/leansearch_ivf_add.h,
// include/leansearch_ivf_remove.h; the handle: ls_ivf_state.h; the kernels: ls_rows.hip).
//
// Both calls place the rows on the host (ls_ivf_add_plan.h: the old rows of every list followed by its new ones;
// ls_ivf_remove_plan.h: the survivors of every list, renumbered densely), build the new list-major storage BESIDE the
// handle with one launch of the row mover - over the old stored rows and, for an add, a flat index of the new ones -,
// bring the existing subsets along (an add shifts their storage rows list by list; a removal compacts them with a
// count and a scatter launch each) and swap everything in under the mutex: the handle ls_ivf_create would have made
// from all rows / from the survivors, or, on any failure, the handle as it was.
//
// Two invariants hold in both: nothing of the handle or its subsets changes before the swap, and nothing in the swap
// can fail or allocate.
#include "ls_ivf_state.h"
#include "ls_ivf_add_plan.h"
#include "ls_ivf_remove_plan.h"

#include "../../include/leansearch_ivf_add.h"
#include "../../include/leansearch_ivf_remove.h"

// ---- the restage path both calls share --------------------------------------------------------------------------------
struct ivf_remove_subset {  // the compacted form of one existing subset
    ls_ivf_subset* ss = nullptr;
    int64_t m = 0;
    u32 *d_soff = nullptr, *d_srow = nullptr, *d_sid = nullptr;
    std::vector<int64_t> sizes, top_rows;
    std::vector<u32> soff;  // host copy of d_soff (lives until its upload on the handle's stream is done)
};

// What a call builds BESIDE the handle; whatever it still holds when it goes out of scope is released (every early
// return, and after the swap: the storage and the subset arrays the handle gave up).
struct ivf_parts {
    std::vector<float> step;     // the handle's sq8 step (empty for the other dtypes): the new storage encodes alike
    ls_index* rows = nullptr;    // the new storage, n_new rows
    u32 *d_src = nullptr, *d_ids = nullptr, *d_off = nullptr;
    std::vector<int64_t> top_rows;
    bool timed = false;          // the event pair was recorded around the row mover
    // ls_ivf_add
    ls_index* fresh = nullptr;   // a flat index of the new rows: converted / encoded and uploaded by the usual code
    u32* d_shift = nullptr;
    u32 *un_row = nullptr, *un_id = nullptr;  // the union step's arrays at the new size (small-batch option)
    unsigned short* un_mask = nullptr;
    // ls_ivf_remove
    u32 *d_dst_of = nullptr, *d_counts = nullptr;
    std::vector<ivf_remove_subset> subs;
    const float* stp() const { return step.empty() ? nullptr : step.data(); }
    ~ivf_parts() {
        if (fresh) ls_destroy(fresh);
        if (rows) ls_destroy(rows);
        for (void* p : {(void*)d_src, (void*)d_ids, (void*)d_off, (void*)d_shift, (void*)un_row, (void*)un_id,
                        (void*)un_mask, (void*)d_dst_of, (void*)d_counts})
            (void)hipFree(p);
        for (ivf_remove_subset& u : subs)
            for (void* p : {(void*)u.d_soff, (void*)u.d_srow, (void*)u.d_sid}) (void)hipFree(p);
    }
};

// prepare: the handle's sq8 step comes down; `fresh`, a flat index of the n_add new rows in stored format (an add; it
// precedes the destination so that device memory is taken in the order it always was); the empty destination (same
// dtype, same step) with room for n_new rows; the tables the row mover and the handle need; top_rows of the new sizes
static int ivf_prepare(ls_ivf* v, ivf_parts& t, const float* rows_add, int64_t n_add, const std::vector<int64_t>& sizes,
                       int64_t n_new, const char* who) {
    ivf_top_rows(sizes, t.top_rows);
    if (v->dtype == LS_DTYPE_SQ8) {
        t.step.resize((size_t)v->d);
        LS_HIP(hipMemcpy(t.step.data(), v->rows->d_sq8_step, sizeof(float) * (size_t)v->d, hipMemcpyDeviceToHost));
    }
    if (n_add > 0)
        if (int rc = ls_i_create(&t.fresh, rows_add, false, n_add, v->d, v->dtype, t.stp(), v->device, who)) return rc;
    if (int rc = ls_i_create(&t.rows, nullptr, false, 0, v->d, v->dtype, t.stp(), v->device, who)) return rc;
    if (int rc = ls_i_reserve_rows(t.rows, n_new)) return rc;
    LS_HIP(hipSetDevice(v->device));
    const size_t nn = (size_t)std::max<int64_t>(n_new, 1);
    LS_HIP(hipMalloc((void**)&t.d_src, sizeof(u32) * nn));
    LS_HIP(hipMalloc((void**)&t.d_ids, sizeof(u32) * nn));
    LS_HIP(hipMalloc((void**)&t.d_off, sizeof(u32) * ((size_t)v->nlist + 1)));
    return LS_OK;
}

// move: the tables go up, then ONE launch of the row mover on the handle's stream, between the event pair when the
// handle profiles (nothing is timed when no row moves). b: the new rows of an add, whose mover also writes the new
// storage row -> original row table from the old one; null for a removal, where the host has that table: `ids`.
static int ivf_move(ls_ivf* v, ivf_parts& t, const std::vector<u32>& src, const u32* ids, const std::vector<u32>& off_new,
                    const void* b, int64_t n_a, int64_t n_new) {
    if (n_new > 0) {
        LS_HIP(hipMemcpy(t.d_src, src.data(), sizeof(u32) * (size_t)n_new, hipMemcpyHostToDevice));
        if (!b) LS_HIP(hipMemcpy(t.d_ids, ids, sizeof(u32) * (size_t)n_new, hipMemcpyHostToDevice));
    }
    LS_HIP(hipMemcpy(t.d_off, off_new.data(), sizeof(u32) * ((size_t)v->nlist + 1), hipMemcpyHostToDevice));
    if (v->profiling)
        for (hipEvent_t& e : v->move_ev)
            if (!e) LS_HIP(hipEventCreate(&e));
    hipStream_t s = v->stream;
    LS_HIP(hipDeviceSynchronize());  // (the uploads and the zero pad rows so far: none of them went to this stream)
    t.timed = v->profiling && n_new > 0;
    if (t.timed) LS_HIP(hipEventRecord(v->move_ev[0], s));
    if (int rc = ls_launch_rows_move(v->rows->d_corpus, b, t.rows->d_corpus, t.d_src, b ? v->d_ids : nullptr,
                                     b ? t.d_ids : nullptr, n_a, n_new, v->rows->g, v->rows->n_cu, s))
        return rc;
    if (t.timed) LS_HIP(hipEventRecord(v->move_ev[1], s));
    return LS_OK;
}

// swap: the handle takes the new storage and tables; t keeps what the handle gave up. Nothing here fails or allocates.
// ms / bytes: the call's own pair of the handle (the last add's or the last removal's).
static void ivf_swap(ls_ivf* v, ivf_parts& t, std::vector<int64_t>& sizes, std::vector<u32>& off_new, int64_t n_new,
                     float* ms, int64_t* bytes) {
    *ms = 0.0f;
    *bytes = 0;
    if (t.timed && hipEventElapsedTime(ms, v->move_ev[0], v->move_ev[1]) == hipSuccess)
        *bytes = 2 * n_new * (int64_t)v->rows->g.chunks * 16;
    t.rows->n = n_new;
    std::swap(v->rows, t.rows);
    std::swap(v->d_ids, t.d_ids);
    std::swap(v->d_off, t.d_off);
    (void)hipFree(v->d_S);  // [n]: allocated again at next need
    v->d_S = nullptr;
    (void)hipFree(v->d_RS);  // (the range search's vectors: [rs_vecs][stride of n])
    v->d_RS = nullptr;
    v->rs_vecs = 0;
    v->n = n_new;
    v->sizes.swap(sizes);
    v->off.swap(off_new);
    v->top_rows.swap(t.top_rows);
}

// ---- ls_ivf_add ---------------------------------------------------------------------------------------------------------
// (under the handle's mutex, arguments checked) Nothing of the handle changes before the swap, and nothing in the swap
// can fail.
static int ivf_add_locked(ls_ivf* v, const float* rows, int64_t n_add, const int32_t* assign) {
    const int64_t n_old = v->n, n_new = n_old + n_add;
    const int32_t d = v->d, nlist = v->nlist;
    LS_HIP(hipSetDevice(v->device));
    std::vector<int32_t> own;
    if (!assign) {
        own.resize((size_t)n_add);
        if (int rc = ivf_default_assign(v->cent, v->metric, nlist, v->device, rows, n_add, d, own.data())) return rc;
        LS_HIP(hipSetDevice(v->device));
        assign = own.data();
    }
    // placement: host work, as in ivf_build (O(n) integers; the handle keeps `assign` on the host anyway)
    ls_ivf_add_plan plan;
    ls_ivf_add_plan_make(v->off.data(), nlist, assign, n_add, plan);
    v->assign.reserve((size_t)n_new);  // (the swap appends without allocating)
    ivf_parts t;
    if (int rc = ivf_prepare(v, t, rows, n_add, plan.sizes, n_new, "ls_ivf_add")) return rc;
    if (!v->subsets.empty()) {
        LS_HIP(hipMalloc((void**)&t.d_shift, sizeof(u32) * (size_t)nlist));
        LS_HIP(hipMemcpy(t.d_shift, plan.shift.data(), sizeof(u32) * (size_t)nlist, hipMemcpyHostToDevice));
    }
    const int64_t un_cap = (n_new + 15) / 16 * 16 + 16;
    if (v->cand_queries >= LS_MQ_NQ) {  // the small-batch option was switched on at some time: its arrays sized by n
        LS_HIP(hipMalloc((void**)&t.un_row, sizeof(u32) * (size_t)un_cap));
        LS_HIP(hipMalloc((void**)&t.un_id, sizeof(u32) * (size_t)un_cap));
        LS_HIP(hipMalloc((void**)&t.un_mask, sizeof(unsigned short) * (size_t)un_cap));
    }
    if (int rc = ivf_move(v, t, plan.src, nullptr, plan.off_new, t.fresh->d_corpus, n_old, n_new)) return rc;
    hipStream_t s = v->stream;
    LS_HIP(hipStreamSynchronize(s));
    // existing subsets keep their rows; the lists moved apart (last: past this point only a lost device fails)
    for (auto& kv : v->subsets)
        if (kv.second->m > 0)
            if (int rc = ls_launch_ivf_subset_shift(kv.second->d_soff, t.d_shift, kv.second->d_srow, nlist, s)) return rc;
    LS_HIP(hipStreamSynchronize(s));
    int64_t inexact_add = 0;  // (bf16 rows: what encoding the new rows lost, ls_ivf_bf16_inexact)
    if (v->dtype == LS_DTYPE_BF16 && t.fresh)
        if (int rc = ls_i_bf16_inexact(t.fresh, &inexact_add)) return rc;
    // ---- swap ----
    v->bf16_inexact += inexact_add;
    ivf_swap(v, t, plan.sizes, plan.off_new, n_new, &v->add_ms, &v->add_bytes);
    if (t.un_row) {
        std::swap(v->un.row, t.un_row);
        std::swap(v->un.id, t.un_id);
        std::swap(v->un.mask, t.un_mask);
        v->un.cap = un_cap;
    }
    v->assign.insert(v->assign.end(), assign, assign + n_add);
    return LS_OK;
}

// ---- ls_ivf_remove ------------------------------------------------------------------------------------------------------
// (under the handle's mutex, arguments checked, at least one row below n selected) Nothing of the handle or its subsets
// changes before the swap, and nothing in the swap can fail.
static int ivf_remove_locked(ls_ivf* v, const uint8_t* bitmap, int64_t nbytes) {
    const int64_t n_old = v->n;
    const int32_t nlist = v->nlist;
    LS_HIP(hipSetDevice(v->device));
    // placement: host work, as in ivf_build and ls_ivf_add (O(n) integers over the host tables)
    ls_ivf_remove_plan plan;
    ls_ivf_remove_plan_make(v->assign.data(), n_old, nlist, v->off.data(), bitmap, nbytes, plan);
    const int64_t n_new = plan.n_new;
    ivf_parts t;
    if (int rc = ivf_prepare(v, t, nullptr, 0, plan.sizes, n_new, "ls_ivf_remove")) return rc;
    for (auto& kv : v->subsets)
        if (kv.second->m > 0) {
            t.subs.emplace_back();
            t.subs.back().ss = kv.second;
        }
    if (!t.subs.empty()) {
        LS_HIP(hipMalloc((void**)&t.d_dst_of, sizeof(u32) * (size_t)n_old));
        LS_HIP(hipMalloc((void**)&t.d_counts, sizeof(u32) * (size_t)nlist));
        LS_HIP(hipMemcpy(t.d_dst_of, plan.dst_of.data(), sizeof(u32) * (size_t)n_old, hipMemcpyHostToDevice));
    }
    if (int rc = ivf_move(v, t, plan.src, plan.ids_new.data(), plan.off_new, nullptr, 0xffffffffll, n_new)) return rc;
    hipStream_t s = v->stream;
    // existing subsets: the host does not keep their rows. Count the survivors of every list, size the new arrays from
    // the counts, scatter in order.
    std::vector<u32> counts((size_t)nlist);
    for (ivf_remove_subset& u : t.subs) {
        std::vector<u32>& soff_new = u.soff;
        soff_new.assign((size_t)nlist + 1, 0);
        const ls_ivf_subset* ss = u.ss;
        if (int rc = ls_launch_list_count(ss->d_soff, ss->d_srow, ss->m, t.d_dst_of, t.d_counts, nlist, s)) return rc;
        LS_HIP(hipMemcpyAsync(counts.data(), t.d_counts, sizeof(u32) * (size_t)nlist, hipMemcpyDeviceToHost, s));
        LS_HIP(hipStreamSynchronize(s));
        u.sizes.resize((size_t)nlist);
        for (int32_t l = 0; l < nlist; ++l) {
            if ((int64_t)counts[(size_t)l] > ss->sizes[(size_t)l]) {
                ls_set_error("ls_ivf_remove: list %d of a subset counts %u survivors of %lld rows", l, counts[(size_t)l],
                             (long long)ss->sizes[(size_t)l]);
                return LS_ERR_HIP;
            }
            u.sizes[(size_t)l] = counts[(size_t)l];
            soff_new[(size_t)l + 1] = soff_new[(size_t)l] + counts[(size_t)l];
        }
        u.m = soff_new[(size_t)nlist];
        ivf_top_rows(u.sizes, u.top_rows);
        const size_t mm = (size_t)std::max<int64_t>(u.m, 1);
        LS_HIP(hipMalloc((void**)&u.d_soff, sizeof(u32) * ((size_t)nlist + 1)));
        LS_HIP(hipMalloc((void**)&u.d_srow, sizeof(u32) * mm));
        LS_HIP(hipMalloc((void**)&u.d_sid, sizeof(u32) * mm));
        LS_HIP(hipMemcpyAsync(u.d_soff, soff_new.data(), sizeof(u32) * ((size_t)nlist + 1), hipMemcpyHostToDevice, s));
        if (u.m > 0)
            if (int rc = ls_launch_list_scatter(ss->d_soff, ss->d_srow, ss->m, t.d_dst_of, t.d_ids, u.d_soff, u.d_srow,
                                                u.d_sid, nlist, s))
                return rc;
    }
    LS_HIP(hipStreamSynchronize(s));
    // ---- swap ----
    ivf_swap(v, t, plan.sizes, plan.off_new, n_new, &v->rm_ms, &v->rm_bytes);
    for (ivf_remove_subset& u : t.subs) {
        ls_ivf_subset* ss = u.ss;
        ss->m = u.m;
        std::swap(ss->d_soff, u.d_soff);
        std::swap(ss->d_srow, u.d_srow);
        std::swap(ss->d_sid, u.d_sid);
        ss->sizes.swap(u.sizes);
        ss->top_rows.swap(u.top_rows);
    }
    v->assign.swap(plan.assign_new);  // (the union step's arrays keep their larger capacity)
    return LS_OK;
}

extern "C" {

int ls_ivf_remove(ls_ivf* v, const uint8_t* bitmap, int64_t nbytes, int64_t* out_removed) {
    if (!v || nbytes < 0 || (nbytes > 0 && !bitmap)) {
        ls_set_error("ls_ivf_remove: bad argument (handle %s, nbytes=%lld, bitmap %s)", v ? "set" : "null", (long long)nbytes,
                     bitmap ? "set" : "null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    const int64_t removed = ls_ivf_remove_count(bitmap, nbytes, v->n);
    if (removed == 0) {  // nothing selected below ntotal: nothing touched
        if (out_removed) *out_removed = 0;
        return LS_OK;
    }
    if (int rc = ls_i_check_device(v->device)) return rc;
    ls_device_guard guard;
    try {
        const int rc = ivf_remove_locked(v, bitmap, nbytes);
        if (rc == LS_OK && out_removed) *out_removed = removed;
        return rc;
    } catch (const std::bad_alloc&) {  // (before the swap: it allocates nothing)
        ls_set_error("ls_ivf_remove: out of host memory");
        return LS_ERR_INVALID_ARG;
    }
}

int ls_ivf_remove_last_kernel_ms(ls_ivf* v, float* compact_ms, int64_t* compact_bytes) {
    if (!v) {
        ls_set_error("ls_ivf_remove_last_kernel_ms: handle is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    if (compact_ms) *compact_ms = v->rm_ms;
    if (compact_bytes) *compact_bytes = v->rm_bytes;
    return LS_OK;
}

int ls_ivf_add(ls_ivf* v, const float* rows, int64_t n_add, const int32_t* assign) {
    if (!v || n_add < 0 || (n_add > 0 && !rows)) {
        ls_set_error("ls_ivf_add: bad argument (handle %s, n_add=%lld, rows %s)", v ? "set" : "null", (long long)n_add,
                     rows ? "set" : "null");
        return LS_ERR_INVALID_ARG;
    }
    if (n_add == 0) return LS_OK;
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->n + n_add >= 0xffffffffll) {
        ls_set_error("ls_ivf_add: %lld rows exceed the 2^32-1 rows one handle can index", (long long)(v->n + n_add));
        return LS_ERR_INVALID_ARG;
    }
    if (assign)
        for (int64_t r = 0; r < n_add; ++r)
            if (assign[r] < 0 || assign[r] >= v->nlist) {
                ls_set_error("ls_ivf_add: assign[%lld] = %d is not a list (nlist %d)", (long long)r, assign[r], v->nlist);
                return LS_ERR_INVALID_ARG;
            }
    if (int rc = ls_i_check_device(v->device)) return rc;
    ls_device_guard guard;
    try {
        return ivf_add_locked(v, rows, n_add, assign);
    } catch (const std::bad_alloc&) {  // (before the swap: it allocates nothing)
        ls_set_error("ls_ivf_add: out of host memory");
        return LS_ERR_INVALID_ARG;
    }
}

int ls_ivf_add_last_kernel_ms(ls_ivf* v, float* merge_ms, int64_t* merge_bytes) {
    if (!v) {
        ls_set_error("ls_ivf_add_last_kernel_ms: handle is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    if (merge_ms) *merge_ms = v->add_ms;
    if (merge_bytes) *merge_bytes = v->add_bytes;
    return LS_OK;
}

}  // extern "C"
