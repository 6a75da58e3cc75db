// ls_index.h — private: the index handle behind include/leansearch.h's opaque `ls_index`, shared by
// ls_api.hip (single-device orchestration; ls_callers.hip, ls_batched.hip, ls_debug.hip are its other parts) and
// ls_shard.hip (the row-sharded group handle).
#pragma once
#include "ls_common.h"
#include "../../include/leansearch_l2.h"  // LS_METRIC_*
#include "ls_scan_call_plan.h"  // LS_NSETS, LS_MQ_KEEP_SLOTS and what a scan-path call launches (ls_api.hip)

#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <deque>
#include <mutex>
#include <vector>

struct ls_shard_group;  // ls_shard.hip
struct ls_subset_state; // ls_subset.hip: the handle's row subsets (ls_subset_create) and their scratch
struct ls_req;          // ls_callers.hip: one queued synchronous host search
struct ls_range_scratch;  // ls_range.hip: what a handle's range searches reuse (below)

// Scratch generations of the second scan lane (ls_index::lanes): candidates and bounds only - a lane launch
// writes no score vectors -, allocated at the lane's first launch.
#define LS_LANE_SETS 2
// Unchecked batched calls a handle carries before it checks them itself (a check drains the pipeline:
// ~2 batch times). Every slot owns a flag slice (capped at 16 MB in total: fewer slots for huge
// batches) and a copy of the raw queries; the copies are allocated in blocks of LS_BC_QKEEP_BLOCK slots
// as the backlog actually grows, so a caller that checks regularly never pays for the rest.
#define LS_BC_SLOTS 1024
#define LS_BC_QKEEP_BLOCK 64
#ifndef LS_BC_LANES
// Scratch sets that consecutive LS_FLAG_PIPELINE batches rotate over. Four, so that nothing a batch
// has to wait for is younger than two batches: prep(i+4) rewrites the prepared queries pass(i) read,
// pass(i+4) the queues select(i) read. (With two, prep(i+2) had to wait for pass(i) itself, and the
// ~20 us a cross-stream dependency takes to resolve landed between two passes.)
#define LS_BC_LANES 4
#endif
#define LS_BC_SETS (1 + LS_BC_LANES)  // batched scratch sets: 0 = caller's stream, then the lanes
#define LS_PROF_MAX 4096

// Buffers of ONE synchronous host search (ls_search) in flight. Two slots: while the call that owns slot
// A still polls for its results, the next caller may already queue its launch with slot B (round 5:
// two callers used to ping-pong as two single launches with the GPU idle in between). Slot c also owns
// scan scratch generation c: a same-launch selection's retry reads its generation's score vector and
// granules after the host has seen its answer, so nothing else may touch that generation meanwhile.
// Lock order: slot mutex(es) first, then ls_index::mu.
struct ls_host_slot {
    std::mutex mu;  // held from the enqueue until the results have been handed back
    hipStream_t stream = nullptr;  // overlapped calls run on their slot's own stream: the next call's scan starts
                                   // while this call's selection workgroup and tail are still running
    float* h_q = nullptr;      size_t h_q_cap = 0;      // pinned query copy (the kernels may read it directly)
    float* d_qraw = nullptr;   size_t qraw_cap = 0;     // device query copy (floats)
    float* d_out_s = nullptr;  int64_t* d_out_i = nullptr;  size_t out_cap = 0;  // nq*k (large results)
    float* h_out_s = nullptr;  int64_t* h_out_i = nullptr;  size_t h_out_cap = 0;  // pinned
    u32* h_done = nullptr;     // pinned [LS_QUERIES_PER_LAUNCH_MAX]: completion words
    u32 done_seq = 0;
    ls_out_gran* h_out_g = nullptr;  size_t h_out_g_cap = 0;  // pinned: result granules of a spinning call
    std::vector<ls_fin_batch> retry_groups;  // the call's same-launch jobs, one batch per launch (LS_DONE_RETRY)
};
#define LS_HOST_SLOTS 2

// Who is calling the scan path (ls_i_search_on_stream, scan_search_on_stream and what they reach), handed down as an
// argument: nothing about the call in flight is kept in the handle. The defaults are a device-output call that is final
// in stream order. DESIGN.md 1 ("Who calls the scan path") lists what every call site passes.
struct ls_scan_call {
    u32* done = nullptr;              // a synchronous host call that polls: its completion words, one per query (pinned) ...
    ls_out_gran* out_gran = nullptr;  // ... and its result granules, k per query (set together with done)
    u32 done_seq = 0;                 // ... and the sequence number both carry
    std::vector<ls_fin_batch>* retry = nullptr;  // where a host call keeps its same-launch jobs, one batch per launch
    int32_t gen = -1;                 // >= 0: the scan scratch generation the call owns (an overlapped host call); -1: rotate
    bool reserving = false;           // a query served a second time (a host call's retry, mq_repair): its launch keeps
                                      // its score vectors, its selection takes its own launch, it is final when queued
    bool repairable = false;          // a device-output call whose results may be repaired after it was queued
                                      // (ls_scan_call_repairable): its launches may keep their raw queries instead of score vectors
    bool host_api = false;            // a synchronous host call: the batched path repairs before it returns, whatever the flags
};

// Selection jobs of the youngest launch of one stream that have not been launched yet: they ride on that stream's next
// scan launch, or ls_i_flush_pending launches them on their own. Three of them: the one-stream pipeline's and the lanes'.
struct ls_fin_queue {
    int n = 0;  // jobs waiting (queries of the launch)
    ls_fin_batch jobs{};
    hipStream_t stream = nullptr;  // where that launch went
    // the waiting jobs as the batch of a launch of their own (LDS for the full LS_FINAL_CAP keys); none wait afterwards
    ls_fin_batch take() {
        ls_fin_batch b = jobs;
        b.njobs = n;
        b.p0.keys_cap = LS_FINAL_CAP;
        n = 0;
        return b;
    }
};

struct ls_index {
    int32_t device = 0;
    int32_t n_cu = 256;
    int64_t n = 0;
    int32_t dtype = 0;
    int32_t metric = 0;  // LS_METRIC_* (include/leansearch_l2.h), fixed at creation: 1 = every score is a negated squared
                         // distance, every query is served alone by the scan path, results leave as distances (ls_l2_out)
    int64_t base = 0;
    ls_geom g{};
    void* d_corpus = nullptr;
    float* d_sq8_step = nullptr;  // LS_DTYPE_SQ8: the per-dimension step [d], fixed at creation (ls_sq8_scan.hip)
    unsigned long long* d_bf16_inexact = nullptr;  // LS_DTYPE_BF16: elements the encode kernel stored inexactly, over every
                                                   // row ever handed to create or add (ls_bf16_scan.hip, ls_bf16_inexact)
    int64_t cap_rows = 0;  // rows d_corpus has room for (+ LS_CORPUS_PAD_ROWS); >= n
    std::mutex mu;
    hipStream_t own_stream = nullptr;
    // synchronous host searches that arrive together are served as one batch (ls_search)
    std::mutex q_mu;
    std::condition_variable q_cv;
    std::deque<ls_req*> req_q;
    bool leader_active = false;
    std::atomic<uint64_t> q_epoch{0};  // bumped whenever the queue's state changes (arrivals too: the gathering leader counts them)
    std::atomic<int64_t> q_len{0};     // req_q.size(), readable without q_mu (the gathering leader polls it)
    std::atomic<uint64_t> lead_epoch{0};  // bumped when the leadership or a host slot comes free: what a QUEUED waiter polls
    int32_t calls_in_flight = 0;       // batches queued whose results have not been handed back yet (under q_mu)
    int64_t requests_in_flight = 0;    // ... and the requests in them
    int64_t peak_callers = 0;          // decaying maximum of (requests in flight + queued): the callers around lately
    std::chrono::steady_clock::time_point last_arrival{};  // (under q_mu) ...
    double arrival_gap_us = 1e4;       // ... running mean of the time between two ls_search arrivals
    uint64_t arrivals_seen = 0;
    uint32_t peak_decay = 0;
    int32_t opt_combine = 1;
    uint64_t n_combined_batches = 0, n_combined_requests = 0;
    std::atomic<int32_t> spinners{0};  // waiters polling right now (ls_spin_cap: as many as the process has CPUs for)
    uint64_t n_waiter_parks = 0;       // (under q_mu) debug counter 33
    uint64_t n_lead_wait_ns = 0, n_lead_call_ns = 0, n_lead_relock_ns = 0, n_lead_begin_ns = 0, n_lead_finish_ns = 0;  // (under q_mu) debug counters 28-30
    // non-null: this handle is a row-sharded GROUP (ls_create_sharded): `n`, `dtype`, `g` and
    // `device` (the primary shard's) describe the whole index, every other member below is unused
    // and the per-device sub-handles live in the group (ls_shard.hip)
    ls_shard_group* group = nullptr;

    // scratch (grown on demand, reused by every search on this handle)
    // per-query scan scratch, LS_NSETS generations: launch i's piggy-backed finalize of group i-1
    // reads one generation while its scan of group i fills the other
    struct scratch_set {
        float* d_S = nullptr;        // s_vecs score vectors, s_stride floats apart
        u64* d_cand = nullptr;       // max_blocks * LS_KP_MAX
        u64* d_bound = nullptr;      // max_blocks
        void* d_gran = nullptr;      // same-launch selection: LS_QUERIES_PER_LAUNCH_MAX * LS_GRAN_MAX tagged
                                     // 16-byte granules (ls_fin_params::gran), allocated at first use
        float* d_qpad = nullptr;     // padded query group of a ragged VALU group (8 x d floats)
        size_t qpad_cap = 0;
        hipStream_t last_stream = nullptr;  // stream of the last launch that used this generation: a launch
                                            // on another stream first waits (on the host) for that one
    } sets[LS_NSETS + LS_LANE_SETS];  // (the last LS_LANE_SETS: lane 1's, without d_S / d_gran)
    uint64_t set_rr = 0;
    int32_t last_set = 0;
    // batched (MFMA) path scratch, allocated on first use. Set 0 serves plain calls on the
    // caller's stream: a handle that only ever sees one stream pays nothing for sharing it; the
    // first call on a second stream synchronises the previous one and switches the set to
    // multi-stream mode, where `done` is recorded behind the last kernel of every call and
    // waited for by the next call's stream (an event record costs a few us of GPU time per
    // batch: a barrier packet with a release). Sets 1 .. LS_BC_LANES serve LS_FLAG_PIPELINE calls:
    // consecutive batches rotate over them (the three-stream chain, batched_search_on_stream).
    struct bc_set {
        void* d_qh = nullptr;      size_t qh_cap = 0;       // bytes: fp16 queries [nq_pad, d_pad]
        u64* d_queues = nullptr;   size_t queues_cap = 0;   // private candidate queues
        u32* d_counts = nullptr;   size_t counts_cap = 0;
        float* d_tau = nullptr;    size_t tau_cap = 0;
        u32* d_sample_top = nullptr; size_t sample_top_cap = 0;  // best sample scores per lane
        hipEvent_t done = nullptr;        // set 0, multi-stream mode
        hipStream_t last_stream = nullptr;  // where the set's results become final (the select's stream)
        bool used = false;
        bool multi_stream = false;
        // sets 1 .. LS_BC_LANES (LS_FLAG_PIPELINE): the three-stream chain, see batched_search_on_stream
        bool chain = false;
        bool sel_recorded = false;        // ev_sel carries a record
        hipEvent_t ev_prep = nullptr;     // the set's prep kernel is done: the caller may reuse its query buffer
        hipEvent_t ev_pass = nullptr;     // the set's pass is done (attached to its dispatch): the select may start
        hipEvent_t ev_sel = nullptr;      // the set's select is done (recorded on the select stream)
    } bc_sets[LS_BC_SETS];
    // one batch between "sample pass + tau queued" and "pass + select queued" (batched_search_on_stream)
    struct bc_stage {
        bool active = false;
        int set_id = 0, lane = 0;
        bool f32 = false, top2 = false;
        int64_t nq = 0, nq_pad = 0, rps = 0;
        int32_t k = 0;
        int nsplits = 0, sample_stride = 0, jrank = 0, keys_need = 0;
        u32* d_flags = nullptr;
        float* d_out_s = nullptr;
        int64_t* d_out_i = nullptr;
    };
    std::deque<bc_stage> held;  // pipelined batches whose pass is held back (at most two: see batched_search_on_stream)
    // LS_FLAG_PIPELINE batches: prep kernels, filter stages (MFMA passes, back to back) and selects each
    // have their own stream; the scratch sets 1 .. LS_BC_LANES alternate between consecutive batches
    hipStream_t chain_main[2] = {nullptr, nullptr};  // the chain's two lanes
    hipStream_t chain_sel = nullptr;                 // ... and its select stream
    hipEvent_t chain_in = nullptr;        // recorded on the caller's stream, waited for by the prep stream
    int32_t opt_fused = 1;                // pipelined fp16 batches of rows <= 768 bytes: a later batch's sample phase rides on the pass launch
    int32_t opt_wave_select = 1;          // one-wave select kernel (<= 48 VGPRs) where the shape allows
    uint64_t bc_lane_rr = 0;
    int32_t bc_last_set = 0;  // the set of the most recent batched call (ls_export_flags)
    u32* d_overflow = nullptr; size_t overflow_cap = 0;
    u32* h_overflow = nullptr; size_t h_overflow_cap = 0;  // pinned
    // async batched calls not yet checked: each keeps its own flag slice of d_overflow AND its own
    // copy of the raw queries (d_qkeep), so that several batches can be in flight before one
    // ls_check repairs whatever was flagged, whatever the caller did to its query buffer meanwhile
    struct batched_call {
        int64_t nq = 0;
        int32_t k = 0;
        uint32_t flags = 0;
        float* d_out_s = nullptr;
        int64_t* d_out_i = nullptr;
        hipStream_t stream = nullptr;
        int32_t slot = 0;
    };
    std::vector<batched_call> bc_pending;
    int64_t bc_slot_stride = 0;  // u32 per flag slot
    float* d_qkeep_blk[LS_BC_SLOTS / LS_BC_QKEEP_BLOCK] = {};  // each LS_BC_QKEEP_BLOCK x bc_qkeep_stride floats
    int64_t bc_qkeep_stride = 0;
    int bc_slots() const {  // slots in use for the current slot stride
        const int64_t by_mem = (4ll << 20) / (bc_slot_stride > 0 ? bc_slot_stride : 1);
        return (int)(by_mem < 16 ? 16 : (by_mem > LS_BC_SLOTS ? LS_BC_SLOTS : by_mem));
    }
    u32* d_last_flags = nullptr;  // flag slice of the most recent batched call (ls_export_flags)
    int64_t last_flags_n = 0;
    uint64_t n_batched_fallback = 0;  // queries repaired by the scan path (host counter)
    int32_t n_batched_launches = 0;   // kernel launches of the most recent batched call (counted)
    int32_t last_path = 0;            // most recent search: 1 scan path, 2 fp16 MFMA path, 3 fp32 MFMA path
    uint64_t n_chunked_calls = 0;     // batched calls cut into sub-batches (candidate-queue capacity)
    uint64_t n_launches_total = 0;    // kernel launches queued by searches on this handle
    int32_t opt_gemm = 1;             // allow the batched MFMA path
    int32_t opt_spec_tau = 1;         // speculative (verified) sample threshold

    ls_fin_queue fin;                  // the one-stream pipeline's selection jobs
    hipStream_t last_scan_stream = nullptr;  // where the youngest scan-path launch that left jobs waiting went, a lane's
                                             // included: mq_repair waits for it
    // Scan lanes: pipelined scan-path calls that are one launch without score vectors (single query, ls_mq,
    // ls_mq16; never LS_FLAG_INORDER) go to chain_main[0] and chain_main[1] in turn, and launch j+1 depends on
    // nothing launch j does: its workgroups take the CU slots those of j leave, so the memory stream does not
    // drain at a launch's edges. Each lane by itself is the one-stream pipeline: its launch j+2 carries the
    // selection of its launch j (a kernel boundary apart), over the lane's own two scratch generations (lane 0:
    // sets[0..1], lane 1: sets[LS_NSETS..]). The caller's stream hands a launch its queries (copied into the
    // launch's slot of d_mq_keep, then lane_in) and waits for the PREVIOUS call's launch (lane_out) behind
    // that record - see lane_begin (ls_api.hip) for the order and why it matters. Which calls take the lanes:
    // ls_scan_call_make_plan (ls_scan_call_plan.h).
    struct scan_lane {
        ls_fin_queue fin;              // the lane's own pipeline (fin.stream: chain_main[lane])
        uint32_t gen_rr = 0;
    } lanes[2];
    bool lanes_active = false;         // launches may be in flight on the lanes (until ls_i_lanes_drain)
    hipStream_t lanes_caller = nullptr;  // the stream the active lanes are fed from
    uint64_t lane_rr = 0;              // launch j -> lane j & 1
    hipEvent_t lane_in[4] = {}, lane_out[4] = {};  // rings: queries ready (caller's stream) / launch done (its lane)
    uint32_t lane_ev_rr = 0;
    hipEvent_t lane_join[2] = {};      // a flush of both lanes: lane 1 done -> lane 0 runs the jobs -> lane 1 may go on
    int32_t lane_prev_out = -1;        // lane_out slot of the previous call: what the caller's stream waits for next
    int32_t opt_lanes = 1;             // debug option 24
    uint64_t n_lane_launches = 0;      // counter 35
    long long s_stride = 0;            // floats between the score vectors of one generation
    int32_t s_vecs = 0;                // score vectors per generation: 8 (one VALU scan group) until a launch that keeps
                                       // its score vectors serves more (ls_mq, LS_FLAG_ASYNC-only calls): grow_score_vectors
    int32_t opt_multi_query = 1;       // several queries per corpus pass (groups of 8 / 4)
    int32_t opt_mq = 1;                // fp32 index: 2..16 queries per pass on the f32 matrix cores (ls_mq.hip)
    int32_t opt_mq32 = 1;              // ... up to 32 queries per pass (two B blocks; debug option 22)
    uint64_t n_mq_launches = 0;
    int32_t opt_mq16 = 0;              // fp16 index: 1..32 queries per pass on the f16 matrix cores (ls_mq16.hip;
                                       // ls_set_f16_small_batch, off by default: other bits than the VALU scan's)
    uint64_t n_mq16_launches = 0;      // ... its launches (counter 34)
    int32_t opt_mq8 = 0;               // sq8 index: 2..16 queries per pass on the f32 matrix cores (ls_mq8.hip;
                                       // ls_set_sq8_small_batch, off by default: the same bits as the sq8 scan)
    uint64_t n_mq8_launches = 0;       // ... its launches (counter 36)
    int32_t opt_mqs = 0;               // fp32 index, subset search: 2..16 queries per pass over the selected rows
                                       // (ls_mq_subset.hip; ls_set_subset_small_batch, off by default: the same bits)
    uint64_t n_mqs_launches = 0;       // ... its passes (counter 37)
    int32_t opt_l2_batch = 0;          // L2 index: VALU scan groups of 8 / 4 / 1 queries per pass (ls_l2_batch.hip;
                                       // ls_set_l2_small_batch, off by default: the same bits as the single-query L2 scan)
    uint64_t n_l2_group_launches = 0;  // ... its launches that carried more than one query (counter 38)
    int32_t opt_scan_skip_scores = 1;  // ... single-query launches of pipelined / synchronous device calls too
    int32_t opt_mq_skip_scores = 1;    // ... whose selection jobs ride along write no score vectors (debug option 19)
    uint64_t n_mq_reserved = 0;        // queries of such launches served again on the scan kernel (counter 25)
    uint64_t n_mq_skipped_repairs = 0; // ... whose output rows a later pipelined call had been given meanwhile (counter 26)
    // (read under q_mu by ls_search, written under the handle's mutex by ls_debug_option: atomics)
    std::atomic<int32_t> opt_early_cap{8};   // ls_search: callers up to which a second batch goes early (debug option 21)
    std::atomic<int32_t> opt_full_early{1};  // ls_search: a queue that fills a pass goes at once behind the call in flight (debug option 23)
    std::atomic<int32_t> opt_gather{1};      // ls_search: concurrent callers are gathered into one pass (debug option 20)
    double call_us_est = 0.0;          // running estimate of one combined call, begin to finish (under q_mu)
    // ... and so do pipelined / synchronous DEVICE-output calls (ls_scan_call::repairable): the launch keeps its raw
    // queries (slot of d_mq_keep), an unproven query raises its word in d_mq_flags, mq_repair (ls_check, the end of a
    // synchronous call, ring full) serves it again in place. LS_FLAG_ASYNC alone keeps the score vectors:
    // its results are promised in stream order.
    struct mq_pending_call {
        int slot, nq;
        int32_t k;
        uint32_t flags;
        float* d_out_s;
        int64_t* d_out_i;
        hipStream_t stream;
    };
    std::vector<mq_pending_call> mq_pend;
    float* d_mq_keep = nullptr;        // [LS_MQ_KEEP_SLOTS][16][mq_keep_d]
    int32_t mq_keep_d = 0;
    u32* d_mq_flags = nullptr;         // [LS_MQ_KEEP_SLOTS][16]
    u32* h_mq_flags = nullptr;         // pinned mirror; its LAST word is raised by any flagged job (ls_fin_params::repair_any)
    int32_t opt_same_launch = 1;       // synchronous host calls: the selection rides on its own query's scan launch
    uint64_t n_forced_checks = 0;           // checks of pending batched calls the library ran on its own
    uint64_t n_same_launch_retries = 0;     // host calls that had to launch the stand-alone finalize
    unsigned long long n_spin_timeouts = 0; // host calls whose 2 ms of polling ran out (they slept in hipStreamSynchronize; counter 27)
    u32 gran_tag = 0;                  // tag of the last same-launch selection (ls_fin_params::tag; never 0)
    int32_t max_blocks = 0;
    u32* d_counters = nullptr;                        // [0] finalize slow-path count
    ls_host_slot hs[LS_HOST_SLOTS];
    std::atomic<unsigned> hs_rr{0};
    int32_t opt_overlap_calls = 1;     // synchronous host calls may overlap two deep (debug option 17)
    uint64_t n_overlapped_calls = 0;   // host calls that were queued while another one was still in flight

    // options / instrumentation
    int32_t opt_kprime = 0;  // 0 = automatic
    int32_t opt_blocks = 0;  // 0 = automatic (scan workgroups per launch)
    int32_t opt_force_slow = 0;
    int32_t opt_overlap = 1;    // finalize of group i-1 rides on the scan launch of group i
    int32_t opt_alternate = 0;  // alternate sweep direction between consecutive scans
    uint64_t sweep_count = 0;
    // profiling: hipEvent pairs around EVERY scan launch (and the finalize after it), recorded
    // on the stream the kernels run on, up to LS_PROF_MAX launches; read by ls_last_kernel_ms
    bool profiling = false;
    std::vector<hipEvent_t> prof_ev;  // 2 events per launch: begin, end
    size_t prof_n = 0;
    ls_subset_state* subsets = nullptr;  // (under the handle's mutex) created by the first ls_subset_create
    ls_range_scratch* range = nullptr;   // (under the handle's mutex) created by the first ls_range_search
    // ls_remove (ls_remove.hip): the staging slab's rows (0: automatic) and what the most recent call did (ls_remove_last)
    int64_t rm_slab_rows = 0;
    int64_t rm_moved = 0, rm_slabs = 0, rm_bytes = 0;
    float rm_ms = 0.0f;
};


// Every synchronous host call in flight has handed its results back (both host slots), then the handle's
// mutex: what every entry point that touches the scan scratch, the corpus or the base takes.
struct ls_quiesce {
    std::unique_lock<std::mutex> a, b, m;
    explicit ls_quiesce(ls_index* ix) {
        std::lock(ix->hs[0].mu, ix->hs[1].mu);
        a = std::unique_lock<std::mutex>(ix->hs[0].mu, std::adopt_lock);
        b = std::unique_lock<std::mutex>(ix->hs[1].mu, std::adopt_lock);
        m = std::unique_lock<std::mutex>(ix->mu);
    }
};

// Restores the calling thread's current HIP device on every exit path: the entry points that make a handle's device
// current (the group's hop over the shards' devices), and PyTorch shares this per-thread state with us.
struct ls_device_guard {
    int prev = -1;
    ls_device_guard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~ls_device_guard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// ls_set_profiling: the next group of `per` timing events of `ev` (`used` groups are taken), created at first need
static inline int ls_prof_events(std::vector<hipEvent_t>& ev, size_t used, size_t per, hipEvent_t** out) {
    while (ev.size() < per * (used + 1)) {
        hipEvent_t e;
        LS_HIP(hipEventCreate(&e));
        ev.push_back(e);
    }
    *out = &ev[per * used];
    return LS_OK;
}

template <typename T>
static inline int ls_grow(T** p, size_t* cap, size_t need) {
    if (need <= *cap) return LS_OK;
    if (*p) LS_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    size_t want = need + need / 2;
    LS_HIP(hipMalloc((void**)p, want * sizeof(T)));
    *cap = want;
    return LS_OK;
}
template <typename T>
static inline int ls_grow_pinned(T** p, size_t* cap, size_t need, unsigned flags = hipHostMallocDefault) {
    if (need <= *cap) return LS_OK;
    if (*p) LS_HIP(hipHostFree(*p));
    *p = nullptr;
    *cap = 0;
    size_t want = need + need / 2;
    LS_HIP(hipHostMalloc((void**)p, want * sizeof(T), flags));
    *cap = want;
    return LS_OK;
}

// ---- internals of ls_api.hip that the group handle drives. The caller holds the mutex of the
// handle it passes and has made that handle's device current. ---------------------------------
int ls_i_check_device(int32_t device);
// (ls_api.hip) what ls_create / ls_create_from_device / ls_create_sq8 share. sq8: step = host [d] or null (trained
// from the rows), ignored for the other dtypes
int ls_i_create(ls_index** out, const float* corpus, bool on_device, int64_t n, int32_t d, int32_t dtype,
                const float* step, int32_t device, const char* who, int32_t metric = 0);
// An L2 handle's scores as the caller sees them: distances. s = -dist inside the library, -FLT_MAX in the padding slots;
// 0.0f - s gives +0.0 for an exact match and +FLT_MAX for the padding.
static inline float ls_l2_out(float s) { return 0.0f - s; }
// (ls_api.hip) room for `rows` >= ix->n stored rows in d_corpus (the rows it has are carried over), the zero pad rows
// behind row `rows`, score vectors of that length. ix->n stays: the caller writes rows [ix->n, rows) of d_corpus in the
// stored layout itself and then sets n (ls_ivf_add gathers a merged index into a new handle this way). On failure the
// handle is unchanged.
int ls_i_reserve_rows(ls_index* ix, int64_t rows);
// (ls_bf16_scan.hip) a bf16 handle's count of inexactly stored elements; the caller holds the handle's ls_quiesce or owns
// the handle outright
int ls_i_bf16_inexact(ls_index* ix, int64_t* out);
int ls_i_check_search_args(const ls_index* ix, const void* q, int64_t nq, int32_t k, uint32_t flags,
                           const void* os, const void* oi);
bool ls_i_batched_eligible(const ls_index* ix, int64_t nq, int32_t k);
int ls_i_search_on_stream(ls_index* ix, const float* d_q, int64_t nq, int32_t k, uint32_t flags,
                          float* d_out_s, int64_t* d_out_i, hipStream_t s, const ls_scan_call& call);
// ls_search_device without its argument checks and without its refusal of L2 handles (the IVF coarse stage of an L2
// handle: the scores written are -distance)
int ls_i_search_device(ls_index* ix, const void* d_q, int64_t nq, int32_t k, uint32_t flags, void* d_out_scores,
                       void* d_out_indices, void* stream);
int ls_i_flush_pending(ls_index* ix);  // (the scan lanes' jobs too)
int ls_i_lanes_drain(ls_index* ix);    // ... and wait for both lanes: the next launch may go anywhere
int ls_i_chain_streams(ls_index* ix);   // chain_main[0..1], chain_sel, chain_in: created at first use
int ls_i_flush_deferred(ls_index* ix);
int ls_i_settle(ls_index* ix);          // queued and repairable work finished under the current base and switches
int ls_i_drain_for_move(ls_index* ix);  // before stored rows move: lanes dry, repairs done, the device idle
int ls_i_batched_repair(ls_index* ix, const ls_scan_call& call);  // (call: of the search it is nested in; ls_scan_call{} from outside any search)
int ls_i_export_flags(ls_index* ix, void* d_dst, int64_t nq, hipStream_t s);
int ls_i_grow_score_vectors(ls_index* ix, int need);  // score vectors per scratch generation, grown on demand
// (ls_batched.hip)
int64_t ls_i_bc_chunk(const ls_index* ix, int64_t nq, int32_t k);  // queries one batched call takes at once (0: none)
int ls_i_batched_search_on_stream(ls_index* ix, const float* d_q, int64_t nq, int32_t k, uint32_t flags,
                                  float* d_out_s, int64_t* d_out_i, hipStream_t s, const ls_scan_call& call);
// (what the synchronous host path, ls_callers.hip, asks about a call's shape)
int ls_i_scan_path_max_nq(const ls_index* ix, int32_t k);            // queries ONE scan-path launch carries at this k
int64_t ls_i_scan_group_count(const ls_index* ix, int64_t nq, int32_t k);  // launches the scan path cuts nq queries into

// ---- ls_remove in two phases (ls_remove.hip), so that a group handle moves no row before every member is ready. The
// caller holds the single-device handle's ls_quiesce and has made its device current.
struct ls_remove_prep;
// Drains the handle's pending work, then plans the removal of the rows the bits [bit0, bit0 + ix->n) of the bitmap
// select and allocates everything it needs: the survivor list, the staging slab, every existing subset's new list
// (device and host copies), the timing events. Nothing of the handle or its subsets has changed when it returns,
// whatever it returns.
int ls_i_remove_prepare(ls_index* ix, const uint8_t* bitmap, int64_t nbytes, int64_t bit0, ls_remove_prep** out);
int64_t ls_i_remove_prepared_rows(const ls_remove_prep* p);  // rows the handle will hold
// Moves the rows (launches and device-to-device copies on the handle's stream only), swaps the subset lists and the
// row count in, and frees the plan. An error leaves the handle fit only for ls_destroy.
int ls_i_remove_commit(ls_remove_prep* p);
void ls_i_remove_discard(ls_remove_prep* p);
void ls_i_remove_group_subsets(ls_index* ix);  // a group's subsets take their row counts from their members'

// ---- the group handle (ls_shard.hip); every function takes the GROUP's ls_index -----------------
int ls_group_remove(ls_index* ix, const uint8_t* bitmap, int64_t nbytes, int64_t* out_removed);
int ls_group_search(ls_index* ix, const float* q, bool q_on_host, int64_t nq, int32_t k,
                    uint32_t flags, float* out_s, int64_t* out_i, hipStream_t s);
int ls_replica_search(ls_index* ix, const float* q, int64_t nq, int32_t k, uint32_t flags, float* out_s,
                      int64_t* out_i);  // replicated handles: synchronous host calls, round-robin
bool ls_group_is_replicated(const ls_index* ix);
int ls_group_check(ls_index* ix, hipStream_t s);
void ls_group_destroy(ls_index* ix);
int ls_group_add(ls_index* ix, const float* rows, int64_t n_add);
int ls_group_reconstruct(ls_index* ix, int64_t row0, int64_t count, float* out);
int ls_group_set_base(ls_index* ix, int64_t base);
int ls_group_debug_option(ls_index* ix, int32_t which, int32_t value);
int ls_group_set_f16_small_batch(ls_index* ix, int32_t enable);
int ls_group_scan_path_max_nq(const ls_index* ix, int32_t k);         // the narrowest shard's ls_i_scan_path_max_nq
int ls_i_set_f16_small_batch(ls_index* ix, int32_t enable, bool size_score_vectors);  // (ls_switch.hip: a group's members)
int64_t ls_group_debug_counter(ls_index* ix, int32_t which);
int ls_group_set_profiling(ls_index* ix, int32_t enabled);
int ls_group_last_kernel_ms(ls_index* ix, float* scan_ms, float* total_ms);
// Merge `lists` sorted [nq, k] result lists (device memory on the current device, list l at byte offsets
// l * stride_s / l * stride_i) into dst on stream s: one launch while lists * k keys fit its LDS, else rounds of merges
// through `tmp` (two ping-pong buffer pairs, grown on demand, owned by the caller). ls_shard.hip.
struct ls_merge_scratch {
    char* s[2] = {nullptr, nullptr};
    size_t s_cap[2] = {0, 0};
    char* i[2] = {nullptr, nullptr};
    size_t i_cap[2] = {0, 0};
    void release() {
        for (int r = 0; r < 2; ++r) {
            (void)hipFree(s[r]);
            (void)hipFree(i[r]);
            s[r] = i[r] = nullptr;
            s_cap[r] = i_cap[r] = 0;
        }
    }
};
int ls_i_merge_rounds(const float* in_s, const int64_t* in_i, int64_t stride_s, int64_t stride_i, int lists, int64_t nq,
                      int32_t k, float* dst_s, int64_t* dst_i, ls_merge_scratch& tmp, hipStream_t s);
ls_index* ls_group_member(ls_index* ix, int32_t g);         // shard / replica g's single-device handle
int64_t ls_group_member_row0(const ls_index* ix, int32_t g);  // its first row, relative to the group's base

// ---- what every scan-path launch and its selection jobs take from the handle (ls_api.hip, ls_subset.hip) ------------------
// The scratch part of a launch's arguments: generation `st`, `blocks` workgroups that emit `kprime` keys each
static inline void ls_fill_scratch_args(ls_scan_args& a, const ls_index* ix, const ls_index::scratch_set& st, int blocks, int kprime) {
    a.d_S = st.d_S;
    a.s_stride = ix->s_stride;
    a.d_cand = st.d_cand;
    a.c_stride = (long long)ix->max_blocks * LS_KP_MAX;
    a.d_bound = st.d_bound;
    a.b_stride = ix->max_blocks;
    a.blocks = blocks;
    a.kprime = kprime;
}
// ... and the selection jobs of that launch's `real` queries over n rows: results [real, k] from out_s / out_i on, row
// numbers + base, S the score vectors the launch wrote (null: none). A stand-alone launch's job; whoever lets the jobs
// ride, answer through completion words or raise repair words adds that on top. (The group's jobs differ by whole-query
// displacements only: job 0 + strides, ls_fin_batch)
static inline void ls_fill_fin_jobs(ls_fin_batch& jobs, const ls_index* ix, const ls_index::scratch_set& st, int blocks, int kprime,
                                    long long n, int k, long long base, float* out_s, int64_t* out_i, const float* S, int real) {
    jobs = ls_fin_batch{};
    ls_fin_params& p = jobs.p0;
    p.S = S;
    p.n = n;
    p.cand = st.d_cand;
    p.bound = st.d_bound;
    p.blocks = blocks;
    p.kprime = kprime;
    p.k = k;
    p.keys_cap = LS_FINAL_CAP;
    p.force_slow = ix->opt_force_slow;
    p.base = base;
    p.out_scores = out_s;
    p.out_indices = (long long*)out_i;
    p.counters = ix->d_counters;
    jobs.S_stride = ix->s_stride;
    jobs.cand_stride = (long long)ix->max_blocks * LS_KP_MAX;
    jobs.bound_stride = ix->max_blocks;
    jobs.gran_stride = (long long)LS_GRAN_MAX * 16;
    jobs.njobs = real;
    for (int i = 0; i < LS_QUERIES_PER_LAUNCH_MAX; ++i) jobs.idx[i] = (unsigned char)i;
}

// ---- range search (ls_range.hip; include/leansearch_range.h) ----------------------------------------------------
// What the range searches of one handle (flat or IVF) reuse, under that handle's mutex, on that handle's device.
struct ls_range_result;
struct ls_range_scratch {
    float* h_q = nullptr;        size_t hq_cap = 0;    // pinned: the flat scans read the call's queries from here
    u32* d_cnt = nullptr;        size_t cnt_cap = 0;   // [group][slabs] hits of every slab
    long long* d_off = nullptr;  size_t off_cap = 0;   // [group][slabs] their exclusive prefix
    long long* h_total = nullptr;                      // pinned [LS_RANGE_GROUP]: the hits of every query of the group
    float* d_scores = nullptr;   size_t scores_cap = 0;  // one group's results, query after query
    long long* d_rows = nullptr; size_t rows_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // profiling: around count + offsets, around emit
};
void ls_i_range_scratch_free(ls_range_scratch* rs);  // (the handle's device is current)
ls_range_result* ls_i_range_result_new(int64_t nq);  // lims all zero, no hits
// One group of G <= LS_RANGE_GROUP queries, queries [q0, q0 + G) of `res`, whose scans were queued on s and write the
// score vectors d_S + j * s_stride (n floats each): count and offsets, one wait, the device result buffers grown to the
// group's hits, emit and the copy into `res` at its lims, one wait. Rows come out as (map ? map[pos] : pos) + base.
void ls_i_range_l2_out(ls_range_result* res, int64_t q0, int G);  // (L2 handles: -distance -> distance)
int ls_i_range_collect(ls_range_scratch& rs, const float* d_S, long long s_stride, long long n, int G, float radius,
                       const u32* map, long long base, bool prof, ls_range_result* res, int64_t q0, hipStream_t s);

// ---- subset search (ls_subset.hip, ls_scan.hip) ---------------------------------------------------------------
int ls_i_pick_kprime(const ls_index* ix, int blocks, int keff);  // k' of a single-query scan launch (ls_api.hip)
ls_mq_in ls_i_mq_in(const ls_index* ix, bool rowlist);            // the handle as ls_mq_plan.h's input (ls_api.hip)
void ls_i_subsets_free(ls_index* ix);                             // ls_destroy
// ls_launch_scan with one query (a.nq == 1, no riding jobs) over the m rows of the ascending list d_list
int ls_launch_scan_subset(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                          hipStream_t s);
