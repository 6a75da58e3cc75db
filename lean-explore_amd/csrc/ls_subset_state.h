// ls_subset_state.h — private: a handle's row subsets (ls_subset_create) and their scratch, shared by ls_subset.hip
// (which owns them) and ls_remove.hip (which renumbers the lists when rows leave the handle).
#pragma once
#include "ls_index.h"

#include <map>
#include <vector>

struct ls_subset {
    int64_t m = 0;                  // selected rows
    int64_t n_at_create = 0;        // rows the handle had: a later ls_add does not extend the subset
    u32* d_list = nullptr;          // ascending local rows [m] (plain handle; device memory of the handle's device)
    std::vector<u32> h_list;        // host copy: maps the synchronous path's results back
    std::vector<int32_t> member;    // group handles: the subset's id on every member (shard / replica)
};
struct ls_subset_state {
    std::map<int32_t, ls_subset*> by_id;
    int32_t next_id = 1;
    float* d_q = nullptr;        size_t q_cap = 0;
    float* d_s = nullptr;        size_t s_cap = 0;
    int64_t* d_i = nullptr;      size_t i_cap = 0;
    float* h_q = nullptr;        size_t hq_cap = 0;   // pinned: the scan reads the queries from here
    float* h_s = nullptr;        size_t hs_cap = 0;   // pinned: the selection writes the results here
    int64_t* h_i = nullptr;      size_t hi_cap = 0;   // pinned
    float* d_gs = nullptr;       size_t gs_cap = 0;   // sharded: per-shard results on the primary [G, nq, k]
    int64_t* d_gi = nullptr;     size_t gi_cap = 0;
    ls_merge_scratch merge_tmp;                       // sharded: rounds of merges (G * k beyond one launch)
    uint32_t rr = 0;                                  // replicated: the replica that serves the next call
};

// (ls_subset.hip) The compaction of ls_subset_create on stream s of the current device: `slice` (host, `need` bytes)
// holds one bit per row, bit `off` + r for row r < n; the set rows, ascending, go to a new device list *d_list ([*m],
// null when *m == 0; the caller frees it). The three launches of the file header; synchronises s.
int ls_i_subset_compact(const uint8_t* slice, int64_t need, int64_t off, int64_t n, hipStream_t s, u32** d_list,
                        int64_t* m);
// (ls_subset.hip) counts[0 .. nwg) -> exclusive offsets in place, the total in *total: ls_subset_scan_kernel on s
int ls_launch_subset_scan(u32* d_counts, int64_t nwg, u32* d_total, hipStream_t s);
