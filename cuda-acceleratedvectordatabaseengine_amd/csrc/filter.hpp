// filter.hpp — vdb_ivf_search_filtered on one handle (filter.cpp), for the C ABI entry
// (engine.cpp).
#pragma once

#include "engine.hpp"

namespace vdbe {

// The calling thread's latest search_filtered, step by step (vdb_filter_last_timing).
struct FilterTiming {
    double mark_ms = 0.0;        // ivf_filter_mark + ivf_filter_count (HIP events)
    double scan_ms = 0.0;        // ivf_filter_scan (+ ivf_filter_fold), summed over the call's batches
    double merge_ms = 0.0;       // ivf_filter_merge + ivf_filter_carry, summed over the call's batches
    uint64_t pairs_scanned = 0;  // (query, row) distances computed
};
extern thread_local FilterTiming g_filter_timing;

// Caller holds h.mu and has made h's device current. The result of vdb_ivf_search(n, nprobe,
// k) on a handle with h's centroids, metric and stale_slots setting that stores only the rows
// the filter allows (include: a row whose id is in `sorted`; else a row whose id is not;
// sorted ascending, each id once), in their original order. Host buffers in and out. Reads
// the handle only, and has synchronised h.stream when it returns or throws. Refuses what it
// does not serve (k > 64, the list-cache tier, a file home, a shard, a group) before any
// device work.
void search_filtered(vdb_ivf& h, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                     const std::vector<uint64_t>& sorted, bool include, float* distances, uint64_t* ids);

// The second part of search_filtered, for masks already on h's device: d_allow[b] bit i = slot i
// of arena block b is allowed (no bit at or above the block's valid count), d_allowed[l] = the
// allowed rows of list l. Same caller duties, same result, same refusals (named after `call`);
// resets the calling thread's timing and fills its scan, merge and pairs (mark_ms stays 0).
// The masks may be null only where no scan runs (an empty handle, nprobe == 0, n == 0, k == 0).
void search_masked(vdb_ivf& h, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                   const unsigned long long* d_allow, const uint32_t* d_allowed, float* distances, uint64_t* ids,
                   const char* call = "search_filtered");

}  // namespace vdbe
