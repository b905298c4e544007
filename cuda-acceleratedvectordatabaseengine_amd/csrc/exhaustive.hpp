// exhaustive.hpp — vdb_ivf_search_exhaustive on one handle (exhaustive.cpp), for the C ABI
// entry (engine.cpp).
#pragma once

#include "engine.hpp"

namespace vdbe {

// The calling thread's latest search_exhaustive (vdb_exhaustive_last_timing).
struct ExhaustiveTiming {
    double scan_ms = 0.0;         // ivf_exhaustive_scan, summed over the call's query tiles (HIP events)
    double merge_ms = 0.0;        // ivf_exhaustive_merge, summed over the call's query tiles
    uint64_t rows_scanned = 0;    // stored rows streamed: rows x query tiles
    uint64_t pairs_computed = 0;  // (query, stored row) distances: rows x n
};
extern thread_local ExhaustiveTiming g_exhaustive_timing;

// Caller holds h.mu and has made h's device current. Per query the first k entries, ascending
// by (d, id), of every stored row of every list, each id once at its smallest (d, id); unfilled
// slots (FLT_MAX, UINT64_MAX). Host buffers in and out. Reads the handle only, and has
// synchronised h.stream when it returns or throws. Refuses what it does not serve (the
// list-cache tier, a file home, a shard, a group) before any device work.
void search_exhaustive(vdb_ivf& h, const float* queries, uint32_t n, uint32_t k, float* distances, uint64_t* ids);

}  // namespace vdbe
