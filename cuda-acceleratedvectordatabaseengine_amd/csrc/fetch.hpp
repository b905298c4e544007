// fetch.hpp — vdb_ivf_fetch_ids(_device) and vdb_ivf_search_ids on one handle (fetch.cpp), for
// the C ABI entries (engine.cpp).
#pragma once

#include "engine.hpp"

namespace vdbe {

// The calling thread's latest fetch_ids / search_ids, step by step (vdb_fetch_last_timing).
struct FetchTiming {
    double sort_ms = 0.0;     // the device sort of the requested ids (HIP events)
    double locate_ms = 0.0;   // the preset of loc + ivf_fetch_locate
    double gather_ms = 0.0;   // ivf_fetch_gather (search_ids: both of its passes)
    uint64_t rows_found = 0;  // request entries a stored row answered
};
extern thread_local FetchTiming g_fetch_timing;

// Caller holds h.mu and has made h's device current. For each of ids[0..n) (host memory, or
// with device_bufs memory of h's device that is complete) the stored row carrying it: the row
// at the lowest (list, position) where an id is stored more than once, dim zeros and found = 0
// where it is not stored. vectors ([n][dim] floats) and found ([n] bytes) may each be null;
// they live where ids lives. Returns the entries found. Reads the handle only, in whichever
// fp32 layout it holds, and has synchronised h.stream when it returns or throws. Refuses what
// it does not serve (n >= 2^31, the list-cache tier, a file home, a shard, a group) before any
// device work.
uint64_t fetch_ids(vdb_ivf& h, const uint64_t* ids, uint64_t n, bool device_bufs, float* vectors, uint8_t* found);

// vdb_ivf_search(rows of the found entries in request order, nprobe, k) with the rows taken
// from the gather's device buffer; entries that are not found get (FLT_MAX, UINT64_MAX) in
// every slot. Host buffers; found may be null. Same caller duties and refusals; the search
// itself is h.search_device on h.stream, so it does to the handle what any search does.
void search_ids(vdb_ivf& h, const uint64_t* ids, uint32_t n, uint32_t nprobe, uint32_t k, float* distances,
                uint64_t* result_ids, uint8_t* found);

}  // namespace vdbe
