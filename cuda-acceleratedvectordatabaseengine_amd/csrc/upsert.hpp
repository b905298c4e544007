// upsert.hpp — vdb_ivf_upsert(_device) on one handle (upsert.cpp), for the C ABI entries
// (engine.cpp).
#pragma once

#include "engine.hpp"

namespace vdbe {

// The calling thread's latest upsert, step by step (vdb_upsert_last_timing).
struct UpsertTiming {
    double resolve_ms = 0.0;    // sort, winners, pack (HIP events; the host's sum of the counts is inside)
    double mark_ms = 0.0;       // ivf_remove_mark (HIP events); 0 on an empty index
    double plan_ms = 0.0;       // the host plan
    double move_ms = 0.0;       // the compact of the survivors and the scatter of the winners (HIP events)
    uint64_t rows_kept = 0;     // stored rows the compact pass moved
    uint64_t rows_written = 0;  // winners the scatter wrote
};
extern thread_local UpsertTiming g_upsert_timing;

// Caller holds h.mu, has made h's device current and has refused what the call does not serve
// (a file home, a shard, a group, n >= 2^31). d_v ([n][dim] floats) and d_ids ([n]) are memory
// of h's device, complete on h.stream or before the call; n > 0. Afterwards h is the handle
// remove_ids(every id of d_ids) followed by add(the winners: for every distinct id its last
// entry, in request order) leaves, with one pass over the arena. replaced / inserted (each may
// be null): stored rows that went, winners that came. Has synchronised h.stream on return.
void upsert(vdb_ivf& h, const float* d_v, const uint64_t* d_ids, uint64_t n, uint64_t* replaced, uint64_t* inserted);

}  // namespace vdbe
