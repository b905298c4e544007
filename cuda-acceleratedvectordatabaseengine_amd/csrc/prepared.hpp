// prepared.hpp — prepared id filters (prepared.cpp), for the C ABI entries (engine.cpp): the
// allow masks vdb_ivf_search_filtered takes per call, taken once and kept on the device for
// vdb_ivf_search_prepared and vdb_ivf_range_search_prepared.
#pragma once

#include <memory>

#include "engine.hpp"
#include "range.hpp"

// What vdb_ivf_filter_create hands out: the per-block allow masks and the per-list allowed
// counts on the handle's device, and what tells whether they still describe the handle. It
// holds nothing else of the handle and may outlive it.
struct vdb_filter {
    vdb_ivf* h = nullptr;       // an address to compare and, while the epoch is live, the handle
    uint64_t epoch = 0;         // filter_epoch.hpp: the handle's when the masks were taken
    uint64_t arena_blocks = 0;  // the handle's block geometry and row count then
    uint64_t total = 0;
    uint32_t nlist = 0;
    int device = 0;
    uint64_t n_allowed = 0;  // stored rows the filter lets through
    vdbe::DevBuf<unsigned long long> allow;  // [arena_blocks]
    vdbe::DevBuf<uint32_t> allowed;          // [nlist]
};

namespace vdbe {

// The calling thread's latest filter_create (vdb_filter_create_last_timing).
struct FilterCreateTiming {
    double sort_ms = 0.0;  // the device sort of the ids (HIP events)
    double mark_ms = 0.0;  // ivf_filter_mark + ivf_filter_count (HIP events)
};
extern thread_local FilterCreateTiming g_filter_create_timing;

// True while `f` describes its handle: the handle exists, no call has moved its rows since
// (filter_epoch.hpp) and its block geometry and row count are the filter's. Reads the handle
// only once the epoch says it exists.
bool filter_live(const vdb_filter& f);

// Caller holds h.mu and has made h's device current. The masks of the rows the id set allows
// (include: a row whose id is listed; else a row whose id is not), `ids` a host array or, with
// device_ids, an array on h's device that is complete before the call; any order, repeats and
// ids that are not stored ignored. Reads the handle only; has synchronised h.stream when it
// returns or throws. Refuses what search_filtered refuses.
std::unique_ptr<vdb_filter> filter_create(vdb_ivf& h, const uint64_t* ids, uint64_t n, bool include, bool device_ids);

// Caller holds the lock of the handle both belong to and has made its device current.
// op: VDB_FILTER_AND / _OR / _ANDNOT.
std::unique_ptr<vdb_filter> filter_combine(const vdb_filter& a, const vdb_filter& b, int op);

// search_filtered / range_search over the filter's rows. Same caller duties and refusals; a
// filter of another handle is VDB_ERR_INVALID_ARGUMENT, a stale one VDB_ERR_STATE.
void search_prepared(vdb_ivf& h, const vdb_filter& f, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                     float* distances, uint64_t* ids);
std::unique_ptr<vdb_range_result> range_search_prepared(vdb_ivf& h, const vdb_filter& f, const float* queries,
                                                        uint32_t n, uint32_t nprobe, float radius, uint64_t reserve,
                                                        bool screen = false);

}  // namespace vdbe
