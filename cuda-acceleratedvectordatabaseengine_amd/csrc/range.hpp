// range.hpp — vdb_ivf_range_search on one handle (range.cpp), for the C ABI entries
// (engine.cpp).
#pragma once

#include <memory>
#include <vector>

#include "engine.hpp"

// What vdb_ivf_range_search hands out: host memory only, nothing of the handle.
struct vdb_range_result {
    uint32_t n = 0;
    std::vector<uint64_t> lims;  // n + 1
    std::vector<float> distances;
    std::vector<uint64_t> ids;
};

namespace vdbe {

constexpr uint64_t kRangeAutoReserve = 1ull << 18;  // reserve == 0: entries of the hit buffer a batch starts with

// The calling thread's latest range_search (vdb_range_last_timing).
struct RangeTiming {
    double scan_ms = 0.0;        // pair grouping + ivf_range_scan, summed over the call's batches, re-runs included
    double order_ms = 0.0;       // the sorts, range_dedup and range_finish, summed over the call's batches
    uint64_t pairs_scanned = 0;  // (query, row) distances computed, re-runs included
    uint64_t hits = 0;           // entries returned
    uint32_t reruns = 0;         // batches scanned again with a larger hit buffer
};
extern thread_local RangeTiming g_range_timing;

// The calling thread's latest range_search with `screen` (vdb_range_screen_last_timing).
struct RangeScreenTiming {
    double pairs_ms = 0.0;          // launch_screen_pairs, summed over the call's batches
    double bound_ms = 0.0;          // ivf_range_screen
    double recheck_ms = 0.0;        // ivf_range_recheck, re-runs included
    uint64_t pairs_bounded = 0;     // (query, row) pairs the bound kernel judged
    uint64_t candidates = 0;        // ... and could not discard (of every batch it ran on)
    uint32_t screened_batches = 0;  // batches served through the screen
    uint32_t exact_batches = 0;     // batches served by the exact scan (no live screen, or too many candidates)
};
extern thread_local RangeScreenTiming g_range_screen_timing;

// Caller holds h.mu and has made h's device current. For each of the n host queries on its
// own: every entry (d, id) of the result vdb_ivf_search gives that query with the same nprobe
// and a k no smaller than the rows it probes, keeping id != UINT64_MAX and d <= radius, in that
// result's order. Reads the handle only, and has synchronised h.stream when it returns or
// throws. Refuses what it does not serve (a NaN radius, a group, a shard, a file home, the
// list-cache tier) before any device work.
// d_allow / d_allowed (both or neither): a prepared filter's per-block allow masks and per-list
// allowed counts on the handle's device. The result is then the one of a handle with the same
// centroids and metric that stores only the allowed rows in their original order.
// screen: serve the batches through the screen the handle holds at this moment, if it holds a
// live one (range_route.hpp); the result is the same, bit for bit.
std::unique_ptr<vdb_range_result> range_search(vdb_ivf& h, const float* queries, uint32_t n, uint32_t nprobe,
                                               float radius, uint64_t reserve,
                                               const unsigned long long* d_allow = nullptr,
                                               const uint32_t* d_allowed = nullptr, bool screen = false);

}  // namespace vdbe
