// exhaustive_screen.hpp — vdb_ivf_search_exhaustive_screened on one handle
// (exhaustive_screen.cpp), for the C ABI entry (engine.cpp).
#pragma once

#include "engine.hpp"

namespace vdbe {

// The calling thread's latest search_exhaustive_screened (vdb_exhaustive_screen_last_timing).
struct ExhScreenTiming {
    double pairs_ms = 0.0;        // launch_screen_pairs, summed over the call's tiles (HIP events)
    double thresh_ms = 0.0;       // ivf_exh_screen_thresh + ivf_exhaustive_merge
    double bound_ms = 0.0;        // ivf_exh_screen_bound
    double select_ms = 0.0;       // ivf_exh_screen_select
    uint64_t rows_bounded = 0;    // (query, stored row) pairs the bound kernel judged
    uint64_t candidates = 0;      // ... and could not discard (of every tile it ran on)
    uint32_t screened_tiles = 0;  // tiles served through the screen
    uint32_t exact_tiles = 0;     // tiles served by the exact exhaustive scan (no live screen, or too many candidates)
};
extern thread_local ExhScreenTiming g_exh_screen_timing;

// search_exhaustive's result, bit for bit (exhaustive.hpp), reading the screen's shadow instead of
// every fp32 row while the handle holds a live screen (exhaustive_screen_route.hpp); otherwise
// search_exhaustive itself. `reserve`: candidate entries per query, 0 the library's choice. Caller
// holds h.mu and has made h's device current. Reads the handle only: it never builds, refreshes
// or releases a screen. Has synchronised h.stream when it returns or throws.
void search_exhaustive_screened(vdb_ivf& h, const float* queries, uint32_t n, uint32_t k, uint64_t reserve,
                                float* distances, uint64_t* ids);

}  // namespace vdbe
