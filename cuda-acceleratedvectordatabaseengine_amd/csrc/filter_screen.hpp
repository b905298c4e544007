// filter_screen.hpp — vdb_ivf_search_prepared_screened on one handle (filter_screen.cpp), for
// the C ABI entries (engine.cpp).
#pragma once

#include "prepared.hpp"

namespace vdbe {

// The calling thread's latest search_prepared_screened (vdb_filter_screen_last_timing).
struct FilterScreenTiming {
    double pairs_ms = 0.0;          // launch_screen_pairs, summed over the call's batches
    double thresh_ms = 0.0;         // ivf_filter_screen_thresh (+ ivf_filter_screen_tau)
    double bound_ms = 0.0;          // ivf_filter_screen_bound
    double select_ms = 0.0;         // the candidates' sort + ivf_filter_screen_select
    uint64_t pairs_bounded = 0;     // (pair, allowed row) pairs the bound kernel judged
    uint64_t candidates = 0;        // ... and could not discard (of every batch it ran on)
    uint32_t screened_batches = 0;  // batches served through the screen
    uint32_t exact_batches = 0;     // batches served by the masked exact scan (no live screen, or too many candidates)
};
extern thread_local FilterScreenTiming g_filter_screen_timing;

// search_prepared's result, bit for bit, through the screen the handle holds at this moment if
// it holds a live one (filter_screen_route.hpp); otherwise search_prepared's path. Same caller
// duties and refusals as search_prepared. reserve: entries of a batch's candidate buffer (0:
// filter_cand_cap's choice). Builds, refreshes and releases nothing of the handle; fills the
// calling thread's FilterTiming as search_prepared does.
void search_prepared_screened(vdb_ivf& h, const vdb_filter& f, const float* queries, uint32_t n, uint32_t nprobe,
                              uint32_t k, uint64_t reserve, float* distances, uint64_t* ids);

}  // namespace vdbe
