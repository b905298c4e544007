// multi_filter_screen.hpp — vdb_ivf_search_prepared_multi_screened on one handle
// (multi_filter_screen.cpp), for the C ABI entry (engine.cpp).
#pragma once

#include "filter_screen.hpp"
#include "multi_filter.hpp"

namespace vdbe {

// search_prepared_multi's result, bit for bit, through the screen the handle holds at this
// moment if it holds a live one (filter_screen_route.hpp); otherwise search_prepared_multi
// itself. Same caller duties and refusals as search_prepared_multi. reserve: entries of a
// batch's candidate buffer (0: filter_cand_cap's choice). Builds, refreshes and releases nothing
// of the handle; fills the calling thread's FilterScreenTiming as search_prepared_screened does
// and its FilterTiming as search_prepared_multi does.
void search_prepared_multi_screened(vdb_ivf& h, const vdb_filter* const* filters, uint32_t n_filters,
                                    const uint32_t* filter_of, const float* queries, uint32_t n, uint32_t nprobe,
                                    uint32_t k, uint64_t reserve, float* distances, uint64_t* ids);

}  // namespace vdbe
