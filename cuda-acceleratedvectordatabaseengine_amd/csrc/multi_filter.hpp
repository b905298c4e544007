// multi_filter.hpp — vdb_ivf_search_prepared_multi on one handle (multi_filter.cpp), for the
// C ABI entry (engine.cpp): one masked scan for a batch whose queries each name their own
// prepared filter.
#pragma once

#include "prepared.hpp"

namespace vdbe {

// Caller holds h.mu, has made h's device current and has checked the pointers (no null entry in
// filters[0..n_filters), every filter_of[i] < n_filters). For every filter index f, the rows of
// the queries with filter_of[i] == f are, bit for bit, what search_prepared(h, *filters[f], those
// queries in call order, nprobe, k) returns; the stale-slot reuse never crosses filters. Host
// buffers in and out. Reads the handle and the filters only, and has synchronised h.stream when
// it returns or throws. Refuses what search_prepared refuses, for every filter of the table
// (referenced or not), before any device work; fills the calling thread's FilterTiming
// (mark_ms 0; pairs_scanned = per (query, probe) pair the rows the query's filter allows there).
void search_prepared_multi(vdb_ivf& h, const vdb_filter* const* filters, uint32_t n_filters, const uint32_t* filter_of,
                           const float* queries, uint32_t n, uint32_t nprobe, uint32_t k, float* distances,
                           uint64_t* ids);

}  // namespace vdbe
