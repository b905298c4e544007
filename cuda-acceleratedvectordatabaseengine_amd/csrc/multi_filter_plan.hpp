// multi_filter_plan.hpp — the host plan of vdb_ivf_search_prepared_multi (multi_filter.cpp): the
// order in which a mixed batch's queries are scanned. Host only, no HIP headers: compiles with
// plain g++ (tests/cpp/multi_filter_plan_test.cpp).
//
// Query i of the call names its filter, filter_of[i]. The queries are scanned in the stable
// order by filter index, so the queries S_f of filter f are one contiguous run in call order.
// The reference's stale-slot reuse looks back over "the earlier queries of the call"; here that
// reads "the earlier queries of the same filter", and in the scanned order those are the
// queries right in front of a query, back to the start of its run. One carry of [P][k] per call
// then crosses the batches: it belongs to the filter of the latest batch's last query.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace vdbe {

struct MultiFilterPlan {
    std::vector<uint32_t> perm;  // perm[j]: the call's query scanned at position j
    std::vector<uint32_t> pos;   // pos[i]: the position query i is scanned at (perm's inverse)
    std::vector<uint32_t> qf;    // qf[j] = filter_of[perm[j]], ascending
};

// A counting sort by filter index; every filter_of[i] < n_filters (the caller has checked).
inline MultiFilterPlan multi_filter_plan(const uint32_t* filter_of, uint32_t n, uint32_t n_filters) {
    MultiFilterPlan pl;
    pl.perm.resize(n);
    pl.pos.resize(n);
    pl.qf.resize(n);
    std::vector<uint32_t> start((std::size_t)n_filters + 1, 0);
    for (uint32_t i = 0; i < n; ++i) ++start[filter_of[i] + 1];
    for (uint32_t f = 0; f < n_filters; ++f) start[f + 1] += start[f];
    for (uint32_t i = 0; i < n; ++i) {  // (ascending i: stable)
        const uint32_t j = start[filter_of[i]]++;
        pl.perm[j] = i;
        pl.pos[i] = j;
        pl.qf[j] = filter_of[i];
    }
    return pl;
}

// The first position of the run of position q's filter inside the batch that begins at b0
// (b0 <= q): the stale walk-back of q stays in [multi_run_begin, q).
inline uint32_t multi_run_begin(const uint32_t* qf, uint32_t b0, uint32_t q) {
    uint32_t r = q;
    while (r > b0 && qf[r - 1] == qf[q]) --r;
    return r;
}

// Whether the call's carry may serve position q of the batch [b0, ...): the run reaches back to
// the batch's first query and the carry belongs to the same filter. carry_f is the filter of the
// previous batch's last query (kNoCarry before the first batch).
constexpr uint32_t kNoCarry = 0xFFFFFFFFu;
inline bool multi_carry_serves(const uint32_t* qf, uint32_t b0, uint32_t q, uint32_t carry_f) {
    return multi_run_begin(qf, b0, q) == b0 && carry_f == qf[q];
}

}  // namespace vdbe
