// multi_filter_kernels.hpp — launchers of the kernels behind vdb_ivf_search_prepared_multi
// (multi_filter_kernels.hip, gfx950, wave64): the masked exact scan of filter_kernels.hip with
// the mask belonging to the query, not to the call.
#pragma once

#include "filter_kernels.hpp"

namespace vdbk {

// gate[q * P + p] = allowed_tab[qf[q]][probes[q * P + p]]: the rows query q's own filter
// allows in the list its probe p names.
void launch_pair_gate(const uint32_t* probes, const uint32_t* qf, const uint32_t* const* allowed_tab, uint32_t B,
                      uint32_t P, uint32_t* gate, hipStream_t s);

struct MultiFilterScanArgs : ScanListArgs {
    uint32_t k = 0;
    const unsigned long long* const* allow_tab = nullptr;  // per filter its masks, per arena block
    const uint32_t* qf = nullptr;                          // the batch's queries' filters [B]
    float* part_d = nullptr;  // [B * P][segs][k]: per segment the top-k of the rows the pair's filter allows
    uint64_t* part_i = nullptr;
};
// One workgroup per item of launch_scan_group_pairs (group kFilterGroup, gate = launch_pair_gate's):
// one segment of one list against up to kFilterGroup of the pairs that probe it, each under its
// own query's mask. A block is read where any of the item's masks has a bit, and a row is
// offered to a query only where that query's own mask has its bit. A pair whose filter allows
// no row of its list gets no item and nothing is written for it.
void launch_filter_scan_multi(int metric, const MultiFilterScanArgs& a, hipStream_t s);

// segs > 1: per pair with gate != 0 the top-k of its segments' partials into slot_d / slot_i [B * P][k].
void launch_filter_fold_multi(const float* part_d, const uint64_t* part_i, const uint32_t* probes,
                              const uint32_t* gate, const uint32_t* count, uint32_t BP, uint32_t segs, uint32_t k,
                              float* slot_d, uint64_t* slot_i, hipStream_t s);

// launch_filter_merge with the pair's gate for "the list has an allowed row" and the stale
// reuse kept inside a filter: a slot without an allowed row takes, with stale != 0, the content
// of the latest earlier query of the batch *with the same filter* (qf is ascending, so those
// are the queries right in front) that had one; if that run reaches the batch's first query and
// carry_same != 0 (the carry belongs to the filter of the batch's first query), the carry; else
// nothing. Then the carry takes, per slot, the latest query with an allowed row among the run
// of the batch's last query; without one it keeps its content if that run is the whole batch
// and carry_same != 0, and holds nothing (ids UINT64_MAX) otherwise.
// pairs (device) grows by the sum of gate over the batch's pairs.
void launch_filter_merge_multi(const uint32_t* gate, const uint32_t* qf, const float* slot_d, const uint64_t* slot_i,
                               float* carry_d, uint64_t* carry_i, int carry_same, uint32_t B, uint32_t P, uint32_t k,
                               int stale, float* out_d, uint64_t* out_i, unsigned long long* pairs, hipStream_t s);

}  // namespace vdbk
