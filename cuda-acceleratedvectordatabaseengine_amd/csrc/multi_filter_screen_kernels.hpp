// multi_filter_screen_kernels.hpp — launchers of the two shadow kernels behind
// vdb_ivf_search_prepared_multi_screened (multi_filter_screen_kernels.hip, gfx950, wave64): the
// threshold and the bound of filter_screen_kernels.hpp with the mask belonging to the pair's
// query, not to the call. The select is launch_filter_screen_select with FilterSelectArgs::gate.
#pragma once

#include "filter_screen_kernels.hpp"

namespace vdbk {

// FilterScreenArgs with the items of launch_scan_group_pairs (group kFilterScreenGroup, gate =
// launch_pair_gate's); allow and allowed stay null.
struct MultiFilterScreenArgs : FilterScreenArgs {
    const unsigned long long* const* allow_tab = nullptr;  // per filter its masks, per arena block
    const uint32_t* qf = nullptr;                          // the batch's queries' filters [B]
    const uint32_t* gate = nullptr;                        // [B * P]: launch_pair_gate's
};

// tau[pair] = the k-th smallest upper bound over the rows of the pair's list that the pair's own
// filter allows (launch_filter_screen_thresh's value for that filter and pair), for every pair
// with gate != 0; the tau of a pair with gate == 0 is not written. A block is read where the
// mask of any of the item's pairs has a bit; a slot counts for a pair only where that pair's own
// mask has its bit. Reads the shadow and the mask words of the item's own blocks only.
void launch_filter_screen_thresh_multi(int metric, const MultiFilterScreenArgs& a, hipStream_t s);

// Every (pair, slot) with the slot below the list's count, the bit of the pair's own mask set
// and !(lb > tau[pair]) is appended at ctrl[kFsCursor], as launch_filter_screen_bound appends.
// ctrl[kFsPairs] grows by the sum of gate over the items' pairs. The same reads as the threshold
// kernel.
void launch_filter_screen_bound_multi(int metric, const MultiFilterScreenArgs& a, hipStream_t s);

}  // namespace vdbk
