// remove.hpp — vdb_ivf_remove_ids on one handle (remove.cpp), for the C ABI entry
// (engine.cpp) and the group form (group.cpp).
#pragma once

#include "engine.hpp"

namespace vdbe {

// The calling thread's latest remove_ids, step by step (vdb_remove_last_timing).
struct RemoveTiming {
    double mark_ms = 0.0;     // ivf_remove_mark (HIP events)
    double plan_ms = 0.0;     // the host plan
    double compact_ms = 0.0;  // ivf_remove_compact (HIP events); 0 when nothing was removed
    uint64_t rows_kept = 0;   // rows the compact pass moved
};
extern thread_local RemoveTiming g_remove_timing;

// Caller holds h.mu and has made h's device current. Removes from the lists h stores every
// row whose id is in `sorted` (ascending, each once; remove_sorted_ids) and returns how many
// went; per_list (may be null) receives the count per list. Nothing matched: the handle is
// untouched. Not for sharded handles: the caller refuses those (a group calls it per member).
uint64_t remove_ids(vdb_ivf& h, const std::vector<uint64_t>& sorted, std::vector<uint64_t>* per_list);

// A fresh, cleared list arena of `blocks` blocks for h in the caller's two empty buffers, where
// h's arena lives (HBM, or page-locked host memory in the list-cache tier), as
// vdb_ivf::relayout allocates it: rows zero, ids 0xFF, one slack block past the last list (the
// scan prefetches one chunk and one block of ids beyond the segment it streams). The clears are
// queued on h.stream. h is not touched: the caller swaps the pair in once it is whole
// (remove.cpp, upsert.cpp).
void fresh_arena(vdb_ivf& h, uint64_t blocks, DevBuf<float4>& rows, DevBuf<uint64_t>& ids);

}  // namespace vdbe
