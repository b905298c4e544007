// scan_kernels.hpp — what the exact scans beside the engine share on the device: the pair
// grouping (scan_items.hip) and the head of their kernel arguments (gfx950, wave64).
#pragma once

#include <hip/hip_runtime.h>

#include "scan_items.hpp"

namespace vdbk {

// The batch's (query, probe) pairs grouped by probed list, pairs of a list with gate[l] == 0
// left out: inv[pair_start[l] .. pair_start[l + 1]) are the pairs (q * P + p) that probe list l
// (in no particular order: every pair's result is computed on its own). item_start[l] is the
// first scan item of list l, scan_items_of(pairs, group, cdiv(count[l], 64), segs) each;
// item_start[nlist] is their number. cursor is scratch ([nlist]).
void launch_scan_group(const uint32_t* probes, uint32_t BP, const uint32_t* gate, const uint32_t* count,
                       uint32_t nlist, uint32_t segs, uint32_t group, uint32_t* cursor, uint32_t* pair_start,
                       uint32_t* item_start, uint32_t* inv, hipStream_t s);

// The same grouping gated per pair: pair i is left out where gate[i] == 0 (gate has BP entries;
// vdb_ivf_search_prepared_multi passes the rows the pair's own filter allows in its list). The
// outputs mean what they mean above, so decode_scan_item serves both.
void launch_scan_group_pairs(const uint32_t* probes, uint32_t BP, const uint32_t* gate, const uint32_t* count,
                             uint32_t nlist, uint32_t segs, uint32_t group, uint32_t* cursor, uint32_t* pair_start,
                             uint32_t* item_start, uint32_t* inv, hipStream_t s);

// What a scan kernel reads to find its items, their rows and their queries.
struct ScanListArgs {
    const float4* lists = nullptr;  // rows == 0: [block][d4][64] float4; rows != 0: [slot][d4] float4
    const uint64_t* ids = nullptr;  // [block][64]
    const uint64_t* block_off = nullptr;  // per list
    const uint32_t* count = nullptr;      // per list
    const float* q = nullptr;             // the batch's padded queries [B][d4 * 4]
    const uint32_t* inv = nullptr;        // launch_scan_group
    const uint32_t* pair_start = nullptr;
    const uint32_t* item_start = nullptr;
    uint32_t nlist = 0, B = 0, P = 0, d4 = 0;
    uint32_t segs = 1;  // the call's segment cap (1 .. kScanMaxSegs)
    int rows = 0;
};

}  // namespace vdbk
