// scan_items.hpp — the work items of the exact scans beside the engine (filter_kernels.hip,
// range_kernels.hip): which blocks of which list, against which of the batch's (query, probe)
// pairs, a workgroup reads. Host and device, no HIP headers: compiles with plain g++
// (tests/cpp/scan_items_test.cpp plays the grouping on the host and decodes every item).
//
// The pairs are grouped by probed list (scan_items.hip): inv[pair_start[l] .. pair_start[l + 1])
// are the pairs of list l. A list of nb blocks is cut into scan_segs(nb, cap) segments and its
// pairs into groups of G; an item is one segment against one group, the segments of a group
// numbered first. item_start[l] is the first item of list l, item_start[nlist] their number.
// The promise that no kernel reads a block it was not given rests on decode_scan_item.
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define VDB_SCAN_HD __host__ __device__ inline
#else
#define VDB_SCAN_HD inline
#endif

namespace vdbk {

constexpr uint32_t kScanSegBlocks = 16;  // a list longer than this many blocks is cut into segments ...
constexpr uint32_t kScanMaxSegs = 16;    // ... at most this many

// Segments a list of nb blocks is cut into, under the call's cap (the segments of its longest list).
VDB_SCAN_HD uint32_t scan_segs(uint32_t nb, uint32_t cap) {
    const uint32_t s = (nb + kScanSegBlocks - 1) / kScanSegBlocks;
    return s < 1 ? 1 : (s > cap ? cap : s);
}

// Items of a list of nb blocks that `pairs` of the batch's pairs probe, in groups of `group`.
VDB_SCAN_HD uint32_t scan_items_of(uint32_t pairs, uint32_t group, uint32_t nb, uint32_t cap) {
    return (pairs + group - 1) / group * scan_segs(nb, cap);
}

struct ExactScanItem {
    uint32_t list, seg;   // segment `seg` of list `list` ...
    uint32_t p0, np;      // ... against the pairs inv[p0 .. p0 + np), 1 <= np <= G
    uint32_t b_lo, b_hi;  // the segment's blocks of the list, b_lo < b_hi <= cdiv(count[list], 64)
};

// Item `item` < item_start[nlist] of a grouping by G under the segment cap `cap`.
template <uint32_t G>
VDB_SCAN_HD ExactScanItem decode_scan_item(uint32_t item, const uint32_t* item_start, const uint32_t* pair_start,
                                           const uint32_t* count, uint32_t nlist, uint32_t cap) {
    uint32_t lo = 0, hi = nlist;  // the first list whose items end beyond `item`
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (item_start[mid + 1] > item) hi = mid;
        else lo = mid + 1;
    }
    ExactScanItem it;
    it.list = lo;
    const uint32_t r = item - item_start[lo];
    const uint32_t nb = (count[lo] + 63) >> 6;
    const uint32_t segs_l = scan_segs(nb, cap);
    it.seg = r % segs_l;
    it.p0 = pair_start[lo] + r / segs_l * G;
    const uint32_t left = pair_start[lo + 1] - it.p0;
    it.np = left < G ? left : G;
    const uint32_t per = (nb + segs_l - 1) / segs_l;
    const uint32_t b_lo = it.seg * per;
    it.b_lo = b_lo < nb ? b_lo : nb;
    it.b_hi = it.b_lo + per < nb ? it.b_lo + per : nb;
    return it;
}

// Host: a call's segment cap, the segments of the longest list the handle stores.
inline uint32_t scan_seg_cap(const uint64_t* count, const uint8_t* owned, uint32_t nlist) {
    uint64_t longest = 0;
    for (uint32_t l = 0; l < nlist; ++l)
        if (owned[l] && (count[l] + 63) / 64 > longest) longest = (count[l] + 63) / 64;
    return scan_segs((uint32_t)longest, kScanMaxSegs);
}

}  // namespace vdbk
