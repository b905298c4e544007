// range_kernels.hpp — launchers of the kernels behind vdb_ivf_range_search
// (range_kernels.hip, gfx950, wave64).
#pragma once

#include "scan_kernels.hpp"

namespace vdbk {

constexpr uint32_t kRangeGroup = 8;   // queries that probe the same list share one read of it
constexpr uint32_t kRangeChunk4 = 8;  // row-major layout: float4 of a row staged through LDS per step

// The device words a scan reports through (cleared by the caller before every scan).
enum { kRangeCursor = 0, kRangeStatus = 1, kRangePairs = 2, kRangeNext = 3, kRangeCtrlWords = 4 };  // (kRangeNext: the scan's item counter)
constexpr unsigned long long kRangeUnserved = 1;  // status bit: a device guard refused the launch's shape

struct RangeScanArgs : ScanListArgs {
    float radius = 0.0f;
    uint64_t cap = 0;             // entries hit_key / hit_id hold
    uint64_t* hit_key = nullptr;  // (batch query << 32) | ord_enc(distance)
    uint64_t* hit_id = nullptr;
    unsigned long long* ctrl = nullptr;  // [kRangeCtrlWords]
};
// True if the scan kernel serves this shape (its fixed-size LDS tile: whole chunks of
// kRangeChunk4 float4 per row). The kernel checks the same and sets kRangeUnserved.
inline bool range_scan_serves(const RangeScanArgs& a) { return a.d4 > 0 && a.d4 % kRangeChunk4 == 0; }

// Persistent workgroups over the items of launch_scan_group (group kRangeGroup, gate = the
// lists' counts): one segment of one list against up to kRangeGroup of the queries that probe it. Every slot below its block's valid count
// whose exact distance d satisfies d <= radius is appended at ctrl[kRangeCursor] (one atomic
// per wave and query); past `cap` nothing is written and the cursor keeps counting.
// ctrl[kRangePairs] grows by the (query, row) distances computed.
void launch_range_scan(int metric, const RangeScanArgs& a, hipStream_t s);

// The same scan over the rows a filter allows (vdb_ivf_range_search_prepared). The unmasked
// kernels keep their own argument block, so nothing of them changes.
struct RangeMaskedScanArgs : RangeScanArgs {
    const unsigned long long* allow = nullptr;  // per arena block: bit i = slot i is allowed (none at or above the block's valid count)
    const uint32_t* allowed = nullptr;          // per list: its allowed rows (the popcounts of its blocks)
};
// Items of launch_scan_group with gate = `allowed`, so a list without an allowed row has none.
// A block whose mask is zero is skipped before any row byte is loaded; in the row-major layout
// only allowed rows are loaded. A hit is a slot below the valid count whose bit is set and
// whose d <= radius. ctrl[kRangePairs] grows by the distances of allowed rows only.
void launch_range_scan_masked(int metric, const RangeMaskedScanArgs& a, hipStream_t s);

// The buffers that order m appended hits (each of at least m entries).
struct RangeOrderBufs {
    uint64_t* key_a = nullptr;  // in: the scan's hit_key
    uint64_t* id_a = nullptr;   // in: the scan's hit_id
    uint64_t* key_b = nullptr;  // out: the ordered ids
    uint64_t* id_b = nullptr;
    uint32_t* perm_a = nullptr;  // out: the ordered distances (as float)
    uint32_t* perm_b = nullptr;
    void* temp = nullptr;
    size_t temp_bytes = 0;
    uint32_t* start = nullptr;  // out [B + 1]: query i of the batch owns [start[i], start[i + 1])
};
// Bytes of `temp` launch_range_order needs for m hits of a batch of B queries.
hipError_t range_order_temp_bytes(uint64_t m, uint32_t B, size_t& bytes);
// m >= 1 hits in arbitrary order into per query ascending (distance, id) (-0.0f ties +0.0f),
// an id stored more than once for a query kept once at its smallest distance. start[B] is the
// number of entries left.
hipError_t launch_range_order(const RangeOrderBufs& b, uint64_t m, uint32_t B, hipStream_t s);

}  // namespace vdbk
