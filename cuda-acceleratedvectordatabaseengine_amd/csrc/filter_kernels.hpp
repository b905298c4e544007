// filter_kernels.hpp — launchers of the kernels behind vdb_ivf_search_filtered
// (filter_kernels.hip, gfx950, wave64).
#pragma once

#include "scan_kernels.hpp"

namespace vdbk {

constexpr uint32_t kFilterMaxK = 64;   // one top-k register per lane (WaveTopK<1>)
constexpr uint32_t kFilterGroup = 4;   // queries that probe the same list share one read of it

// allow[b] bit i = slot i of block b holds a row (i < valid[b]) that the filter lets through:
// include == 0: its id is not one of sorted[0..n); include != 0: it is. sorted is ascending
// (the binary search finds an id that stands more than once just as well). Reads the ids of
// slots below valid[b] only (8 bytes per slot).
void launch_filter_mark(const uint64_t* arena_ids, const uint32_t* valid, uint64_t nblocks, const uint64_t* sorted,
                        uint32_t n, int include, unsigned long long* allow, hipStream_t s);

// allowed[l] = rows of list l the masks let through (the popcounts of its cdiv(count[l], 64)
// blocks from block_off[l] on).
void launch_filter_count(const unsigned long long* allow, const uint64_t* block_off, const uint32_t* count,
                         uint32_t nlist, uint32_t* allowed, hipStream_t s);

struct FilterScanArgs : ScanListArgs {
    uint32_t k = 0;
    const unsigned long long* allow = nullptr;  // per arena block
    float* part_d = nullptr;  // [B * P][segs][k]: per segment the top-k of its allowed rows
    uint64_t* part_i = nullptr;
};
// One workgroup per item of launch_scan_group (group kFilterGroup, gate = the lists' allowed
// rows): one segment of one list against up to kFilterGroup of the queries that probe it. A
// pair whose list has no allowed row gets no item and nothing is written for it.
void launch_filter_scan(int metric, const FilterScanArgs& a, hipStream_t s);

// segs > 1: per pair the top-k of its segments' partials into slot_d / slot_i [B * P][k].
void launch_filter_fold(const float* part_d, const uint64_t* part_i, const uint32_t* probes, const uint32_t* allowed,
                        const uint32_t* count, uint32_t BP, uint32_t segs, uint32_t k, float* slot_d, uint64_t* slot_i,
                        hipStream_t s);

// Per query the unique-id top-k of its P slot lists (merge_results) into out_d / out_i [B][k],
// unfilled entries (FLT_MAX, UINT64_MAX). A slot whose list has no allowed row contributes
// nothing, or with stale != 0 the content of the latest earlier query with an allowed row at
// that slot: in this batch, else the carry ([P][k], ids UINT64_MAX where the call has none yet).
// Then the carry takes, per slot, the batch's latest query with an allowed row.
// pairs (device) grows by the (query, row) distances the batch's scan computed.
void launch_filter_merge(const uint32_t* probes, const uint32_t* allowed, const float* slot_d, const uint64_t* slot_i,
                         float* carry_d, uint64_t* carry_i, uint32_t B, uint32_t P, uint32_t k, int stale,
                         float* out_d, uint64_t* out_i, unsigned long long* pairs, hipStream_t s);

}  // namespace vdbk
