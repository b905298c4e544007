// filter_screen_kernels.hpp — launchers of the kernels behind vdb_ivf_search_prepared_screened
// (filter_screen_kernels.hip, gfx950, wave64): per (query, probe) pair the k-th smallest upper
// bound of its list's allowed rows, the rows whose lower bound does not exceed it, and the exact
// top-k of those rows.
#pragma once

#include "range_kernels.hpp"

namespace vdbk {

constexpr uint32_t kFilterScreenGroup = 16;  // pairs of an item: one MFMA A operand
constexpr uint32_t kFilterScreenMaxK = 64;   // one top-k register per lane

// The device words the kernels report through (cleared by the caller before the first launch).
enum {
    kFsCursor = 0,  // candidates the bound kernel kept (it keeps counting past the capacity)
    kFsStatus = 1,  // kRangeUnserved: a device guard refused the launch's shape
    kFsPairs = 2,   // (pair, allowed row) pairs the bound kernel judged
    kFsNextT = 3,   // the threshold kernel's item counter
    kFsNextB = 4,   // the bound kernel's item counter
    kFsCtrlWords = 5
};

struct FilterScreenArgs {
    // the handle's screen (ivf_screen_build / ivf_screen_build_i8), addressed by arena block
    const uint4* shadow = nullptr;
    const float4* meta = nullptr;
    const float* sscale = nullptr;  // int8: per slot s_b; null: the bf16 shadow
    // the batch's pairs (launch_screen_pairs), addressed by pair q * P + p
    const void* qres = nullptr;
    const float4* pst = nullptr;
    const float* qscale = nullptr;
    // the lists and the items (launch_scan_group with a group of kFilterScreenGroup, gated by allowed[])
    const uint64_t* block_off = nullptr;
    const uint32_t* count = nullptr;
    const uint32_t* inv = nullptr;
    const uint32_t* pair_start = nullptr;
    const uint32_t* item_start = nullptr;
    const uint32_t* probes = nullptr;  // [B * P]: the pairs' lists (the segments' fold reads them)
    uint32_t nlist = 0, B = 0, P = 0, dp = 0;
    uint32_t segs = 1;
    uint32_t k = 0;
    // the prepared filter's masks
    const unsigned long long* allow = nullptr;  // per arena block: bit i = slot i is allowed
    const uint32_t* allowed = nullptr;          // per list: its allowed rows
    // the threshold: part [B * P][segs][k] (segs > 1: per segment its k smallest upper bounds,
    // ascending), tau [B * P]
    float* part = nullptr;
    float* tau = nullptr;
    // the candidates: (pair << 32) | arena slot
    uint64_t* cand = nullptr;
    uint64_t cand_cap = 0;
    unsigned long long* ctrl = nullptr;  // [kFsCtrlWords]
};
// True if the two shadow kernels serve this shape: whole k-steps per row, 1 <= k <= 64. The
// kernels check the same and set kRangeUnserved in ctrl[kFsStatus].
inline bool filter_screen_serves_shape(const FilterScreenArgs& a) {
    return a.dp > 0 && a.dp % (a.sscale ? 64u : 32u) == 0 && a.k >= 1 && a.k <= kFilterScreenMaxK;
}

// metric: kL2 or kIP. tau[pair] = the k-th smallest upper bound ub = approx + del over the
// allowed rows of the pair's list (a NaN ub never counts; +inf if fewer than k count), for every
// pair of the grouping; a pair whose list has no allowed row has no item and its tau is not
// written. approx and del are the screened search's own. Reads the shadow of the item's own
// blocks only, and of no block whose mask is zero.
void launch_filter_screen_thresh(int metric, const FilterScreenArgs& a, hipStream_t s);

// Every (pair, slot) with the slot below the list's count, its allow bit set and
// !(lb > tau[pair]), lb = approx - del, is appended at ctrl[kFsCursor] (one atomic per wave and
// block); past cand_cap nothing is written and the cursor keeps counting. ctrl[kFsPairs] grows
// by the pairs judged. The same reads as the threshold kernel.
void launch_filter_screen_bound(int metric, const FilterScreenArgs& a, hipStream_t s);

struct FilterSelectArgs {
    const uint64_t* cand = nullptr;  // the candidates ascending, n of them
    uint64_t n = 0;
    const float4* rows = nullptr;  // the row-major fp32 copy [slot][d4]
    const uint64_t* ids = nullptr;
    const float* q = nullptr;  // the batch's padded queries [B][d4 * 4]
    const uint32_t* probes = nullptr;   // [B * P]
    const uint32_t* allowed = nullptr;  // per list
    uint32_t BP = 0, P = 0, d4 = 0, k = 0;
    float* slot_d = nullptr;  // [B * P][k]
    uint64_t* slot_i = nullptr;
    unsigned long long* ctrl = nullptr;  // [kFsCtrlWords]
    // per-query filters: [BP], gate[pair] == 0 for "nothing to do for this pair"; null: allowed[probes[pair]] == 0
    const uint32_t* gate = nullptr;
};
// True if the select kernel serves this shape (its LDS tile: whole chunks of kRangeChunk4 float4 per row).
inline bool filter_select_serves(const FilterSelectArgs& a) {
    return a.d4 > 0 && a.d4 % kRangeChunk4 == 0 && a.k >= 1 && a.k <= kFilterScreenMaxK;
}

// Per pair whose list has an allowed row: the k smallest (distance, id) among its candidates,
// the distance the reference's sequential fp32 sum, ascending, unfilled entries (+inf,
// UINT64_MAX): what launch_filter_scan (+ launch_filter_fold) leave in slot_d / slot_i. Nothing
// is written for a pair whose list has no allowed row.
void launch_filter_screen_select(int metric, const FilterSelectArgs& a, hipStream_t s);

}  // namespace vdbk
