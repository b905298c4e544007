// range_screen_kernels.hpp — launchers of the two kernels behind vdb_ivf_range_search_screened
// (range_screen_kernels.hip, gfx950, wave64): the screen's lower bounds against a fixed radius,
// and the exact re-check of the pairs the bound could not discard.
#pragma once

#include "range_kernels.hpp"

namespace vdbk {

constexpr uint32_t kRangeScreenGroup = 16;  // queries of an item: one MFMA A operand

// The device words the bound kernel reports through (cleared by the caller before the launch).
enum { kRsCursor = 0, kRsStatus = 1, kRsPairs = 2, kRsNext = 3, kRsCtrlWords = 4 };  // (kRsNext: its item counter)

struct RangeScreenArgs {
    // the handle's screen (ivf_screen_build / ivf_screen_build_i8), addressed by arena block
    const uint4* shadow = nullptr;   // per block dp / 32 (bf16) or dp / 64 (int8) k-steps x 4 vector tiles x 64 lanes
    const float4* meta = nullptr;    // per slot {|b|^2, |b| up, |b - b'| up, |x| up}
    const float* sscale = nullptr;   // int8: per slot s_b; null: the bf16 shadow
    // the batch's pairs (launch_screen_pairs), addressed by pair q * P + p
    const void* qres = nullptr;      // the A rows [B * P][dp], bf16 or int8
    const float4* pst = nullptr;
    const float* qscale = nullptr;   // int8: per pair s_a
    // the lists and the items (launch_scan_group with a group of kRangeScreenGroup)
    const uint64_t* block_off = nullptr;
    const uint32_t* count = nullptr;
    const uint32_t* inv = nullptr;
    const uint32_t* pair_start = nullptr;
    const uint32_t* item_start = nullptr;
    uint32_t nlist = 0, B = 0, P = 0, dp = 0;
    uint32_t segs = 1;
    float radius = 0.0f;
    // a prepared filter's masks, or null
    const unsigned long long* allow = nullptr;  // per arena block: bit i = slot i is allowed
    const uint32_t* allowed = nullptr;          // per list: its allowed rows
    uint2* cand = nullptr;                      // out: {batch query, arena slot}
    uint64_t cand_cap = 0;
    unsigned long long* ctrl = nullptr;  // [kRsCtrlWords]
};
// True if the bound kernel serves this shape: whole k-steps per row. The kernel checks the same
// and sets kRangeUnserved in ctrl[kRsStatus].
inline bool range_screen_serves_shape(const RangeScreenArgs& a) {
    return a.dp > 0 && a.dp % (a.sscale ? 64u : 32u) == 0;
}

// metric: kL2 or kIP. Persistent workgroups of 4 waves over the items: one segment of one list
// against up to 16 of the pairs that probe it. Every (pair, slot) with the slot below the list's
// count (and, with masks, its allow bit set) whose lower bound lb satisfies !(lb > radius) is
// appended at ctrl[kRsCursor] as {query, slot} (one atomic per wave and block); past cand_cap
// nothing is written and the cursor keeps counting. ctrl[kRsPairs] grows by the pairs judged
// (with masks: of allowed rows). lb is the screened search's own: the operations of its collect
// kernel's epilogue in their order. Reads the shadow of the item's own blocks only.
void launch_range_screen(int metric, const RangeScreenArgs& a, hipStream_t s);

struct RangeRecheckArgs {
    const uint2* cand = nullptr;  // launch_range_screen's, n of them
    uint64_t n = 0;
    const float4* rows = nullptr;  // the row-major fp32 copy [slot][d4]
    const uint64_t* ids = nullptr;
    const float* q = nullptr;  // the batch's padded queries [B][d4 * 4]
    uint32_t d4 = 0;
    float radius = 0.0f;
    uint64_t cap = 0;  // entries hit_key / hit_id hold
    uint64_t* hit_key = nullptr;
    uint64_t* hit_id = nullptr;
    unsigned long long* ctrl = nullptr;  // [kRangeCtrlWords]: kRangeCursor and kRangeStatus as the range scan uses them
};
// True if the re-check serves this shape (its LDS tile: whole chunks of kRangeChunk4 float4 per row).
inline bool range_recheck_serves(const RangeRecheckArgs& a) { return a.d4 > 0 && a.d4 % kRangeChunk4 == 0; }

// The exact distance (the reference's sequential fp32 sum) of every candidate; d <= radius is
// appended at ctrl[kRangeCursor] exactly as ivf_range_scan appends a hit, the id read for hit
// lanes only.
void launch_range_recheck(int metric, const RangeRecheckArgs& a, hipStream_t s);

}  // namespace vdbk
