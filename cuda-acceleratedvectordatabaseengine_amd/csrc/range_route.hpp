// range_route.hpp — the routing and sizing of vdb_ivf_range_search_screened (range.cpp): whether
// a call's batches go through the screen, how many candidates a batch's bound may collect, and
// when a batch falls back to the exact scan. Host only, no HIP headers: compiles with plain g++
// (tests/cpp/range_route_test.cpp).
//
// Through the screen: per batch the pairs kernel the screened search uses (launch_screen_pairs),
// the bound kernel (ivf_range_screen: every (query, row) pair's lower bound against the radius,
// from the shadow) and the exact re-check of the pairs it could not discard (ivf_range_recheck,
// from screen_rows). The call never builds, refreshes or releases a screen: it uses the one the
// handle holds at that moment or none.
#pragma once

#include <cstdint>

namespace vdbe {

// Queries of an item of the bound kernel: one MFMA A operand (16 rows).
constexpr uint32_t kRangeScreenGroup = 16;
// A batch's candidate buffer holds this many times the entries of its hit buffer (8 bytes each,
// beside the hit buffer's 56): a bound that keeps more than a few times the hits it may return
// is not pruning, and the exact scan serves such a batch at its own, known cost.
constexpr uint64_t kRangeCandPerHit = 4;
// ... and never more than this many entries (2 GiB), whatever `reserve` asks for.
constexpr uint64_t kRangeCandMax = 1ull << 28;
constexpr uint64_t kRangeHitMax = (1ull << 31) - 1;  // a batch's hit buffer (range.cpp)

// What the routing reads of the handle and the call.
struct RangeScreenFacts {
    bool asked = false;         // the caller chose the screened route
    bool screen_ready = false;  // the handle holds a screen ...
    bool screen_stale = false;  // ... that an add / remove / upsert / new centroids outdated
    bool rows = false;          // screen_rows is present (the re-check reads it)
    int metric = 0;             // the configured metric: 0 L2, 1 InnerProduct, 2 Cosine, 3 CosineDistance
    uint32_t dp = 0;            // the padded dimension
    bool i8 = false;            // the shadow the handle holds is int8 (k-steps of 64 dims), else bf16 (32)
    uint64_t slots = 0;         // 64 x the arena's blocks: a candidate names its slot in 32 bits
};

// True if the call's batches are served through the screen; otherwise the whole call is the
// exact path, unchanged. Only a live screen serves (the call builds none); Cosine (2) has no
// screen; the two shape conditions hold for every handle the screened search serves (dp is a
// multiple of 64, an arena has fewer than 2^32 slots) and are checked so that the kernels
// never see another shape.
inline bool range_screen_serves(const RangeScreenFacts& f) {
    if (!f.asked || !f.screen_ready || f.screen_stale || !f.rows) return false;
    if (f.metric != 0 && f.metric != 1 && f.metric != 3) return false;
    if (f.dp == 0 || f.dp % (f.i8 ? 64u : 32u) != 0) return false;
    return f.slots > 0 && f.slots <= (1ull << 32);
}

// Entries of the hit buffer a batch starts with (reserve == 0: auto_reserve).
inline uint64_t range_hit_cap(uint64_t reserve, uint64_t auto_reserve) {
    const uint64_t r = reserve ? reserve : auto_reserve;
    return r < kRangeHitMax ? r : kRangeHitMax;
}

// Entries of the candidate buffer beside a hit buffer of hit_cap entries.
inline uint64_t range_cand_cap(uint64_t hit_cap) {
    const uint64_t c = hit_cap > kRangeCandMax / kRangeCandPerHit ? kRangeCandMax : hit_cap * kRangeCandPerHit;
    return c < kRangeCandMax ? c : kRangeCandMax;
}

// A batch whose bound kept `candidates` pairs is served by the exact scan instead (the bound
// kernel wrote nothing past the buffer and kept counting).
inline bool range_falls_back(uint64_t candidates, uint64_t cand_cap) { return candidates > cand_cap; }

}  // namespace vdbe
