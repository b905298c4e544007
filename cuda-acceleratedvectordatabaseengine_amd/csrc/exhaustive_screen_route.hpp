// exhaustive_screen_route.hpp — the routing and sizing of vdb_ivf_search_exhaustive_screened
// (exhaustive_screen.cpp): whether a call goes through the screen, how many queries a tile holds,
// how many candidates a query's bound may collect, and when a tile falls back to the exact
// exhaustive scan. Host only, no HIP headers: compiles with plain g++
// (tests/cpp/exhaustive_screen_route_test.cpp).
//
// Through the screen: per tile the pairs kernel the screened search uses (launch_screen_pairs, an
// identity probe table: every (query, list) is a pair), the threshold kernel (per query the k-th
// smallest upper bound over distinct ids of every stored row), the bound kernel (every stored
// row's lower bound against that threshold) and the exact unique top-k of the rows it could not
// discard, read from screen_rows. The call never builds, refreshes or releases a screen: it uses
// the one the handle holds at that moment or none.
#pragma once

#include <cstdint>

namespace vdbe {

// Queries of a tile: two MFMA A operands of 16 rows; the threshold lists then take
// 4 waves x 32 queries x 64 entries x 12 B = 96 KiB of LDS.
constexpr uint32_t kExhScreenTile = 32;
// One WaveTopK register per threshold list.
constexpr uint32_t kExhScreenMaxK = 64;
// reserve == 0: a query's candidate buffer holds max(kExhCandFloor, kExhCandPerK * k) entries. A
// choice, not a measurement: the survivors of one index-wide threshold are about k plus the rows
// within one bound width of the k-th distance (DESIGN 7o records what was counted).
constexpr uint64_t kExhCandFloor = 4096;
constexpr uint64_t kExhCandPerK = 64;
// ... and never more than this many entries per query (2 GiB per tile), whatever `reserve` asks.
constexpr uint64_t kExhCandMax = 1ull << 24;
// The pairs' A rows of a tile (tile x nlist x dp bytes int8, twice that bf16) stay within this;
// a tile of 32 that would not is halved to 16 (one A operand).
constexpr uint64_t kExhPairsBudget = 1ull << 30;

// What the routing reads of the handle.
struct ExhScreenFacts {
    bool screen_ready = false;  // the handle holds a screen ...
    bool screen_stale = false;  // ... that an add / remove / upsert / new centroids outdated
    bool buffers = false;       // screen_rows, screen_sh, screen_meta, screen_blist and, for int8, screen_scale
    int metric = 0;             // the configured metric: 0 L2, 1 InnerProduct, 2 Cosine, 3 CosineDistance
    uint32_t dp = 0;            // the padded dimension
    bool i8 = false;            // the shadow the handle holds is int8 (k-steps of 64 dims), else bf16 (32)
    uint64_t slots = 0;         // 64 x the arena's blocks: a candidate names its slot in 32 bits
};

// True if the call is served through the screen; otherwise the whole call is
// vdb_ivf_search_exhaustive's path, unchanged.
inline bool exh_screen_serves(const ExhScreenFacts& f, uint32_t k) {
    if (!f.screen_ready || f.screen_stale || !f.buffers) return false;
    if (f.metric != 0 && f.metric != 1 && f.metric != 3) return false;
    if (f.dp == 0 || f.dp % (f.i8 ? 64u : 32u) != 0) return false;
    if (k < 1 || k > kExhScreenMaxK) return false;
    return f.slots > 0 && f.slots < (1ull << 32);
}

// Bytes of a tile's A rows.
inline uint64_t exh_pairs_bytes(uint32_t tile, uint32_t nlist, uint32_t dp, bool i8) {
    return (uint64_t)tile * nlist * dp * (i8 ? 1u : 2u);
}

// Queries per tile.
inline uint32_t exh_screen_tile(uint32_t nlist, uint32_t dp, bool i8) {
    return exh_pairs_bytes(kExhScreenTile, nlist, dp, i8) > kExhPairsBudget ? kExhScreenTile / 2 : kExhScreenTile;
}

// Entries of a query's region of the candidate buffer.
inline uint64_t exh_cand_cap(uint64_t reserve, uint32_t k) {
    uint64_t c = reserve;
    if (c == 0) c = kExhCandPerK * k > kExhCandFloor ? kExhCandPerK * k : kExhCandFloor;
    return c < kExhCandMax ? c : kExhCandMax;
}

// A tile in which a query kept `candidates` rows is served by the exact exhaustive scan instead
// (the bound kernel wrote nothing past the query's region and kept counting).
inline bool exh_falls_back(uint64_t candidates, uint64_t cand_cap) { return candidates > cand_cap; }

}  // namespace vdbe
