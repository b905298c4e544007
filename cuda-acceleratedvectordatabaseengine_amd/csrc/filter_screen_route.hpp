// filter_screen_route.hpp — the routing and sizing of vdb_ivf_search_prepared_screened
// (filter_screen.cpp): whether a call's batches go through the screen, how many candidates a
// batch's bound may collect, and when a batch falls back to the masked exact scan. Host only, no
// HIP headers: compiles with plain g++ (tests/cpp/filter_screen_route_test.cpp).
//
// Through the screen: per batch the pairs kernel the screened search uses (launch_screen_pairs),
// the threshold kernel (per pair the k-th smallest upper bound of its list's allowed rows), the
// bound kernel (every allowed (pair, row)'s lower bound against that threshold) and the exact
// top-k of the rows it could not discard, read from screen_rows. The call never builds,
// refreshes or releases a screen: it uses the one the handle holds at that moment or none.
#pragma once

#include <cstdint>

namespace vdbe {

// Pairs of an item of the two shadow kernels: one MFMA A operand (16 rows).
constexpr uint32_t kFilterScreenGroup = 16;
// reserve == 0: a batch's candidate buffer holds this many times the entries the batch's pairs
// may return (B * P * k): a bound that keeps more than a few times what the top-k can use is
// not pruning, and the masked exact scan serves such a batch at its own, known cost.
constexpr uint64_t kFilterCandPerSlot = 4;
// ... and never more than this many entries (2 GiB), whatever `reserve` asks for.
constexpr uint64_t kFilterCandMax = 1ull << 28;

// What the routing reads of the handle.
struct FilterScreenFacts {
    bool screen_ready = false;  // the handle holds a screen ...
    bool screen_stale = false;  // ... that an add / remove / upsert / new centroids outdated
    bool buffers = false;       // screen_rows, screen_sh, screen_meta and, for int8, screen_scale are present
    int metric = 0;             // the configured metric: 0 L2, 1 InnerProduct, 2 Cosine, 3 CosineDistance
    uint32_t dp = 0;            // the padded dimension
    bool i8 = false;            // the shadow the handle holds is int8 (k-steps of 64 dims), else bf16 (32)
    uint64_t slots = 0;         // 64 x the arena's blocks: a candidate names its slot in 32 bits
};

// True if the call's batches are served through the screen; otherwise the whole call is
// vdb_ivf_search_prepared's path, unchanged. Only a live screen serves (the call builds none);
// Cosine (2) has no screen; the padded dimension is a whole number of k-steps (then a row is
// also whole 128-byte runs for the select kernel); a candidate names its slot in 32 bits.
inline bool filter_screen_serves(const FilterScreenFacts& f) {
    if (!f.screen_ready || f.screen_stale || !f.buffers) return false;
    if (f.metric != 0 && f.metric != 1 && f.metric != 3) return false;
    if (f.dp == 0 || f.dp % (f.i8 ? 64u : 32u) != 0) return false;
    return f.slots > 0 && f.slots < (1ull << 32);
}

// Entries of the candidate buffer of a call whose batches hold at most B queries.
inline uint64_t filter_cand_cap(uint64_t reserve, uint32_t B, uint32_t P, uint32_t k) {
    uint64_t c = reserve;
    if (c == 0) {
        const uint64_t slots = (uint64_t)B * P * k;  // < 2^32 * 2^6
        c = slots > kFilterCandMax / kFilterCandPerSlot ? kFilterCandMax : slots * kFilterCandPerSlot;
    }
    return c < kFilterCandMax ? c : kFilterCandMax;
}

// A batch whose bound kept `candidates` pairs is served by the masked exact scan instead (the
// bound kernel wrote nothing past the buffer and kept counting).
inline bool filter_falls_back(uint64_t candidates, uint64_t cand_cap) { return candidates > cand_cap; }

}  // namespace vdbe
