// CPU unit test of the screened exhaustive search's routing and sizing
// (csrc/exhaustive_screen_route.hpp): the predicate that sends a call through the screen at each
// condition's edge, the tile and its halving at the pairs budget, the candidate capacity from
// `reserve` and k, and the fallback rule at the capacity and one past it. Every expected value is
// a literal worked out by hand from the rules the header states. Exit status 0 = every check
// passed. Built and run by tests/test_exhaustive_screen_abi.py with g++ (no GPU).
#include <cstdio>

#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/exhaustive_screen_route.hpp"

using namespace vdbe;

static int failures = 0;
#define CHECK_EQ(a, b)                                                                             \
    do {                                                                                           \
        const long long va = (long long)(a), vb = (long long)(b);                                  \
        if (va != vb) {                                                                            \
            std::printf("FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, va, vb); \
            ++failures;                                                                            \
        }                                                                                          \
    } while (0)

// an L2 handle of 768 dims whose int8 screen is live, 1M rows in 16,384 blocks
static ExhScreenFacts live() {
    ExhScreenFacts f;
    f.screen_ready = true;
    f.buffers = true;
    f.dp = 768;
    f.i8 = true;
    f.slots = 16384ull * 64;
    return f;
}

int main() {
    CHECK_EQ(exh_screen_serves(live(), 10), 1);
    CHECK_EQ(exh_screen_serves(ExhScreenFacts{}, 10), 0);
    // one WaveTopK register per list: k 1 .. 64
    CHECK_EQ(exh_screen_serves(live(), 0), 0);
    CHECK_EQ(exh_screen_serves(live(), 64), 1);
    CHECK_EQ(exh_screen_serves(live(), 65), 0);
    // a ready, fresh (not stale) screen with its buffers, a metric the screen exists for
    for (int bits = 0; bits < 8; ++bits)
        for (int metric = -1; metric < 5; ++metric) {
            ExhScreenFacts f = live();
            f.screen_ready = bits & 1;
            f.screen_stale = bits & 2;
            f.buffers = bits & 4;
            f.metric = metric;
            CHECK_EQ(exh_screen_serves(f, 10), bits == 5 && (metric == 0 || metric == 1 || metric == 3));
        }
    // whole k-steps (64 dims int8, 32 bf16); fewer than 2^32 slots
    ExhScreenFacts f = live();
    f.dp = 0;
    CHECK_EQ(exh_screen_serves(f, 10), 0);
    f.dp = 96;
    CHECK_EQ(exh_screen_serves(f, 10), 0);
    f.i8 = false;
    CHECK_EQ(exh_screen_serves(f, 10), 1);
    f.dp = 80;
    CHECK_EQ(exh_screen_serves(f, 10), 0);
    f = live();
    f.slots = 0;
    CHECK_EQ(exh_screen_serves(f, 10), 0);
    f.slots = (1ull << 32) - 64;
    CHECK_EQ(exh_screen_serves(f, 10), 1);
    f.slots = 1ull << 32;
    CHECK_EQ(exh_screen_serves(f, 10), 0);
    // the tile's A rows: 32 x nlist x dp bytes int8, twice that bf16; above 2^30 the tile is 16
    CHECK_EQ(kExhScreenTile, 32);
    CHECK_EQ(exh_pairs_bytes(32, 4096, 768, true), 100663296ll);
    CHECK_EQ(exh_screen_tile(32768, 1024, true), 32);   // 2^5 2^15 2^10 = 2^30 exactly
    CHECK_EQ(exh_screen_tile(32768, 1024, false), 16);  // 2^31
    CHECK_EQ(exh_screen_tile(32769, 1024, true), 16);
    CHECK_EQ(exh_screen_tile(0xFFFFFFFFu, 4096, false), 16);  // (no overflow of the product)
    // the capacity per query: reserve 0 is max(4096, 64 k), never more than 2^24
    CHECK_EQ(exh_cand_cap(0, 10), 4096);
    CHECK_EQ(exh_cand_cap(0, 64), 4096);
    CHECK_EQ(exh_cand_cap(0, 65), 4160);
    CHECK_EQ(exh_cand_cap(1, 10), 1);
    CHECK_EQ(exh_cand_cap(1 << 17, 10), 131072);
    CHECK_EQ(exh_cand_cap(~0ull, 10), 16777216);
    // the fallback: at the capacity every candidate was written
    CHECK_EQ(exh_falls_back(1, 1), 0);
    CHECK_EQ(exh_falls_back(2, 1), 1);
    CHECK_EQ(exh_falls_back(4096, exh_cand_cap(0, 10)), 0);
    CHECK_EQ(exh_falls_back(4097, exh_cand_cap(0, 10)), 1);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
