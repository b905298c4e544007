// CPU unit test of the screened prepared search's routing and sizing
// (csrc/filter_screen_route.hpp): the predicate that sends a call through the screen, the
// candidate capacity from `reserve` and the batch's shape, and the fallback rule at the capacity
// and one past it. Every expected value is a literal worked out by hand from the rules the
// header states. Exit status 0 = every check passed. Built and run by
// tests/test_filter_screen_abi.py with g++ (no GPU).
#include <cstdio>

#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/filter_screen_route.hpp"

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
static FilterScreenFacts live() {
    FilterScreenFacts f;
    f.screen_ready = true;
    f.buffers = true;
    f.dp = 768;
    f.i8 = true;
    f.slots = 16384ull * 64;
    return f;
}

int main() {
    CHECK_EQ(filter_screen_serves(live()), 1);
    CHECK_EQ(filter_screen_serves(FilterScreenFacts{}), 0);
    // the three flags and the metrics: served only with a ready, fresh screen whose buffers are
    // there and a metric the screen exists for (L2 0, InnerProduct 1, CosineDistance 3)
    for (int bits = 0; bits < 8; ++bits)
        for (int metric = -1; metric < 5; ++metric) {
            FilterScreenFacts f = live();
            f.screen_ready = bits & 1;
            f.screen_stale = bits & 2;
            f.buffers = bits & 4;
            f.metric = metric;
            CHECK_EQ(filter_screen_serves(f), bits == 5 && (metric == 0 || metric == 1 || metric == 3));
        }
    // whole k-steps (64 dims int8, 32 bf16); fewer than 2^32 slots
    FilterScreenFacts f = live();
    f.dp = 0;
    CHECK_EQ(filter_screen_serves(f), 0);
    f.dp = 96;
    CHECK_EQ(filter_screen_serves(f), 0);
    f.i8 = false;
    CHECK_EQ(filter_screen_serves(f), 1);
    f.dp = 80;
    CHECK_EQ(filter_screen_serves(f), 0);
    f = live();
    f.slots = 0;
    CHECK_EQ(filter_screen_serves(f), 0);
    f.slots = (1ull << 32) - 64;
    CHECK_EQ(filter_screen_serves(f), 1);
    f.slots = 1ull << 32;
    CHECK_EQ(filter_screen_serves(f), 0);
    // the capacity: reserve 0 is 4 B P k, never more than 2^28, whatever reserve asks for
    CHECK_EQ(kFilterScreenGroup, 16);
    CHECK_EQ(filter_cand_cap(0, 64, 16, 10), 40960);
    CHECK_EQ(filter_cand_cap(0, 1, 1, 1), 4);
    CHECK_EQ(filter_cand_cap(1, 64, 16, 10), 1);
    CHECK_EQ(filter_cand_cap(0, 1u << 20, 1, 64), 268435456ll);        // 4 * 2^26 = 2^28 exactly
    CHECK_EQ(filter_cand_cap(0, (1u << 20) - 1, 1, 64), 268435200ll);  // 2^28 - 256
    CHECK_EQ(filter_cand_cap(0, 0xFFFFFFFFu, 1024, 64), 268435456ll);  // (no overflow of the product)
    CHECK_EQ(filter_cand_cap(~0ull, 64, 16, 10), 268435456ll);
    CHECK_EQ(filter_cand_cap((1ull << 28) + 1, 1, 1, 1), 268435456ll);
    // the fallback: at the capacity every candidate was written
    CHECK_EQ(filter_falls_back(0, 0), 0);
    CHECK_EQ(filter_falls_back(1, 0), 1);
    CHECK_EQ(filter_falls_back(40960, filter_cand_cap(0, 64, 16, 10)), 0);
    CHECK_EQ(filter_falls_back(40961, filter_cand_cap(0, 64, 16, 10)), 1);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
