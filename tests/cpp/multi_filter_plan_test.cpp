// multi_filter_plan_test.cpp — the host plan of vdb_ivf_search_prepared_multi
// (csrc/multi_filter_plan.hpp), compiled with plain g++: no GPU, no HIP headers.
//
// For filter_of patterns i % 3, all equal, all distinct and descending (and a seeded random
// run): the permutation is a permutation, pos is its inverse, qf is filter_of in scanned order
// and ascending, every filter's queries are one contiguous run in call order (stable). Then the
// carry rule is played on the host under batch cuts of 1, 7 and n: for every query and slot, the
// query whose slot content a stale slot takes (walking back inside the batch over the same
// filter, else the carry if it serves) must be the one the definition names — the latest
// earlier query of the same filter, in call order, with an allowed row at that slot — whatever
// the cut.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/multi_filter_plan.hpp"

using namespace vdbe;

static int failures = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static void check_plan(const std::vector<uint32_t>& fo, uint32_t F) {
    const uint32_t n = (uint32_t)fo.size();
    const MultiFilterPlan pl = multi_filter_plan(fo.data(), n, F);
    CHECK(pl.perm.size() == n && pl.pos.size() == n && pl.qf.size() == n);
    std::vector<int> seen(n, 0);
    for (uint32_t j = 0; j < n; ++j) {
        CHECK(pl.perm[j] < n);
        if (pl.perm[j] >= n) return;
        ++seen[pl.perm[j]];
        CHECK(pl.pos[pl.perm[j]] == j);        // the inverse
        CHECK(pl.qf[j] == fo[pl.perm[j]]);     // the filter in scanned order
        if (j) {
            CHECK(pl.qf[j - 1] <= pl.qf[j]);   // runs contiguous (ascending by filter) ...
            if (pl.qf[j - 1] == pl.qf[j]) CHECK(pl.perm[j - 1] < pl.perm[j]);  // ... and in call order
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        CHECK(seen[i] == 1);
        CHECK(pl.perm[pl.pos[i]] == i);
    }
}

// The carry rule on the host. has[i * P + p]: query i (call order) has an allowed row at slot p.
// Returns per (call query, slot) the call query whose content the slot shows: itself, an earlier
// one of the same filter, or -1 for nothing.
static std::vector<int> play(const std::vector<uint32_t>& fo, uint32_t F, const std::vector<uint8_t>& has, uint32_t P,
                             uint32_t cut) {
    const uint32_t n = (uint32_t)fo.size();
    const MultiFilterPlan pl = multi_filter_plan(fo.data(), n, F);
    std::vector<int> src((size_t)n * P, -1);
    std::vector<int> carry(P, -1);  // the call query whose content the carry holds per slot
    uint32_t carry_f = kNoCarry;
    auto H = [&](uint32_t j, uint32_t p) { return has[(size_t)pl.perm[j] * P + p] != 0; };
    for (uint32_t b0 = 0; b0 < n; b0 += cut) {
        const uint32_t B = cut < n - b0 ? cut : n - b0;
        for (uint32_t j = b0; j < b0 + B; ++j)
            for (uint32_t p = 0; p < P; ++p) {
                int s = -1;
                if (H(j, p)) s = (int)pl.perm[j];
                else {
                    const uint32_t r = multi_run_begin(pl.qf.data(), b0, j);
                    for (uint32_t j2 = j; j2 > r && s < 0;)
                        if (H(--j2, p)) s = (int)pl.perm[j2];
                    if (s < 0 && multi_carry_serves(pl.qf.data(), b0, j, carry_f)) s = carry[p];
                }
                src[(size_t)pl.perm[j] * P + p] = s;
            }
        // the carry after the batch: the run of the batch's last query
        const uint32_t last = b0 + B - 1;
        const uint32_t r = multi_run_begin(pl.qf.data(), b0, last);
        for (uint32_t p = 0; p < P; ++p) {
            int s = -1;
            for (uint32_t j2 = last + 1; j2 > r && s < 0;)
                if (H(--j2, p)) s = (int)pl.perm[j2];
            if (s < 0 && r == b0 && carry_f == pl.qf[last]) s = carry[p];
            carry[p] = s;
        }
        carry_f = pl.qf[last];
    }
    return src;
}

// The definition: the latest query i2 <= i of the same filter, in call order, with has.
static std::vector<int> definition(const std::vector<uint32_t>& fo, const std::vector<uint8_t>& has, uint32_t P) {
    const uint32_t n = (uint32_t)fo.size();
    std::vector<int> src((size_t)n * P, -1);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t p = 0; p < P; ++p)
            for (int i2 = (int)i; i2 >= 0; --i2)
                if (fo[i2] == fo[i] && has[(size_t)i2 * P + p]) {
                    src[(size_t)i * P + p] = i2;
                    break;
                }
    return src;
}

static void check_carry(const std::vector<uint32_t>& fo, uint32_t F, std::mt19937& gen) {
    const uint32_t n = (uint32_t)fo.size(), P = 5;
    if (!n) return;
    std::vector<uint8_t> has((size_t)n * P);
    for (auto& x : has) x = gen() % 4 == 0;  // most slots without an allowed row
    const std::vector<int> want = definition(fo, has, P);
    for (uint32_t cut : {1u, 7u, n}) CHECK(play(fo, F, has, P, cut) == want);
}

int main() {
    std::mt19937 gen(11);
    const uint32_t n = 40;
    std::vector<std::vector<uint32_t>> pats(4, std::vector<uint32_t>(n));
    for (uint32_t i = 0; i < n; ++i) {
        pats[0][i] = i % 3;      // interleaved
        pats[1][i] = 2;          // all equal
        pats[2][i] = i;          // all distinct
        pats[3][i] = n - 1 - i;  // descending
    }
    for (const auto& fo : pats) {
        check_plan(fo, n);
        check_carry(fo, n, gen);
    }
    // hand-derived: filter_of = 2 0 2 1 0 -> scanned 1 4 3 0 2
    {
        const std::vector<uint32_t> fo{2, 0, 2, 1, 0};
        const MultiFilterPlan pl = multi_filter_plan(fo.data(), 5, 3);
        CHECK((pl.perm == std::vector<uint32_t>{1, 4, 3, 0, 2}));
        CHECK((pl.pos == std::vector<uint32_t>{3, 0, 4, 2, 1}));
        CHECK((pl.qf == std::vector<uint32_t>{0, 0, 1, 2, 2}));
        CHECK(multi_run_begin(pl.qf.data(), 0, 1) == 0 && multi_run_begin(pl.qf.data(), 0, 2) == 2);
        CHECK(multi_run_begin(pl.qf.data(), 1, 1) == 1 && multi_run_begin(pl.qf.data(), 0, 4) == 3);
        CHECK(multi_carry_serves(pl.qf.data(), 1, 1, 0) && !multi_carry_serves(pl.qf.data(), 1, 1, kNoCarry));
        CHECK(!multi_carry_serves(pl.qf.data(), 1, 2, 1));  // its run begins behind the batch's first query
        CHECK(!multi_carry_serves(pl.qf.data(), 3, 4, 1) && multi_carry_serves(pl.qf.data(), 3, 4, 2));
    }
    // empty and single
    check_plan({}, 1);
    check_plan({0}, 1);
    int cases = 0;
    for (; cases < 1000; ++cases) {
        const uint32_t m = 1 + gen() % 50, F = 1 + gen() % 9;
        std::vector<uint32_t> fo(m);
        for (auto& x : fo) x = gen() % F;
        check_plan(fo, F);
        check_carry(fo, F, gen);
    }
    std::printf("random run: %d cases\n", cases);
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
