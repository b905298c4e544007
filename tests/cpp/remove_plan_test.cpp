// CPU unit test of the host plan behind vdb_ivf_remove_ids (csrc/remove_plan.hpp): from the
// per-block keep masks and the old directory, every list's new count, the new block offsets
// (relayout's packing rule), every old block's destination slot and the removed total; plus
// the sorted, de-duplicated request and the per-block valid-slot counts the mark kernel reads.
// Hand-derived cases, then a seeded random run in which the test plays both kernels on the
// host (mark: id lookup per valid slot; compact: base + kept lanes below) over explicit
// per-list id arrays and compares the compacted arena with a brute-force filter of each list.
// Exit status 0 = every check passed. Built and run by tests/test_remove_plan.py with g++ (no
// GPU), once plain and once with the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/remove_plan.hpp"

using vdbe::remove_plan;
using vdbe::RemovePlan;
using U64 = std::vector<uint64_t>;
using U8 = std::vector<uint8_t>;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static uint64_t cdiv64(uint64_t n) { return (n + 63) / 64; }

// relayout's packing: lists in order, cdiv(count, 64) blocks per stored list
static U64 pack(const U64& count, const U8& owned, uint64_t& blocks) {
    U64 off(count.size(), 0);
    blocks = 0;
    for (size_t l = 0; l < count.size(); ++l) {
        off[l] = blocks;
        if (owned[l]) blocks += cdiv64(count[l]);
    }
    return off;
}

// keep masks of an arena in which list l loses the slots gone[l] (slot = index in the list)
static U64 masks(const U64& count, const U64& off, const U8& owned, uint64_t blocks,
                 const std::vector<std::set<uint64_t>>& gone) {
    U64 keep(blocks, 0);
    for (size_t l = 0; l < count.size(); ++l) {
        if (!owned[l]) continue;
        for (uint64_t s = 0; s < count[l]; ++s)
            if (!gone[l].count(s)) keep[off[l] + s / 64] |= 1ull << (s % 64);
    }
    return keep;
}

static void hand_cases() {
    {  // nothing removed: the plan is the old directory
        const U64 count = {100, 64, 1};
        const U8 owned = {1, 1, 1};
        uint64_t nb;
        const U64 off = pack(count, owned, nb);
        CHECK(nb == 4);
        const RemovePlan p = remove_plan(masks(count, off, owned, nb, {{}, {}, {}}), count, off, owned);
        CHECK(p.removed_total == 0);
        CHECK(p.new_count == count);
        CHECK((p.new_off == U64{0, 2, 3}));
        CHECK(p.new_blocks == 4);
        CHECK((p.base == U64{0, 64, 128, 192}));
        CHECK((p.removed == U64{0, 0, 0}));
        CHECK((vdbe::remove_block_valid(count, off, owned, nb) == std::vector<uint32_t>{64, 36, 64, 1}));
    }
    {  // a whole list removed: it keeps its place in the order with no block
        const U64 count = {100, 70, 5};
        const U8 owned = {1, 1, 1};
        uint64_t nb;
        const U64 off = pack(count, owned, nb);
        CHECK(nb == 5);
        std::set<uint64_t> all;
        for (uint64_t s = 0; s < 70; ++s) all.insert(s);
        const RemovePlan p = remove_plan(masks(count, off, owned, nb, {{}, all, {}}), count, off, owned);
        CHECK(p.removed_total == 70);
        CHECK((p.new_count == U64{100, 0, 5}));
        CHECK((p.new_off == U64{0, 2, 2}));
        CHECK(p.new_blocks == 3);
        CHECK((p.removed == U64{0, 70, 0}));
        CHECK(p.base[0] == 0 && p.base[1] == 64 && p.base[4] == 128);
    }
    {  // the first full block of a three-block list (150 = 64 + 64 + 22) behind a one-block list
        const U64 count = {10, 150};
        const U8 owned = {1, 1};
        uint64_t nb;
        const U64 off = pack(count, owned, nb);
        CHECK(nb == 4);
        std::set<uint64_t> first;
        for (uint64_t s = 0; s < 64; ++s) first.insert(s);
        RemovePlan p = remove_plan(masks(count, off, owned, nb, {{}, first}), count, off, owned);
        CHECK(p.removed_total == 64);
        CHECK((p.new_count == U64{10, 86}));
        CHECK((p.new_off == U64{0, 1}));
        CHECK(p.new_blocks == 3);
        CHECK((p.base == U64{0, 64, 64, 128}));
        // ... and only its first 10 rows: the second block's rows start at slot 54 of the
        // list's first new block and run over into the next
        std::set<uint64_t> ten;
        for (uint64_t s = 0; s < 10; ++s) ten.insert(s);
        p = remove_plan(masks(count, off, owned, nb, {{}, ten}), count, off, owned);
        CHECK((p.new_count == U64{10, 140}));
        CHECK(p.new_blocks == 4);
        CHECK((p.base == U64{0, 64, 64 + 54, 64 + 118}));
    }
    {  // only the last, partial block touched; mask bits in the pad lanes are ignored
        const U64 count = {150};
        const U8 owned = {1};
        uint64_t nb;
        const U64 off = pack(count, owned, nb);
        U64 keep = masks(count, off, owned, nb, {{130, 149}});
        keep[2] |= ~0ull << 22;  // (the device never sets these: lanes at or above the count)
        const RemovePlan p = remove_plan(keep, count, off, owned);
        CHECK(p.removed_total == 2);
        CHECK((p.new_count == U64{148}));
        CHECK(p.new_blocks == 3);
        CHECK((p.base == U64{0, 64, 128}));
    }
    {  // lists stored elsewhere and empty lists between stored ones
        const U64 count = {0, 100, 50, 0, 65, 7};
        const U8 owned = {1, 1, 0, 1, 1, 0};
        uint64_t nb;
        const U64 off = pack(count, owned, nb);
        CHECK(nb == 4);
        CHECK((off == U64{0, 0, 2, 2, 2, 4}));
        std::set<uint64_t> head;
        for (uint64_t s = 0; s < 36; ++s) head.insert(s);
        const RemovePlan p = remove_plan(masks(count, off, owned, nb, {{}, head, {}, {}, {64}, {}}), count, off, owned);
        CHECK(p.removed_total == 37);
        CHECK((p.new_count == U64{0, 64, 50, 0, 64, 7}));  // (lists stored elsewhere keep their count)
        CHECK((p.removed == U64{0, 36, 0, 0, 1, 0}));
        CHECK((p.new_off == U64{0, 0, 1, 1, 1, 2}));
        CHECK(p.new_blocks == 2);
        CHECK(p.base[0] == 0 && p.base[1] == 28 && p.base[2] == 64);
        CHECK((vdbe::remove_block_valid(count, off, owned, nb) == std::vector<uint32_t>{64, 36, 64, 1}));
    }
    {  // every list emptied: no block but the caller's slack block
        const U64 count = {70, 3};
        const U8 owned = {1, 1};
        uint64_t nb;
        const U64 off = pack(count, owned, nb);
        const RemovePlan p = remove_plan(U64(nb, 0), count, off, owned);
        CHECK(p.removed_total == 73);
        CHECK((p.new_count == U64{0, 0}));
        CHECK((p.new_off == U64{0, 0}));
        CHECK(p.new_blocks == 0);
    }
    {  // the request: sorted, each id once
        const uint64_t ids[] = {9, 3, ~0ull, 3, 0, 9, 9};
        CHECK((vdbe::remove_sorted_ids(ids, 7) == U64{0, 3, 9, ~0ull}));
        CHECK(vdbe::remove_sorted_ids(nullptr, 0).empty());
    }
}

static uint64_t random_run(uint32_t seed, int cases) {
    std::mt19937_64 rng(seed);
    uint64_t done = 0;
    for (int c = 0; c < cases; ++c) {
        const size_t L = 1 + rng() % 12;
        U64 count(L);
        U8 owned(L);
        std::vector<U64> ids(L);
        const uint64_t id_space = 1 + rng() % 400;  // small: ids repeat within and across lists
        for (size_t l = 0; l < L; ++l) {
            const uint64_t kind = rng() % 6;
            count[l] = kind == 0 ? 0 : (kind == 1 ? 64 * (1 + rng() % 3) : rng() % 200);
            owned[l] = rng() % 5 != 0;
            if (owned[l])
                for (uint64_t s = 0; s < count[l]; ++s) ids[l].push_back(rng() % id_space);
        }
        // the old directory: relayout's packing, sometimes with room a list has not filled
        U64 off(L, 0);
        uint64_t nb = 0;
        const bool roomy = rng() % 4 == 0;
        for (size_t l = 0; l < L; ++l) {
            off[l] = nb;
            if (owned[l]) nb += cdiv64(count[l]) + (roomy ? rng() % 3 : 0);
        }
        // the old arena's ids, pads UINT64_MAX
        U64 arena(nb * 64, ~0ull);
        for (size_t l = 0; l < L; ++l)
            for (size_t s = 0; s < ids[l].size(); ++s) arena[off[l] * 64 + s] = ids[l][s];
        // the request: some ids, repeats, the pad value, sometimes everything or nothing
        U64 req;
        const uint64_t mode = rng() % 8;
        if (mode == 0) {
            for (uint64_t i = 0; i < id_space; ++i) req.push_back(i);
        } else if (mode != 1) {
            const uint64_t n = rng() % (id_space + 1);
            for (uint64_t i = 0; i < n; ++i) req.push_back(rng() % (id_space + 20));
        }
        req.push_back(~0ull);
        const U64 sorted = vdbe::remove_sorted_ids(req.data(), req.size());
        CHECK(std::is_sorted(sorted.begin(), sorted.end()));
        CHECK(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end());
        // mark, as the kernel does it: lane < valid && id not listed
        const std::vector<uint32_t> valid = vdbe::remove_block_valid(count, off, owned, nb);
        U64 keep(nb, 0);
        for (uint64_t b = 0; b < nb; ++b)
            for (uint32_t i = 0; i < 64; ++i)
                if (i < valid[b] && !std::binary_search(sorted.begin(), sorted.end(), arena[b * 64 + i]))
                    keep[b] |= 1ull << i;
        const RemovePlan p = remove_plan(keep, count, off, owned);
        // brute force: filter each list
        std::vector<U64> want(L);
        uint64_t gone = 0, blocks = 0;
        for (size_t l = 0; l < L; ++l) {
            for (uint64_t id : ids[l])
                if (!std::binary_search(sorted.begin(), sorted.end(), id)) want[l].push_back(id);
            gone += ids[l].size() - want[l].size();
            CHECK(p.new_count[l] == (owned[l] ? want[l].size() : count[l]));
            CHECK(p.removed[l] == ids[l].size() - want[l].size());
            CHECK(p.new_off[l] == blocks);
            if (owned[l]) blocks += cdiv64(want[l].size());
        }
        CHECK(p.removed_total == gone);
        CHECK(p.new_blocks == blocks);
        // compact, as the kernel does it, into a cleared arena with its slack block
        U64 fresh((blocks + 1) * 64, ~0ull);
        std::vector<uint8_t> written(fresh.size(), 0);
        bool in_range = true;
        for (uint64_t b = 0; b < nb; ++b)
            for (uint32_t i = 0; i < 64; ++i) {
                if (!((keep[b] >> i) & 1)) continue;
                const uint64_t below = (uint64_t)__builtin_popcountll(keep[b] & ((1ull << i) - 1));
                const uint64_t dest = p.base[b] + below;
                if (dest >= blocks * 64 || written[dest]) {
                    in_range = false;
                    continue;
                }
                written[dest] = 1;
                fresh[dest] = arena[b * 64 + i];
            }
        CHECK(in_range);
        for (size_t l = 0; l < L; ++l) {
            if (!owned[l]) continue;
            const uint64_t slots = cdiv64(want[l].size()) * 64;
            bool same = true;
            for (uint64_t s = 0; s < slots; ++s) {
                const uint64_t got = fresh[p.new_off[l] * 64 + s];
                same &= s < want[l].size() ? (got == want[l][s] && written[p.new_off[l] * 64 + s])
                                           : !written[p.new_off[l] * 64 + s];
            }
            CHECK(same);
        }
        ++done;
    }
    return done;
}

int main() {
    hand_cases();
    const uint64_t n = random_run(20240607u, 3000);
    std::printf("random run: %llu cases\n", (unsigned long long)n);
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
