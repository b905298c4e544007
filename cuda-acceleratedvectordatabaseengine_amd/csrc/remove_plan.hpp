// remove_plan.hpp — the host side of vdb_ivf_remove_ids (remove.cpp), host-only: no HIP
// headers, compiles with plain g++ (tests/cpp/remove_plan_test.cpp).
//
// A remove is a relayout whose copy compacts. The device marks, per 64-slot arena block, the
// slots that stay (one bit per slot, ivf_remove_mark); from those masks and the old directory
// this header computes where every block's survivors go in the fresh arena, by the packing
// rule of vdb_ivf::relayout: lists in list order, cdiv(count, 64) blocks per stored list (the
// slack block past the last list is the caller's). Survivors keep their order within a list,
// so the k-th kept row of a list lands in slot k of the list's new blocks.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace vdbe {

// The request's ids as the mark kernel's binary search reads them: sorted, each once.
inline std::vector<uint64_t> remove_sorted_ids(const uint64_t* ids, uint64_t n) {
    std::vector<uint64_t> s(ids, ids + n);
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    return s;
}

// Per old arena block the slots that hold a row (0..64): only those are matched, never the
// pad slots of a list's last block, and never a block no stored, non-empty list covers.
inline std::vector<uint32_t> remove_block_valid(const std::vector<uint64_t>& count,
                                                const std::vector<uint64_t>& block_off,
                                                const std::vector<uint8_t>& owned, uint64_t arena_blocks) {
    std::vector<uint32_t> valid(arena_blocks, 0);
    for (size_t l = 0; l < count.size(); ++l) {
        if (!owned[l] || count[l] == 0) continue;
        const uint64_t nb = (count[l] + 63) / 64;
        for (uint64_t b = 0; b < nb; ++b)
            valid[block_off[l] + b] = (uint32_t)std::min<uint64_t>(64, count[l] - b * 64);
    }
    return valid;
}

struct RemovePlan {
    std::vector<uint64_t> new_count;  // per list (a list not stored here keeps its count)
    std::vector<uint64_t> new_off;    // per list: first block in the fresh arena
    std::vector<uint64_t> removed;    // per list: rows that go
    std::vector<uint64_t> base;       // per OLD block: arena slot (block * 64 + lane) of its first kept row
    uint64_t new_blocks = 0;          // blocks of the fresh arena, the slack block not counted
    uint64_t removed_total = 0;
};

// keep[b]: bit i set = slot i of old block b stays (bits at or above the block's valid slots
// are ignored). count / block_off / owned: the directory the masks were taken on.
inline RemovePlan remove_plan(const std::vector<uint64_t>& keep, const std::vector<uint64_t>& count,
                              const std::vector<uint64_t>& block_off, const std::vector<uint8_t>& owned) {
    const size_t L = count.size();
    RemovePlan p;
    p.new_count = count;
    p.new_off.assign(L, 0);
    p.removed.assign(L, 0);
    p.base.assign(keep.size(), 0);
    std::vector<uint64_t> kept_before(keep.size(), 0);  // per old block: kept rows of its list before it
    for (size_t l = 0; l < L; ++l) {
        if (!owned[l] || count[l] == 0) continue;
        const uint64_t nb = (count[l] + 63) / 64;
        uint64_t kept = 0;
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t valid = std::min<uint64_t>(64, count[l] - b * 64);
            const uint64_t lanes = valid == 64 ? ~0ull : ((1ull << valid) - 1);
            kept_before[block_off[l] + b] = kept;
            kept += (uint64_t)__builtin_popcountll(keep[block_off[l] + b] & lanes);
        }
        p.new_count[l] = kept;
        p.removed[l] = count[l] - kept;
        p.removed_total += p.removed[l];
    }
    uint64_t blocks = 0;
    for (size_t l = 0; l < L; ++l) {
        p.new_off[l] = blocks;
        if (owned[l]) blocks += (p.new_count[l] + 63) / 64;
    }
    p.new_blocks = blocks;
    for (size_t l = 0; l < L; ++l) {
        if (!owned[l] || count[l] == 0) continue;
        const uint64_t nb = (count[l] + 63) / 64;
        for (uint64_t b = 0; b < nb; ++b) p.base[block_off[l] + b] = p.new_off[l] * 64 + kept_before[block_off[l] + b];
    }
    return p;
}

}  // namespace vdbe
