// upsert_plan.hpp — the host side of vdb_ivf_upsert (upsert.cpp), host-only: no HIP headers,
// compiles with plain g++ (tests/cpp/upsert_plan_test.cpp).
//
// An upsert is a remove whose fresh arena leaves room, behind each list's survivors, for the
// rows that come in. The survivors are remove_plan's (remove_plan.hpp: the keep masks of
// ivf_remove_mark, every list's kept count, every old block's place within its list); only
// the packing differs: lists in list order, cdiv(kept[l] + added[l], 64) blocks per stored
// list (vdb_ivf::relayout's rule; the slack block past the last list is the caller's). The
// k-th kept row of list l lands in slot k of the list's new blocks and the j-th incoming row
// in slot kept[l] + j, so the arena is the one remove_ids followed by add leaves.
//
// Also here, because it is the other host-checkable rule of the call: which entries of a
// request win (upsert_winners, the rule ivf_upsert_winners applies to the sorted pairs).
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "remove_plan.hpp"

namespace vdbe {

struct UpsertPlan {
    std::vector<uint64_t> new_count;    // per list: kept + added (a list not stored here: count + added)
    std::vector<uint64_t> new_off;      // per list: first block in the fresh arena
    std::vector<uint64_t> removed;      // per list: stored rows that go
    std::vector<uint64_t> base;         // per OLD block: arena slot (block * 64 + lane) of its first kept row
    std::vector<uint64_t> append_base;  // per list: arena slot of its first incoming row (~0: not stored here)
    uint64_t new_blocks = 0;            // blocks of the fresh arena, the slack block not counted
    uint64_t removed_total = 0;
    uint64_t added_total = 0;
};

// keep / count / block_off / owned: as for remove_plan (keep may be empty when there is no
// arena yet: every stored list is empty then). added[l]: rows coming into list l.
inline UpsertPlan upsert_plan(const std::vector<uint64_t>& keep, const std::vector<uint64_t>& count,
                              const std::vector<uint64_t>& block_off, const std::vector<uint8_t>& owned,
                              const std::vector<uint64_t>& added) {
    const size_t L = count.size();
    const RemovePlan r = remove_plan(keep, count, block_off, owned);  // the survivors, packed without room
    UpsertPlan p;
    p.new_count = r.new_count;
    p.removed = r.removed;
    p.removed_total = r.removed_total;
    p.base = r.base;
    p.new_off.assign(L, 0);
    p.append_base.assign(L, ~0ull);
    uint64_t blocks = 0;
    for (size_t l = 0; l < L; ++l) {
        p.new_off[l] = blocks;
        p.new_count[l] += added[l];
        p.added_total += added[l];
        if (!owned[l]) continue;
        p.append_base[l] = blocks * 64 + r.new_count[l];
        blocks += (p.new_count[l] + 63) / 64;
    }
    p.new_blocks = blocks;
    // every old block keeps its place within its list; the list's first block moved
    for (size_t l = 0; l < L; ++l) {
        if (!owned[l] || count[l] == 0) continue;
        const uint64_t nb = (count[l] + 63) / 64;
        const uint64_t shift = (p.new_off[l] - r.new_off[l]) * 64;  // (room only ever pushes a list back)
        for (uint64_t b = 0; b < nb; ++b) p.base[block_off[l] + b] += shift;
    }
    return p;
}

// Last write wins: win[i] = 1 iff no later entry of ids[0..n) carries ids[i]. Stated as the
// device states it: a stable sort of (id, position), then entry j of the sorted pairs wins
// iff it is the last one or its successor carries another id.
inline std::vector<uint8_t> upsert_winners(const uint64_t* ids, uint64_t n) {
    std::vector<uint32_t> pos(n);
    std::iota(pos.begin(), pos.end(), 0u);
    std::stable_sort(pos.begin(), pos.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
    std::vector<uint8_t> win(n, 0);
    for (uint64_t j = 0; j < n; ++j) win[pos[j]] = j + 1 == n || ids[pos[j + 1]] != ids[pos[j]];
    return win;
}

}  // namespace vdbe
