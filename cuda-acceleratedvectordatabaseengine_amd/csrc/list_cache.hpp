// list_cache.hpp — the list-cache tier's bookkeeping: which lists sit where in the HBM cache,
// which leave when room is needed, and how a call is cut into sub-batches that fit. Host
// arithmetic only (no HIP, nothing about data movement), so the CPU tests drive it directly
// (tests/cpp/list_cache_test.cpp). The engine moves the data a plan names (load_lists).
//
// The cache is `capacity` blocks of 64 vectors. A cached list holds one extent of
// cdiv(count, 64) blocks; the length placed is remembered, so freeing never depends on the
// list's live count. Lists that are empty or not stored here are never cached.
//  * Placement is first fit: the lowest free extent that is long enough, the remainder
//    staying free behind the list. A freed extent merges with the free extent after it,
//    then with the one before, so free extents are never adjacent and an empty cache is
//    the single extent {0: capacity}.
//  * plan_loads makes a set of lists resident. The missing ones are placed largest first
//    (count descending, then id). When one does not fit, victims leave one at a time until
//    it does: every cached, unprotected list, the one whose next use (rank: larger = later,
//    ~0 = never) is furthest away first, then the least recently used, then the lowest id.
//    A plan that cannot be placed changes nothing and returns false: over capacity, or out
//    of victims with `repack` off. With `repack` on, running out of victims (fragmentation:
//    the lists fit by size) drops every cached list and lays the wanted ones from offset 0.
//  * cut_subbatches cuts a call's probes into runs of at most bmax queries whose lists fill
//    at most half the cache, so the next run's lists can load beside the current one's.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

namespace vdbe {

// The handle's list sizes (vectors) and which lists it stores, as the cache sees them.
struct ListSizes {
    const std::vector<uint64_t>& count;
    const std::vector<uint8_t>& owned;
    bool cacheable(uint32_t l) const { return l < count.size() && owned[l] && count[l] != 0; }
    uint64_t blocks(uint32_t l) const { return (count[l] + 63) / 64; }

    // Unique cacheable lists of a probe array, in first-seen order (mark: nlist zeros, left so).
    std::vector<uint32_t> unique(const uint32_t* lists, size_t n, std::vector<uint8_t>& mark) const {
        std::vector<uint32_t> out;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t l = lists[i];
            if (!cacheable(l) || mark[l]) continue;
            mark[l] = 1;
            out.push_back(l);
        }
        for (uint32_t l : out) mark[l] = 0;
        return out;
    }
};

class ListCache {
public:
    static constexpr uint64_t kAbsent = ~0ull;
    using Load = std::pair<uint32_t, uint64_t>;  // (list, its block offset in the cache)

    // An empty cache of `capacity` blocks for nlist lists (0: the tier is off). The loads,
    // evictions and blocks-loaded counters run on: they count over the handle's life.
    void reset(uint32_t nlist, uint64_t capacity) {
        cap_ = capacity;
        off_.assign(nlist, kAbsent);
        len_.assign(nlist, 0);
        last_use_.assign(nlist, 0);
        free_.clear();
        if (cap_) free_[0] = cap_;
        used_ = 0;
        resident_ = 0;
    }

    uint64_t capacity() const { return cap_; }
    uint64_t used() const { return used_; }
    uint64_t resident_lists() const { return resident_; }
    uint64_t loads() const { return loads_; }
    uint64_t evictions() const { return evictions_; }
    uint64_t blocks_loaded() const { return blocks_in_; }
    bool resident(uint32_t l) const { return l < off_.size() && off_[l] != kAbsent; }
    uint64_t offset(uint32_t l) const { return off_[l]; }  // kAbsent: not cached
    uint64_t length(uint32_t l) const { return len_[l]; }  // blocks placed (0: not cached)
    uint64_t last_use(uint32_t l) const { return last_use_[l]; }
    const std::map<uint64_t, uint64_t>& free_extents() const { return free_; }  // offset -> blocks

    // Place list l (not cached) in nb blocks and count one load. kAbsent, nothing changed,
    // when no free extent is long enough.
    uint64_t place(uint32_t l, uint64_t nb) {
        for (auto it = free_.begin(); it != free_.end(); ++it) {
            if (it->second < nb) continue;
            const uint64_t off = it->first, len = it->second;
            free_.erase(it);
            if (len > nb) free_[off + nb] = len - nb;
            used_ += nb;
            off_[l] = off;
            len_[l] = nb;
            ++resident_;
            ++loads_;
            blocks_in_ += nb;
            return off;
        }
        return kAbsent;
    }

    // Drop list l (cached) from the cache. (Not counted: `evictions` counts plan_loads' victims.)
    void evict(uint32_t l) {
        const uint64_t nb = len_[l];
        auto it = free_.emplace(off_[l], nb).first;
        off_[l] = kAbsent;
        len_[l] = 0;
        used_ -= nb;
        --resident_;
        auto nx = std::next(it);
        if (nx != free_.end() && it->first + it->second == nx->first) {
            it->second += nx->second;
            free_.erase(nx);
        }
        if (it != free_.begin()) {
            auto pv = std::prev(it);
            if (pv->first + pv->second == it->first) {
                pv->second += it->second;
                free_.erase(it);
            }
        }
    }

    // One more batch: `lists` are its lists, the most recently used from now on.
    void touch(const std::vector<uint32_t>& lists) {
        ++tick_;
        for (uint32_t l : lists) last_use_[l] = tick_;
    }

    // Make `want` (unique cacheable lists) resident; `protect` (per list, `want` among them)
    // are never evicted.
    // True: `loads` names the lists to copy in, in placement order (none: all were cached).
    // False: `want` cannot be placed, `loads` is empty and nothing has changed. The map
    // changes at once; the caller moves the data in stream order.
    template <class Rank>
    bool plan_loads(const std::vector<uint32_t>& want, const std::vector<uint8_t>& protect, const ListSizes& sz,
                    Rank&& rank, bool repack, std::vector<Load>& loads) {
        loads.clear();
        uint64_t need = 0;
        std::vector<uint32_t> miss;
        for (uint32_t l : want) {
            need += sz.blocks(l);
            if (off_[l] == kAbsent) miss.push_back(l);
        }
        if (need > cap_) return false;
        if (miss.empty()) return true;
        auto by_size = [&](uint32_t a, uint32_t b) {
            return sz.count[a] != sz.count[b] ? sz.count[a] > sz.count[b] : a < b;
        };
        const uint32_t nlist = (uint32_t)off_.size();
        std::vector<uint32_t> victims;
        for (uint32_t l = 0; l < nlist; ++l)
            if (off_[l] != kAbsent && !protect[l]) victims.push_back(l);
        std::vector<uint64_t> rk(nlist, 0);
        for (uint32_t v : victims) rk[v] = rank(v);
        std::sort(victims.begin(), victims.end(), [&](uint32_t a, uint32_t b) {
            if (rk[a] != rk[b]) return rk[a] > rk[b];
            return last_use_[a] != last_use_[b] ? last_use_[a] < last_use_[b] : a < b;
        });
        const ListCache before = *this;  // a failed plan puts it back
        std::sort(miss.begin(), miss.end(), by_size);
        size_t vi = 0;
        for (size_t m = 0; m < miss.size(); ++m) {
            const uint32_t l = miss[m];
            uint64_t off;
            while ((off = place(l, sz.blocks(l))) == kAbsent && vi < victims.size()) {
                evict(victims[vi++]);
                ++evictions_;
            }
            if (off != kAbsent) {
                loads.push_back({l, off});
                continue;
            }
            loads.clear();
            if (!repack) {
                *this = before;
                return false;
            }
            // fragmented: keep only `want`, packed from offset 0 (they fit), all placed anew
            for (uint32_t v = 0; v < nlist; ++v)
                if (off_[v] != kAbsent) evict(v);
            loads_ = before.loads_;
            blocks_in_ = before.blocks_in_;
            miss = want;
            std::sort(miss.begin(), miss.end(), by_size);
            m = (size_t)-1;
        }
        return true;
    }

private:
    uint64_t cap_ = 0;                    // capacity in blocks
    std::vector<uint64_t> off_;           // per list: block offset or kAbsent
    std::vector<uint64_t> len_;           // per list: blocks placed
    std::vector<uint64_t> last_use_;      // per list: tick of the last batch that used it
    std::map<uint64_t, uint64_t> free_;   // free extents: block offset -> blocks
    uint64_t tick_ = 0, used_ = 0, resident_ = 0;
    uint64_t loads_ = 0, evictions_ = 0, blocks_in_ = 0;
};

// A call cut into sub-batches: sub-batch b is the queries begin[b] .. begin[b + 1], lists[b]
// its unique cacheable lists in first-seen order, uses[l] the sub-batches that use list l,
// ascending.
struct SubBatches {
    std::vector<uint32_t> begin;  // size() + 1 entries, the last one n
    std::vector<std::vector<uint32_t>> lists;
    std::vector<std::vector<uint32_t>> uses;
    size_t size() const { return lists.size(); }
};

// One query's own lists exceed the cache: no cut can serve the call.
struct QueryOverCapacity : std::runtime_error {
    uint32_t query;
    explicit QueryOverCapacity(uint32_t q) : std::runtime_error("one query's lists exceed the cache"), query(q) {}
};

// Cut the probes [n][P] of a call. A new sub-batch starts at a query when there is none yet,
// when the current one holds bmax queries, or when the query's new lists would take it past
// half the cache (so a query needing more than half sits alone, and so does any query after
// a sub-batch already past half, new lists or not).
inline SubBatches cut_subbatches(const uint32_t* probes, uint32_t n, uint32_t P, uint32_t bmax, const ListSizes& sz,
                                 const ListCache& cache) {
    const size_t nlist = sz.count.size();
    SubBatches sb;
    std::vector<uint8_t> qmark(nlist, 0), umark(nlist, 0);  // (a query's lists, the sub-batch's lists)
    uint64_t blocks = 0;
    for (uint32_t q = 0; q < n; ++q) {
        const std::vector<uint32_t> ql = sz.unique(probes + (size_t)q * P, P, qmark);
        uint64_t qb = 0, add = 0;
        for (uint32_t l : ql) {
            qb += sz.blocks(l);
            if (!umark[l]) add += sz.blocks(l);
        }
        if (qb > cache.capacity()) throw QueryOverCapacity(q);
        if (sb.lists.empty() || q - sb.begin.back() >= bmax || blocks + add > cache.capacity() / 2) {
            if (!sb.lists.empty())
                for (uint32_t l : sb.lists.back()) umark[l] = 0;
            sb.begin.push_back(q);
            sb.lists.emplace_back();
            blocks = 0;
        }
        for (uint32_t l : ql)
            if (!umark[l]) {
                umark[l] = 1;
                sb.lists.back().push_back(l);
                blocks += sz.blocks(l);
            }
    }
    sb.begin.push_back(n);
    sb.uses.resize(nlist);
    for (size_t b = 0; b < sb.size(); ++b)
        for (uint32_t l : sb.lists[b]) sb.uses[l].push_back((uint32_t)b);
    return sb;
}

// The first sub-batch after `cur` that uses list l, or ~0 when none does: plan_loads' rank.
inline uint64_t next_use(const SubBatches& sb, uint32_t l, size_t cur) {
    const auto& u = sb.uses[l];
    auto it = std::upper_bound(u.begin(), u.end(), (uint32_t)cur);
    return it == u.end() ? ~0ull : (uint64_t)*it;
}

}  // namespace vdbe
