// filter_epoch.hpp — when a prepared filter (vdb_filter, prepared.cpp) stops describing its
// handle. Host only, no HIP headers: compiles with plain g++ (tests/cpp/filter_epoch_test.cpp).
//
// A filter's masks are addressed by arena block and slot, so they hold only while every stored
// row sits in the slot it sat in when the masks were taken. The block geometry alone does not
// tell: removing a row from a list and adding one to the same list restores every count with
// other rows underneath. So every handle has an epoch, a value drawn from one process-wide
// counter, and every C ABI entry point that can change which row sits in which slot draws a new
// one (bump). A filter remembers the epoch it was made under and is live while the handle still
// has that epoch. A handle that is destroyed loses its entry (erase), and a later handle at the
// same address draws values the counter has never given before, so it never matches an old
// filter. The handle itself is never read here: a key is an address, nothing more.
#pragma once

#include <cstdint>
#include <mutex>
#include <unordered_map>

namespace vdbe {

class FilterEpochs {
public:
    // The handle's epoch, drawn now if it has none yet (never 0).
    uint64_t get(const void* handle) {
        std::lock_guard<std::mutex> g(mu_);
        uint64_t& e = map_[handle];
        if (e == 0) e = ++last_;
        return e;
    }
    // The rows of `handle` may have moved: every filter made before this is stale. A handle
    // without an entry has no filter and gets none.
    void bump(const void* handle) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = map_.find(handle);
        if (it != map_.end()) it->second = ++last_;
    }
    // The handle is gone.
    void erase(const void* handle) {
        std::lock_guard<std::mutex> g(mu_);
        map_.erase(handle);
    }
    // True while `handle` exists and still has the epoch `epoch`.
    bool live(const void* handle, uint64_t epoch) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = map_.find(handle);
        return epoch != 0 && it != map_.end() && it->second == epoch;
    }
    size_t size() {
        std::lock_guard<std::mutex> g(mu_);
        return map_.size();
    }

private:
    std::mutex mu_;
    std::unordered_map<const void*, uint64_t> map_;
    uint64_t last_ = 0;  // the latest value given out: values only grow
};

// The process's one table.
inline FilterEpochs& filter_epochs() {
    static FilterEpochs e;
    return e;
}

}  // namespace vdbe
