// exact_call.hpp — the host preamble of the exact-scan calls beside the engine (filter.cpp,
// range.cpp, and prepared.cpp which calls into both): what they refuse, the fp32 layout they
// read, their grouping buffers and the head of their scan arguments. A host header over
// vdb_ivf's public members, for those files only.
#pragma once

#include <algorithm>
#include <string>

#include "engine.hpp"
#include "scan_kernels.hpp"

namespace vdbe {

// `call` serves one handle whose lists are resident in HBM.
inline void require_resident_single(const vdb_ivf& h, const char* call) {
    const std::string c(call);
    require(!h.is_group(), c + " is not available on a group handle", VDB_ERR_UNSUPPORTED);
    require(h.world == 1 && h.comm_world == 1,
            c + " is not available on a sharded handle (set_shard / plan_shard / a shard file / "
                "attach_comm with world > 1)",
            VDB_ERR_UNSUPPORTED);
    require(!h.file_home(), c + " is not available while the lists are served from a file (vdb_ivf_open_lists)",
            VDB_ERR_UNSUPPORTED);
    require(!h.tiered() && !h.arena.host,
            c + " is not available in the list-cache tier (list_cache_bytes, or max_gpu_memory exceeded)",
            VDB_ERR_UNSUPPORTED);
}

// The lists a call probes per query.
inline uint32_t exact_probes(const vdb_ivf& h, uint32_t nprobe) {
    const uint32_t P = std::min(nprobe, h.nlist);
    require(P <= (uint32_t)vdbk::kMaxK, "nprobe above 1024 is not supported", VDB_ERR_UNSUPPORTED);
    return P;
}

// The fp32 layout the handle holds at this moment: the interleaved arena, or the screen's
// row-major copy while the arena is dropped.
inline const float4* resident_lists(const vdb_ivf& h) {
    const float4* lists = h.arena_dropped ? (const float4*)h.screen_rows.p : h.arena.p;
    require(lists != nullptr && h.arena_ids.p != nullptr, "the handle holds no fp32 copy of its lists", VDB_ERR_STATE);
    return lists;
}

// The stream is idle before the call's buffers go and before the caller releases the mutex,
// on every way out.
struct StreamFence {
    hipStream_t s;
    ~StreamFence() { (void)hipStreamSynchronize(s); }
};

// What launch_scan_group writes for a batch of at most `pairs` (query, probe) pairs.
struct ScanGroupBufs {
    DevBuf<uint32_t> cursor, pair_start, item_start, inv;
    void ensure(uint32_t nlist, size_t pairs) {
        cursor.ensure(nlist);
        pair_start.ensure((size_t)nlist + 1);
        item_start.ensure((size_t)nlist + 1);
        inv.ensure(pairs);
    }
};

// The head of a scan's arguments for a batch of B queries whose coarse step is in w.
inline void fill_scan_list_args(vdbk::ScanListArgs& a, const vdb_ivf& h, const vdb_ivf::SearchSlot& w,
                                const ScanGroupBufs& g, uint32_t B, uint32_t P, uint32_t segs) {
    a.lists = resident_lists(h);
    a.ids = h.arena_ids.p;
    a.block_off = h.d_block_off.p;
    a.count = h.d_count_local.p;
    a.q = w.q;
    a.inv = g.inv.p;
    a.pair_start = g.pair_start.p;
    a.item_start = g.item_start.p;
    a.nlist = h.nlist;
    a.B = B;
    a.P = P;
    a.d4 = h.d4;
    a.segs = segs;
    a.rows = h.arena_dropped ? 1 : 0;
}

}  // namespace vdbe
