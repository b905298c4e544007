// remove.cpp — vdb_ivf_remove_ids on one handle: device-side list compaction.
//
// "The index after a remove" is the index built from the same centroids by adding the
// surviving rows in their original order: survivors keep their order within each list, so
// list contents, sizes, totals and every search result match that index bit for bit.
//
// Three steps: mark (ivf_remove_mark: per 64-slot block a keep mask, from the ids alone), plan
// (remove_plan.hpp, host: new counts, offsets and every old block's destination) and compact
// (ivf_remove_compact: the kept rows into a fresh arena, never in place). The rows never
// travel through the host; peak memory is old arena + new arena, as for an add.
//
// A free function over vdb_ivf's public members, and not a member next to relayout(): the
// handle's header is one of the sources the build id hashes, and this feature touches no scan
// kernel. The price is that fresh_arena below repeats the allocation of vdb_ivf::relayout
// (engine.hpp) — keep the two in step. upsert.cpp calls it too.
#include "remove.hpp"

#include <chrono>

#include "remove_kernels.hpp"
#include "remove_plan.hpp"

namespace vdbe {

thread_local RemoveTiming g_remove_timing;

namespace {

struct TimedEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};  // mark begin / end, compact begin / end
    TimedEvents() {
        for (auto& x : e) HIPCHECK(hipEventCreate(&x));
    }
    ~TimedEvents() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
    double ms(int a, int b) const {
        float t = 0.f;
        HIPCHECK(hipEventElapsedTime(&t, e[a], e[b]));
        return t;
    }
};

}  // namespace

void fresh_arena(vdb_ivf& h, uint64_t blocks, DevBuf<float4>& rows, DevBuf<uint64_t>& ids) {
    const bool host_arena = h.arena.host;
    rows.pooled = ids.pooled = !host_arena && VDB_DEVICE_POOL;
    rows.host = ids.host = host_arena;
    const size_t vec4 = (size_t)(blocks + 1) * h.d4 * 64;
    rows.ensure(vec4);
    ids.ensure((size_t)(blocks + 1) * 64);
    HIPCHECK(hipMemsetAsync(rows.p, 0, vec4 * sizeof(float4), h.stream));
    HIPCHECK(hipMemsetAsync(ids.p, 0xFF, (size_t)(blocks + 1) * 64 * 8, h.stream));
}

uint64_t remove_ids(vdb_ivf& h, const std::vector<uint64_t>& sorted, std::vector<uint64_t>* per_list) {
    require(!h.file_home(), "lists are served from a file (vdb_ivf_open_lists): the index is read-only",
            VDB_ERR_STATE);
    require(sorted.size() < (1ull << 31), "more than 2^31 - 1 ids in one remove", VDB_ERR_UNSUPPORTED);
    h.quiesce();
    g_remove_timing = RemoveTiming{};
    if (per_list) per_list->assign(h.nlist, 0);
    if (sorted.empty() || h.arena_blocks == 0 || h.total == 0) return 0;
    hipStream_t s = h.stream;
    TimedEvents ev;
    DevBuf<uint64_t> d_sorted;
    HIPCHECK(hipMemcpyAsync(d_sorted.ensure(sorted.size()), sorted.data(), sorted.size() * 8, hipMemcpyHostToDevice, s));

    // mark + plan on the current directory (the ids stay in place while the screen serves
    // from its row copy, so the match pass needs no arena)
    DevBuf<unsigned long long> d_keep;
    RemovePlan plan;
    auto mark_and_plan = [&] {
        const uint64_t nb = h.arena_blocks;
        const std::vector<uint32_t> valid = remove_block_valid(h.count, h.block_off, h.owned, nb);
        DevBuf<uint32_t> d_valid;
        std::vector<uint64_t> keep(nb, 0);
        HIPCHECK(hipMemcpyAsync(d_valid.ensure(nb), valid.data(), nb * 4, hipMemcpyHostToDevice, s));
        HIPCHECK(hipEventRecord(ev.e[0], s));
        vdbk::launch_remove_mark(h.arena_ids.p, d_valid.p, nb, d_sorted.p, (uint32_t)sorted.size(), d_keep.ensure(nb), s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev.e[1], s));
        HIPCHECK(hipMemcpyAsync(keep.data(), d_keep.p, nb * 8, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        const auto t0 = std::chrono::steady_clock::now();
        plan = remove_plan(keep, h.count, h.block_off, h.owned);
        g_remove_timing.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_remove_timing.mark_ms = ev.ms(0, 1);
    };
    mark_and_plan();
    if (plan.removed_total == 0) return 0;  // nothing matched: the handle is untouched

    // the screen's data describes the old lists (and its row copy may be the lists' only fp32
    // copy: screen_release makes the arena whole first); the next search rebuilds it
    h.screen_release();
    h.screen_stale = true;
    {
        // a handle in the tier only because of max_gpu_memory leaves it when the survivors fit
        // again; that moves the arena, and the masks are per block of the arena they were taken on
        const std::vector<uint64_t> off0 = h.block_off;
        const uint64_t nb0 = h.arena_blocks;
        h.apply_memory_cap(plan.new_count);
        if (h.block_off != off0 || h.arena_blocks != nb0) mark_and_plan();
    }

    // the fresh arena; the old one is swapped out only once this one is whole
    const uint64_t blocks = plan.new_blocks;
    DevBuf<float4> na;
    DevBuf<uint64_t> ni;
    fresh_arena(h, blocks, na, ni);
    DevBuf<uint64_t> d_base;
    HIPCHECK(hipMemcpyAsync(d_base.ensure(plan.base.size()), plan.base.data(), plan.base.size() * 8,
                            hipMemcpyHostToDevice, s));
    HIPCHECK(hipEventRecord(ev.e[2], s));
    vdbk::launch_remove_compact(h.arena.p, h.arena_ids.p, d_keep.p, d_base.p, h.arena_blocks, h.d4, na.p, ni.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev.e[3], s));
    HIPCHECK(hipStreamSynchronize(s));
    g_remove_timing.compact_ms = ev.ms(2, 3);
    for (uint32_t l = 0; l < h.nlist; ++l)
        if (h.owned[l]) g_remove_timing.rows_kept += plan.new_count[l];

    h.arena.swap(na);
    h.arena_ids.swap(ni);
    h.arena_blocks = blocks;
    h.block_off = plan.new_off;
    h.count = plan.new_count;
    h.total -= plan.removed_total;
    h.lc.reset(h.nlist, h.lc.capacity());  // list contents and offsets changed: nothing cached stays valid
    h.upload_directory();
    if (per_list) *per_list = plan.removed;
    return plan.removed_total;
}

}  // namespace vdbe
