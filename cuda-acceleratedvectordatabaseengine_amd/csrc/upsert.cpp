// upsert.cpp — vdb_ivf_upsert(_device) on one handle: replace and insert in one compaction.
//
// "The index after an upsert" is the index remove_ids(every request id) followed by add(W)
// leaves, W being the request's winners: for every distinct id the entry with the largest
// index, in request order. So every stored copy of a listed id goes, survivors keep their
// order in each list, and each winner is appended behind its list's survivors in request
// order, assigned by add's exact assignment (and normalised once under CosineDistance).
//
// The sequence rebuilds the arena twice (remove.cpp compacts into a fresh one, vdb_ivf::append
// relayouts into another); this call moves it once. Steps:
//   resolve   sort (id, position), mark the winners, pack their raw rows and ids densely
//             (upsert_kernels.hip; the exclusive sum over the 64-entry groups' counts is the host's)
//   assign    padded_rows, assign, group_by_key, key_counts: the add side's own members
//   mark      ivf_remove_mark over the stored ids against the sorted request (repeats left in)
//   plan      upsert_plan.hpp: remove_plan's survivors, packed with room for the winners
//   move      ivf_remove_compact with the plan's base into the one fresh arena, then
//             launch_slots_from_order / launch_scatter_rows with append_base, as append does
// The rows never travel through the host; peak memory is old arena + one fresh arena sized
// for survivors and winners.
//
// A free function over vdb_ivf's public members, as remove.cpp is and for the same reason: the
// handle's header is one of the sources the build id hashes.
#include "upsert.hpp"

#include <chrono>

#include "remove.hpp"
#include "remove_kernels.hpp"
#include "upsert_kernels.hpp"
#include "upsert_plan.hpp"

namespace vdbe {

thread_local UpsertTiming g_upsert_timing;

namespace {

struct TimedEvents {
    hipEvent_t e[6] = {};  // begin / end of: resolve, mark, move
    TimedEvents() {
        for (auto& x : e) HIPCHECK(hipEventCreate(&x));
    }
    ~TimedEvents() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
    double ms(int a, int b) const {  // (the stream is synchronised)
        float t = 0.f;
        HIPCHECK(hipEventElapsedTime(&t, e[a], e[b]));
        return t;
    }
};

}  // namespace

void upsert(vdb_ivf& h, const float* d_v, const uint64_t* d_ids, uint64_t n64, uint64_t* replaced, uint64_t* inserted) {
    require(n64 > 0 && n64 < (1ull << 31), "upsert: the caller serves n == 0 and refuses n >= 2^31", VDB_ERR_UNSUPPORTED);
    const uint32_t n = (uint32_t)n64;
    h.quiesce();
    hipStream_t s = h.stream;
    TimedEvents ev;

    // 1. resolve: the sorted ids (what the mark reads), the winners, their rows and ids dense
    DevBuf<uint64_t> d_sorted, w_ids;
    DevBuf<float> w_rows;
    uint64_t nw = 0;
    {
        DevBuf<uint32_t> iota, pos, d_cnt, d_gbase;
        DevBuf<unsigned char> temp;
        DevBuf<uint8_t> win;
        DevBuf<unsigned long long> d_mask;
        const uint64_t groups = cdiv(n, 64);
        size_t tb = 0;
        HIPCHECK(vdbk::upsert_sort_pairs(nullptr, tb, d_ids, d_sorted.ensure(n), iota.ensure(n), pos.ensure(n), n, s));
        temp.ensure(tb);
        HIPCHECK(hipEventRecord(ev.e[0], s));
        vdbk::launch_iota(iota.p, n, s);
        HIPCHECK(vdbk::upsert_sort_pairs(temp.p, tb, d_ids, d_sorted.p, iota.p, pos.p, n, s));
        vdbk::launch_upsert_winners(d_sorted.p, pos.p, n, win.ensure(n), s);
        vdbk::launch_upsert_ballot(win.p, n, d_mask.ensure(groups), d_cnt.ensure(groups), s);
        HIPCHECK(hipGetLastError());
        std::vector<uint32_t> cnt(groups), gbase(groups);
        HIPCHECK(hipMemcpyAsync(cnt.data(), d_cnt.p, groups * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        for (uint64_t g = 0; g < groups; ++g) {  // (nw <= n < 2^31: it fits)
            gbase[g] = (uint32_t)nw;
            nw += cnt[g];
        }
        HIPCHECK(hipMemcpyAsync(d_gbase.ensure(groups), gbase.data(), groups * 4, hipMemcpyHostToDevice, s));
        vdbk::launch_upsert_pack(d_v, d_ids, n, h.dim, d_mask.p, d_gbase.p, w_rows.ensure(nw * h.dim), w_ids.ensure(nw), s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev.e[1], s));
        HIPCHECK(hipStreamSynchronize(s));  // (gbase and the temporaries go)
    }
    g_upsert_timing.resolve_ms = ev.ms(0, 1);

    // 2.-4. the winners as add takes rows in: padded (CosineDistance: unit rows, once), assigned, grouped
    DevBuf<float> tmp;
    const float* vpad = h.padded_rows(w_rows.p, nw, tmp);
    DevBuf<uint32_t> asg, skeys, order, counts;
    h.assign(vpad, nw, asg.ensure(nw));
    h.group_by_key(asg.p, nw, skeys, order);
    const std::vector<uint32_t> added32 = h.key_counts(asg.p, nw, counts);
    const std::vector<uint64_t> added(added32.begin(), added32.end());

    // 5.-6. mark + plan on the current directory (the ids stay in place while the screen serves
    // from its row copy, so the match pass needs no arena)
    DevBuf<unsigned long long> d_keep;
    UpsertPlan plan;
    auto mark_and_plan = [&] {
        const uint64_t nb = h.arena_blocks;
        std::vector<uint64_t> keep(nb, 0);
        if (nb) {
            const std::vector<uint32_t> valid = remove_block_valid(h.count, h.block_off, h.owned, nb);
            DevBuf<uint32_t> d_valid;
            HIPCHECK(hipMemcpyAsync(d_valid.ensure(nb), valid.data(), nb * 4, hipMemcpyHostToDevice, s));
            HIPCHECK(hipEventRecord(ev.e[2], s));
            vdbk::launch_remove_mark(h.arena_ids.p, d_valid.p, nb, d_sorted.p, n, d_keep.ensure(nb), s);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipEventRecord(ev.e[3], s));
            HIPCHECK(hipMemcpyAsync(keep.data(), d_keep.p, nb * 8, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
            g_upsert_timing.mark_ms = ev.ms(2, 3);
        }
        const auto t0 = std::chrono::steady_clock::now();
        plan = upsert_plan(keep, h.count, h.block_off, h.owned, added);
        g_upsert_timing.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    mark_and_plan();

    // 7. the screen's data describes the old lists (and its row copy may be the lists' only fp32
    // copy: screen_release makes the arena whole first); the next search rebuilds it
    h.screen_release();
    h.screen_stale = true;
    {
        // 8. lists that outgrow max_gpu_memory enter the tier, lists that shrink below it leave
        // it; either moves the arena, and the masks are per block of the arena they were taken on
        const std::vector<uint64_t> off0 = h.block_off;
        const uint64_t nb0 = h.arena_blocks;
        h.apply_memory_cap(plan.new_count);
        if (h.block_off != off0 || h.arena_blocks != nb0) mark_and_plan();
    }

    // 9. the one fresh arena; the old one is swapped out only once this one is whole
    const uint64_t blocks = plan.new_blocks;
    DevBuf<float4> na;
    DevBuf<uint64_t> ni;
    fresh_arena(h, blocks, na, ni);

    // 10. the survivors to their places, then the winners behind them
    std::vector<uint64_t> group_start(h.nlist, 0);
    for (uint32_t l = 1; l < h.nlist; ++l) group_start[l] = group_start[l - 1] + added[l - 1];
    DevBuf<uint64_t> d_base, d_gs, d_ab, dest;
    if (h.arena_blocks)
        HIPCHECK(hipMemcpyAsync(d_base.ensure(plan.base.size()), plan.base.data(), plan.base.size() * 8,
                                hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_gs.ensure(h.nlist), group_start.data(), h.nlist * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_ab.ensure(h.nlist), plan.append_base.data(), h.nlist * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipEventRecord(ev.e[4], s));
    if (h.arena_blocks)
        vdbk::launch_remove_compact(h.arena.p, h.arena_ids.p, d_keep.p, d_base.p, h.arena_blocks, h.d4, na.p, ni.p, s);
    vdbk::launch_slots_from_order(skeys.p, nw, d_gs.p, d_ab.p, dest.ensure(nw), s);
    vdbk::launch_scatter_rows(vpad, w_ids.p, order.p, nw, h.dp, dest.p, na.p, ni.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev.e[5], s));
    HIPCHECK(hipStreamSynchronize(s));
    g_upsert_timing.move_ms = ev.ms(4, 5);

    // 11.-14. swap, directory
    h.arena.swap(na);
    h.arena_ids.swap(ni);
    h.arena_blocks = blocks;
    h.block_off = plan.new_off;
    h.count = plan.new_count;
    h.total = h.total - plan.removed_total + plan.added_total;
    h.lc.reset(h.nlist, h.lc.capacity());  // list contents and offsets changed: nothing cached stays valid
    h.upload_directory();
    g_upsert_timing.rows_kept = h.total - plan.added_total;
    g_upsert_timing.rows_written = plan.added_total;
    if (replaced) *replaced = plan.removed_total;
    if (inserted) *inserted = nw;
}

}  // namespace vdbe
