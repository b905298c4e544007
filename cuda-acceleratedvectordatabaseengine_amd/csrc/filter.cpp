// filter.cpp — vdb_ivf_search_filtered on one handle: a search over the rows an id filter
// allows, through a masked exact scan.
//
// "The result of a filtered search" is the result of vdb_ivf_search on the index built from
// the same centroids by adding only the allowed rows in their original order: per probed list
// the top-min(k, allowed) by (distance, id), the unique-id merge over the slots, the stale-slot
// reuse with "empty list" reading "no allowed row". Bit for bit: ids and distance bits.
//
// Nothing moves and nothing is rebuilt. Per call: mark (ivf_filter_mark: per 64-slot block an
// allow mask, from the ids alone, and per list the allowed count), then per batch the handle's
// own coarse step, the pairs grouped by list (launch_scan_group, the allowed counts as the gate),
// the masked scan (ivf_filter_scan: blocks with an empty mask are skipped, allowed lanes only)
// and the merge (ivf_filter_merge). The lists are read in the fp32 layout
// the handle holds at that moment: the interleaved arena, or the screen's row-major copy while
// the arena is dropped. Exact scan only: the screen's shadow bounds and thresholds describe
// whole lists.
//
// A free function over vdb_ivf's public members, as remove.cpp is and for the same reason: the
// handle's header is one of the sources the build id hashes, and this feature touches no
// existing scan kernel. It calls nothing that changes the handle: no screen_update,
// screen_release, ensure_arena or upload_directory; the workspace is the call's own. What it
// shares with range.cpp (the refusals, the layout choice, the grouping buffers) is exact_call.hpp.
//
// Two parts: search_filtered takes the masks from the call's sorted ids, and search_masked runs
// steps 3 to 6 over masks already on the device. vdb_ivf_search_prepared (prepared.cpp) calls
// the second part alone with a prepared filter's masks.
#include "filter.hpp"

#include <algorithm>
#include <cfloat>

#include "exact_call.hpp"
#include "filter_kernels.hpp"
#include "remove_plan.hpp"

namespace vdbe {

thread_local FilterTiming g_filter_timing;

namespace {

// Event pairs around the scan and the merge of every batch, summed: a small ring, an entry
// read (after waiting for it) when its turn comes again.
struct BatchTimer {
    static constexpr int kRing = 16;
    hipEvent_t e[kRing][3] = {};  // scan begin, scan end = merge begin, merge end
    bool live[kRing] = {};
    int next = 0;
    double scan_ms = 0.0, merge_ms = 0.0;
    BatchTimer() {
        for (auto& q : e)
            for (auto& x : q) HIPCHECK(hipEventCreate(&x));
    }
    ~BatchTimer() {
        for (auto& q : e)
            for (auto& x : q)
                if (x) (void)hipEventDestroy(x);
    }
    void drain(int i) {
        if (!live[i]) return;
        HIPCHECK(hipEventSynchronize(e[i][2]));
        float a = 0.f, b = 0.f;
        HIPCHECK(hipEventElapsedTime(&a, e[i][0], e[i][1]));
        HIPCHECK(hipEventElapsedTime(&b, e[i][1], e[i][2]));
        scan_ms += a;
        merge_ms += b;
        live[i] = false;
    }
    hipEvent_t* take() {
        const int i = next;
        next = (next + 1) % kRing;
        drain(i);
        live[i] = true;
        return e[i];
    }
    void finish() {
        for (int i = 0; i < kRing; ++i) drain(i);
    }
};

}  // namespace

void search_filtered(vdb_ivf& h, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                     const std::vector<uint64_t>& sorted, bool include, float* distances, uint64_t* ids) {
    require(k <= vdbk::kFilterMaxK, "search_filtered serves k <= 64", VDB_ERR_UNSUPPORTED);
    require(sorted.size() < (1ull << 31), "more than 2^31 - 1 ids in one filter", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, "search_filtered");
    g_filter_timing = FilterTiming{};
    if (n == 0 || k == 0) return;
    const uint32_t P = exact_probes(h, nprobe);
    if (P == 0 || h.arena_blocks == 0 || h.total == 0) return search_masked(h, queries, n, nprobe, k, nullptr, nullptr, distances, ids);
    (void)resident_lists(h);  // (refused before any device work)

    hipStream_t s = h.stream;
    const uint64_t nb = h.arena_blocks;
    DevBuf<uint64_t> d_sorted;
    DevBuf<uint32_t> d_valid, d_allowed;
    DevBuf<unsigned long long> d_allow;
    hipEvent_t mark_ev[2] = {nullptr, nullptr};
    struct MarkEvents {
        hipEvent_t* e;
        ~MarkEvents() {
            for (int i = 0; i < 2; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } mark_guard{mark_ev};
    for (auto& x : mark_ev) HIPCHECK(hipEventCreate(&x));
    const std::vector<uint32_t> valid = remove_block_valid(h.count, h.block_off, h.owned, nb);
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

    // 1. the filter and the per-block valid counts to the device
    if (!sorted.empty())
        HIPCHECK(hipMemcpyAsync(d_sorted.ensure(sorted.size()), sorted.data(), sorted.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_valid.ensure(nb), valid.data(), nb * 4, hipMemcpyHostToDevice, s));

    // 2. mark: per block the allow mask, per list the allowed rows (no host round trip)
    HIPCHECK(hipEventRecord(mark_ev[0], s));
    vdbk::launch_filter_mark(h.arena_ids.p, d_valid.p, nb, d_sorted.p, (uint32_t)sorted.size(), include ? 1 : 0,
                             d_allow.ensure(nb), s);
    HIPCHECK(hipGetLastError());
    vdbk::launch_filter_count(d_allow.p, h.d_block_off.p, h.d_count_local.p, h.nlist, d_allowed.ensure(h.nlist), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(mark_ev[1], s));

    // 3. to 6. the scan over those masks (it synchronises the stream and resets the timing)
    search_masked(h, queries, n, nprobe, k, d_allow.p, d_allowed.p, distances, ids);
    float mark = 0.f;
    HIPCHECK(hipEventElapsedTime(&mark, mark_ev[0], mark_ev[1]));
    g_filter_timing.mark_ms = mark;
}

void search_masked(vdb_ivf& h, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                   const unsigned long long* d_allow, const uint32_t* d_allowed, float* distances, uint64_t* ids,
                   const char* call) {
    require(k <= vdbk::kFilterMaxK, std::string(call) + " serves k <= 64", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, call);
    g_filter_timing = FilterTiming{};
    if (n == 0 || k == 0) return;
    const uint32_t P = exact_probes(h, nprobe);
    const size_t nk = (size_t)n * k;
    auto all_unfilled = [&] {
        std::fill(distances, distances + nk, FLT_MAX);
        std::fill(ids, ids + nk, ~0ull);
    };
    if (P == 0 || h.arena_blocks == 0 || h.total == 0) return all_unfilled();
    (void)resident_lists(h);  // (refused before any device work)
    require(d_allow && d_allowed, std::string(call) + ": no masks", VDB_ERR_STATE);

    hipStream_t s = h.stream;
    DevBuf<uint64_t> d_out_i, d_slot_i, d_part_i, d_carry_i;
    ScanGroupBufs grp;
    DevBuf<unsigned long long> d_pairs;
    DevBuf<float> d_q, d_out_d, d_slot_d, d_part_d, d_carry_d;
    vdb_ivf::SearchSlot w;  // the call's own workspace, not one of the ring's
    BatchTimer timer;
    unsigned long long pairs = 0;
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

    HIPCHECK(hipMemcpyAsync(d_q.ensure((size_t)n * h.dim), queries, (size_t)n * h.dim * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(d_pairs.ensure(1), 0, 8, s));

    // a list longer than kScanSegBlocks blocks is cut into segments (the longest list's: the cap)
    const uint32_t segs = vdbk::scan_seg_cap(h.count.data(), h.owned.data(), h.nlist);

    const uint32_t bmax = std::min(h.batch_cap(P, k), n);
    h.ensure_workspace(w, bmax, P, k);
    const size_t BPk = (size_t)bmax * P * k;
    d_slot_d.ensure(BPk);
    d_slot_i.ensure(BPk);
    if (segs > 1) {
        d_part_d.ensure(BPk * segs);
        d_part_i.ensure(BPk * segs);
    }
    d_out_d.ensure(nk);
    d_out_i.ensure(nk);
    grp.ensure(h.nlist, (size_t)bmax * P);
    d_carry_d.ensure((size_t)P * k);
    HIPCHECK(hipMemsetAsync(d_carry_i.ensure((size_t)P * k), 0xFF, (size_t)P * k * 8, s));

    for (uint32_t b0 = 0, B = bmax; b0 < n; b0 += B, B = std::min(B, n - b0)) {
        // 3. the handle's own coarse step: padded queries (w.q) and probes (w.probes)
        h.coarse_batch(w, d_q.p + (size_t)b0 * h.dim, B, P, s);
        HIPCHECK(hipGetLastError());
        hipEvent_t* ev = timer.take();
        // 4. the masked exact scan: the pairs grouped by list, then one item per (list segment, 4 queries)
        HIPCHECK(hipEventRecord(ev[0], s));
        vdbk::launch_scan_group(w.probes.p, B * P, d_allowed, h.d_count_local.p, h.nlist, segs, vdbk::kFilterGroup,
                                grp.cursor.p, grp.pair_start.p, grp.item_start.p, grp.inv.p, s);
        HIPCHECK(hipGetLastError());
        vdbk::FilterScanArgs a;
        fill_scan_list_args(a, h, w, grp, B, P, segs);
        a.allow = d_allow;
        a.k = k;
        a.part_d = segs > 1 ? d_part_d.p : d_slot_d.p;
        a.part_i = segs > 1 ? d_part_i.p : d_slot_i.p;
        vdbk::launch_filter_scan(h.metric, a, s);
        HIPCHECK(hipGetLastError());
        if (segs > 1) {
            vdbk::launch_filter_fold(d_part_d.p, d_part_i.p, w.probes.p, d_allowed, h.d_count_local.p, B * P, segs, k,
                                     d_slot_d.p, d_slot_i.p, s);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipEventRecord(ev[1], s));
        // 5. the merge; the stale carry crosses the batches, so results never depend on `batch`
        vdbk::launch_filter_merge(w.probes.p, d_allowed, d_slot_d.p, d_slot_i.p, d_carry_d.p, d_carry_i.p, B, P, k,
                                  h.stale, d_out_d.p + (size_t)b0 * k, d_out_i.p + (size_t)b0 * k, d_pairs.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[2], s));
    }
    h.cos_finish(d_out_d.p, d_out_i.p, nk, s);  // (CosineDistance: after the last merge; the carry holds -dot)
    HIPCHECK(hipMemcpyAsync(distances, d_out_d.p, nk * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ids, d_out_i.p, nk * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(&pairs, d_pairs.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    // 6. the step times
    timer.finish();
    g_filter_timing.scan_ms = timer.scan_ms;
    g_filter_timing.merge_ms = timer.merge_ms;
    g_filter_timing.pairs_scanned = pairs;
}

}  // namespace vdbe
