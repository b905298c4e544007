// range.cpp — vdb_ivf_range_search on one handle: every stored row within a radius of each
// query, through a thresholded exact scan.
//
// "The result of a range search" is, for each query on its own, the result vdb_ivf_search
// gives that single query with the same nprobe and a k no smaller than the rows it probes,
// cut to the entries with id != UINT64_MAX and d <= radius: the reference's sequential fp32
// distances bit for bit, an id stored more than once among the probed lists once at its
// smallest distance, ascending by (distance, id). A query answered alone has no stale slot, so
// the result depends on neither stale_slots nor batch.
//
// Per batch: the handle's own coarse step, the pairs grouped by list (launch_scan_group: eight
// queries share one read of a list), the thresholded scan (ivf_range_scan: hits appended
// to a buffer through one global cursor) and the ordering on the device (three stable radix
// sorts around range_dedup, then range_finish). The size of a batch's result is known only
// after its scan: a batch whose hits exceed the buffer is scanned once more with a buffer of
// the size the cursor counted. The lists are read in the fp32 layout the handle holds at that
// moment: the interleaved arena, or the screen's row-major copy while the arena is dropped.
// The exact scan, unless the caller chose the screen (below).
//
// With a prepared filter's masks (d_allow, d_allowed: prepared.cpp) the same call runs over the
// allowed rows: the allowed counts gate the grouping, so a list without an allowed row gets no
// item, and the masked scan (ivf_range_scan_masked) appends allowed rows only. Everything after
// the scan is the same code.
//
// Through the screen (vdb_ivf_range_search_screened; `screen`, routed by range_route.hpp): while
// the handle holds a live screen, a batch's scan is replaced by three steps that read the
// shadow instead of the fp32 lists. The pairs are grouped sixteen to an item (one MFMA A
// operand); launch_screen_pairs, the screened search's own kernel, writes their A rows and
// norms into the call's workspace; ivf_range_screen (range_screen_kernels.hip) computes the
// screened search's lower bound of every (query, row) pair on the matrix cores and appends the
// pairs it cannot discard (not lb > radius) to a candidate buffer; ivf_range_recheck computes
// those pairs' exact distances from the screen's row-major copy and appends the hits exactly as
// the scan does. lb <= d for every pair, so no hit is lost, and the hits' bits are the scan's.
// A batch whose candidates exceed the buffer (kRangeCandPerHit times the hit buffer's entries) is
// served by the exact scan instead; a batch whose hits exceed the hit buffer runs its re-check
// once more, the candidates kept. Without a live screen the whole call is the exact path.
//
// A free function over vdb_ivf's public members, as filter.cpp is and for the same reason. It
// calls nothing that changes the handle: no screen_update, screen_release, ensure_arena or
// upload_directory; the workspace is the call's own. What it shares with filter.cpp (the
// refusals, the layout choice, the grouping buffers) is exact_call.hpp.
#include "range.hpp"

#include <algorithm>
#include <cmath>

#include "cosine_map.hpp"
#include "exact_call.hpp"
#include "range_kernels.hpp"
#include "range_route.hpp"
#include "range_screen_kernels.hpp"

namespace vdbe {

thread_local RangeTiming g_range_timing;
thread_local RangeScreenTiming g_range_screen_timing;

namespace {

struct Events {
    // scan begin, scan end, order begin, order end; screened: pairs begin, pairs end, bound end
    hipEvent_t e[7] = {};
    Events() {
        for (auto& x : e) HIPCHECK(hipEventCreate(&x));
    }
    ~Events() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
    double ms(int a, int b) {
        float t = 0.f;
        HIPCHECK(hipEventElapsedTime(&t, e[a], e[b]));
        return t;
    }
};

// The device buffers that hold and order a batch's hits: one allocation, cut into the four
// key / id arrays, the two permutations and the sorts' scratch.
struct HitBufs {
    DevBuf<unsigned char> slab;
    uint64_t *key_a = nullptr, *id_a = nullptr, *key_b = nullptr, *id_b = nullptr;
    uint32_t *perm_a = nullptr, *perm_b = nullptr;
    void* temp = nullptr;
    uint64_t cap = 0;
    size_t temp_bytes = 0;
    void ensure(uint64_t entries, uint32_t B) {
        if (entries <= cap) return;
        HIPCHECK(vdbk::range_order_temp_bytes(entries, B, temp_bytes));
        const size_t e8 = (entries * 8 + 255) / 256 * 256, e4 = (entries * 4 + 255) / 256 * 256;
        unsigned char* p = slab.ensure(4 * e8 + 2 * e4 + temp_bytes);
        key_a = (uint64_t*)p;
        id_a = (uint64_t*)(p + e8);
        key_b = (uint64_t*)(p + 2 * e8);
        id_b = (uint64_t*)(p + 3 * e8);
        perm_a = (uint32_t*)(p + 4 * e8);
        perm_b = (uint32_t*)(p + 4 * e8 + e4);
        temp = p + 4 * e8 + 2 * e4;
        cap = entries;
    }
};

}  // namespace

std::unique_ptr<vdb_range_result> range_search(vdb_ivf& h, const float* queries, uint32_t n, uint32_t nprobe,
                                               float radius, uint64_t reserve, const unsigned long long* d_allow,
                                               const uint32_t* d_allowed, bool screen) {
    require(!std::isnan(radius), "the radius is NaN");
    require_resident_single(h, "range_search");
    g_range_timing = RangeTiming{};
    if (screen) g_range_screen_timing = RangeScreenTiming{};
    auto res = std::make_unique<vdb_range_result>();
    res->n = n;
    res->lims.assign((size_t)n + 1, 0);
    if (n == 0) return res;
    const uint32_t P = exact_probes(h, nprobe);
    if (P == 0 || h.arena_blocks == 0 || h.total == 0) return res;
    (void)resident_lists(h);  // (refused before any device work)

    // CosineDistance: the radius is in mapped distances; the scan thresholds the handle's own
    // -dot at the largest t with fl(1.0f + t) <= radius, and the hits are mapped on the way out
    // (on the host: the same IEEE add as launch_cos_finish). The order stays (-dot, id).
    const float scan_radius = h.unit_rows ? cos_threshold(radius) : radius;

    hipStream_t s = h.stream;
    DevBuf<uint32_t> d_start;
    ScanGroupBufs grp;
    DevBuf<unsigned long long> d_ctrl, d_sctrl;
    DevBuf<uint2> d_cand;  // through the screen: the pairs the bound could not discard
    DevBuf<float> d_q;
    HitBufs hit;
    vdb_ivf::SearchSlot w;  // the call's own workspace, not one of the ring's
    Events ev;
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

    HIPCHECK(hipMemcpyAsync(d_q.ensure((size_t)n * h.dim), queries, (size_t)n * h.dim * 4, hipMemcpyHostToDevice, s));

    // a list longer than kScanSegBlocks blocks is cut into segments (the longest list's: the cap)
    const uint32_t segs = vdbk::scan_seg_cap(h.count.data(), h.owned.data(), h.nlist);

    const uint32_t bmax = std::min(h.batch_cap(P, 1), n);
    h.ensure_workspace(w, bmax, P, 1);
    grp.ensure(h.nlist, (size_t)bmax * P);
    d_start.ensure((size_t)bmax + 1);
    d_ctrl.ensure(vdbk::kRangeCtrlWords);
    const uint64_t hit_cap0 = range_hit_cap(reserve, kRangeAutoReserve);
    hit.ensure(hit_cap0, bmax);
    std::vector<uint32_t> start((size_t)bmax + 1);

    // Through the screen (range_route.hpp) only with the screen the handle holds right now: the
    // call builds and releases nothing. The pairs kernel writes into the call's own workspace.
    RangeScreenFacts rf;
    rf.asked = screen;
    rf.screen_ready = h.screen_ready;
    rf.screen_stale = h.screen_stale;
    rf.rows = h.screen_rows.p != nullptr && h.screen_sh.p != nullptr && h.screen_meta.p != nullptr &&
              (!h.screen_fmt_i8 || h.screen_scale.p != nullptr);
    rf.metric = h.config_metric();
    rf.dp = h.dp;
    rf.i8 = h.screen_fmt_i8;
    rf.slots = h.arena_blocks * 64;
    const bool via_screen = range_screen_serves(rf);
    const uint64_t cand_cap = range_cand_cap(hit_cap0);
    if (via_screen) {
        const size_t bp = (size_t)bmax * P;
        w.qres.ensure(bp * h.dp);
        w.pst.ensure(bp);
        w.qscale.ensure(bp);
        w.thr4.ensure(4 * bp);
        // (what the pairs kernel resets for the deferred search: the int8 one writes them unguarded)
        w.scnt.ensure(bp);
        w.ovf.ensure(bp);
        w.ubcnt.ensure(bp);
        d_cand.ensure(cand_cap);
        d_sctrl.ensure(vdbk::kRsCtrlWords);
    }

    for (uint32_t b0 = 0, B = bmax; b0 < n; b0 += B, B = std::min(B, n - b0)) {
        // 1. the handle's own coarse step: padded queries (w.q) and probes (w.probes)
        h.coarse_batch(w, d_q.p + (size_t)b0 * h.dim, B, P, s);
        HIPCHECK(hipGetLastError());
        unsigned long long ctrl[vdbk::kRangeCtrlWords] = {};
        bool exact = !via_screen;
        if (via_screen) {
            // 2s. the pairs grouped by list, one item per (list segment, 16 queries: one MFMA A
            // operand); the pairs' A rows and norms; every pair's lower bound against the radius
            unsigned long long sc[vdbk::kRsCtrlWords] = {};
            HIPCHECK(hipEventRecord(ev.e[0], s));
            vdbk::launch_scan_group(w.probes.p, B * P, d_allow ? d_allowed : h.d_count_local.p, h.d_count_local.p,
                                    h.nlist, segs, vdbk::kRangeScreenGroup, grp.cursor.p, grp.pair_start.p,
                                    grp.item_start.p, grp.inv.p, s);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipEventRecord(ev.e[4], s));
            vdbk::launch_screen_pairs(h.metric, w.q, B, P, w.probes.p, h.cent_rm.p, h.dp, w.qres.p, w.pst.p, w.thr4.p, s,
                                      w.scnt.p, w.ovf.p, w.counters.p, w.ubcnt.p, rf.i8 ? w.qscale.p : nullptr);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipEventRecord(ev.e[5], s));
            vdbk::RangeScreenArgs a;
            a.shadow = h.screen_sh.p;
            a.meta = h.screen_meta.p;
            a.sscale = rf.i8 ? h.screen_scale.p : nullptr;
            a.qres = w.qres.p;
            a.pst = w.pst.p;
            a.qscale = rf.i8 ? w.qscale.p : nullptr;
            a.block_off = h.d_block_off.p;
            a.count = h.d_count_local.p;
            a.inv = grp.inv.p;
            a.pair_start = grp.pair_start.p;
            a.item_start = grp.item_start.p;
            a.nlist = h.nlist;
            a.B = B;
            a.P = P;
            a.dp = h.dp;
            a.segs = segs;
            a.radius = scan_radius;
            a.allow = d_allow;
            a.allowed = d_allowed;
            a.cand = d_cand.p;
            a.cand_cap = cand_cap;
            a.ctrl = d_sctrl.p;
            require(vdbk::range_screen_serves_shape(a), "range_search: the row padding does not fit the screen's k-steps",
                    VDB_ERR_STATE);
            HIPCHECK(hipMemsetAsync(d_sctrl.p, 0, sizeof(sc), s));
            vdbk::launch_range_screen(h.metric, a, s);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipEventRecord(ev.e[6], s));
            HIPCHECK(hipMemcpyAsync(sc, d_sctrl.p, sizeof(sc), hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
            g_range_timing.scan_ms += ev.ms(0, 6);
            g_range_screen_timing.pairs_ms += ev.ms(4, 5);
            g_range_screen_timing.bound_ms += ev.ms(5, 6);
            require(!(sc[vdbk::kRsStatus] & vdbk::kRangeUnserved),
                    "range_search: the bound kernel refused the launch's shape", VDB_ERR_STATE);
            g_range_screen_timing.pairs_bounded += sc[vdbk::kRsPairs];
            const uint64_t ncand = sc[vdbk::kRsCursor];
            g_range_screen_timing.candidates += ncand;
            // a bound that keeps more than the buffer holds is not pruning: the exact scan serves the batch
            exact = range_falls_back(ncand, cand_cap);
            if (!exact) {
                ++g_range_screen_timing.screened_batches;
                // 3s. the candidates' exact distances, once more if the hits did not fit (the candidates are kept)
                for (int pass = 0; ncand; ++pass) {
                    vdbk::RangeRecheckArgs r;
                    r.cand = d_cand.p;
                    r.n = ncand;
                    r.rows = (const float4*)h.screen_rows.p;
                    r.ids = h.arena_ids.p;
                    r.q = w.q;
                    r.d4 = h.d4;
                    r.radius = scan_radius;
                    r.cap = hit.cap;
                    r.hit_key = hit.key_a;
                    r.hit_id = hit.id_a;
                    r.ctrl = d_ctrl.p;
                    require(vdbk::range_recheck_serves(r), "range_search: the row padding does not fit the re-check's LDS tile",
                            VDB_ERR_STATE);
                    HIPCHECK(hipEventRecord(ev.e[0], s));
                    HIPCHECK(hipMemsetAsync(d_ctrl.p, 0, sizeof(ctrl), s));
                    vdbk::launch_range_recheck(h.metric, r, s);
                    HIPCHECK(hipGetLastError());
                    HIPCHECK(hipEventRecord(ev.e[1], s));
                    HIPCHECK(hipMemcpyAsync(ctrl, d_ctrl.p, sizeof(ctrl), hipMemcpyDeviceToHost, s));
                    HIPCHECK(hipStreamSynchronize(s));
                    g_range_timing.scan_ms += ev.ms(0, 1);
                    g_range_screen_timing.recheck_ms += ev.ms(0, 1);
                    g_range_timing.pairs_scanned += ncand;
                    require(!(ctrl[vdbk::kRangeStatus] & vdbk::kRangeUnserved),
                            "range_search: the re-check kernel refused the launch's shape", VDB_ERR_STATE);
                    const unsigned long long m = ctrl[vdbk::kRangeCursor];
                    require(m < (1ull << 31),
                            "range_search: more than 2^31 - 1 hits in one batch (lower the `batch` option or the radius)",
                            VDB_ERR_UNSUPPORTED);
                    if (m <= hit.cap) break;
                    require(pass == 0, "range_search: the hit count changed between two re-checks of a batch", VDB_ERR_STATE);
                    hit.ensure(m, bmax);  // (the stream is idle)
                    ++g_range_timing.reruns;
                }
            }
        }
        if (exact && screen) ++g_range_screen_timing.exact_batches;
        // 2. the pairs grouped by list, one item per (list segment, 8 queries); empty lists get none
        if (exact) {
            HIPCHECK(hipEventRecord(ev.e[0], s));
            vdbk::launch_scan_group(w.probes.p, B * P, d_allow ? d_allowed : h.d_count_local.p, h.d_count_local.p, h.nlist,
                                    segs, vdbk::kRangeGroup, grp.cursor.p, grp.pair_start.p, grp.item_start.p, grp.inv.p, s);
            HIPCHECK(hipGetLastError());
        }
        // 3. the thresholded scan, once more if the hits did not fit
        for (int pass = 0; exact; ++pass) {
            vdbk::RangeMaskedScanArgs a;  // (the unmasked scan takes its RangeScanArgs part)
            fill_scan_list_args(a, h, w, grp, B, P, segs);
            a.allow = d_allow;
            a.allowed = d_allowed;
            a.radius = scan_radius;
            a.cap = hit.cap;
            a.hit_key = hit.key_a;
            a.hit_id = hit.id_a;
            a.ctrl = d_ctrl.p;
            require(vdbk::range_scan_serves(a), "range_search: the row padding does not fit the scan's LDS tile",
                    VDB_ERR_STATE);
            if (pass) HIPCHECK(hipEventRecord(ev.e[0], s));
            HIPCHECK(hipMemsetAsync(d_ctrl.p, 0, sizeof(ctrl), s));
            if (d_allow) vdbk::launch_range_scan_masked(h.metric, a, s);
            else vdbk::launch_range_scan(h.metric, a, s);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipEventRecord(ev.e[1], s));
            HIPCHECK(hipMemcpyAsync(ctrl, d_ctrl.p, sizeof(ctrl), hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
            g_range_timing.scan_ms += ev.ms(0, 1);
            g_range_timing.pairs_scanned += ctrl[vdbk::kRangePairs];
            require(!(ctrl[vdbk::kRangeStatus] & vdbk::kRangeUnserved),
                    "range_search: the scan kernel refused the launch's shape", VDB_ERR_STATE);
            const unsigned long long m = ctrl[vdbk::kRangeCursor];
            require(m < (1ull << 31),
                    "range_search: more than 2^31 - 1 hits in one batch (lower the `batch` option or the radius)",
                    VDB_ERR_UNSUPPORTED);
            if (m <= hit.cap) break;
            require(pass == 0, "range_search: the hit count changed between two scans of a batch", VDB_ERR_STATE);
            hit.ensure(m, bmax);  // (the stream is idle)
            ++g_range_timing.reruns;
        }
        // 4. order and de-duplicate on the device, then the batch's part of the result
        const uint64_t m = ctrl[vdbk::kRangeCursor];
        const uint64_t at = res->ids.size();
        uint64_t kept = 0;
        if (m) {
            vdbk::RangeOrderBufs o;
            o.key_a = hit.key_a;
            o.id_a = hit.id_a;
            o.key_b = hit.key_b;
            o.id_b = hit.id_b;
            o.perm_a = hit.perm_a;
            o.perm_b = hit.perm_b;
            o.temp = hit.temp;
            o.temp_bytes = hit.temp_bytes;
            o.start = d_start.p;
            HIPCHECK(hipEventRecord(ev.e[2], s));
            HIPCHECK(vdbk::launch_range_order(o, m, B, s));
            HIPCHECK(hipEventRecord(ev.e[3], s));
            HIPCHECK(hipMemcpyAsync(start.data(), d_start.p, ((size_t)B + 1) * 4, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
            g_range_timing.order_ms += ev.ms(2, 3);
            kept = start[B];
            res->ids.resize(at + kept);
            res->distances.resize(at + kept);
            if (kept) {
                HIPCHECK(hipMemcpyAsync(res->ids.data() + at, o.key_b, kept * 8, hipMemcpyDeviceToHost, s));
                HIPCHECK(hipMemcpyAsync(res->distances.data() + at, o.perm_a, kept * 4, hipMemcpyDeviceToHost, s));
                HIPCHECK(hipStreamSynchronize(s));
                if (h.unit_rows)
                    for (uint64_t i = at; i < at + kept; ++i) res->distances[i] = cos_map(res->distances[i]);
            }
        } else {
            std::fill(start.begin(), start.end(), 0u);
        }
        for (uint32_t i = 0; i < B; ++i) res->lims[(size_t)b0 + i + 1] = at + start[i + 1];
    }
    g_range_timing.hits = res->ids.size();
    return res;
}

}  // namespace vdbe
