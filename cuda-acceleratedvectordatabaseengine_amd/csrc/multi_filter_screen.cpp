// multi_filter_screen.cpp — vdb_ivf_search_prepared_multi_screened on one handle:
// vdb_ivf_search_prepared_multi's result, bit for bit, reading the screen's shadow instead of
// every fp32 row that any of an item's queries may see.
//
// multi_filter.cpp's call around filter_screen.cpp's batch. Before the batches: the plan (the
// queries in the stable order by filter index), the upload of the queries, qf and the filters'
// two tables, the route (filter_screen_serves) and the candidate buffer (filter_cand_cap). Per
// batch, while the handle holds a live screen:
//   1. the handle's own coarse step;
//   2. the per-pair gate (the rows the pair's own filter allows in its list) and the pairs
//      grouped by list under it, sixteen to an item (one MFMA A operand);
//   3. launch_screen_pairs, the screened search's own kernel, into the call's own workspace;
//   4. ivf_filter_screen_thresh_multi: per pair tau, the exact k-th smallest upper bound over
//      the rows of its list that its own filter allows;
//   5. ivf_filter_screen_bound_multi: those (pair, row)s with !(lb > tau) into the candidate
//      buffer;
//   6. the candidates sorted by (pair, slot) and ivf_filter_screen_select gated per pair, into
//      the slot lists exactly as the masked scan leaves them;
//   7. launch_filter_merge_multi, unchanged, with the same carry_same / carry_f handling.
// A batch whose candidates exceed the buffer is served by the masked scan of multi_filter.cpp
// (the pairs grouped again by four) into the same slot lists. Without a live screen, or for an
// empty index, the whole call is search_prepared_multi.
//
// A free function over vdb_ivf's public members, as its two parents are. It calls nothing that
// changes the handle or a filter; the workspace and the tables are the call's own.
#include "multi_filter_screen.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include "exact_call.hpp"
#include "filter.hpp"
#include "filter_screen_route.hpp"
#include "multi_filter_kernels.hpp"
#include "multi_filter_plan.hpp"
#include "multi_filter_screen_kernels.hpp"
#include "prepared_kernels.hpp"

namespace vdbe {

namespace {

struct Events {
    // gate begin, pairs begin, pairs end, threshold end, bound end, select / scan end, merge end
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

}  // namespace

void search_prepared_multi_screened(vdb_ivf& h, const vdb_filter* const* filters, uint32_t n_filters,
                                    const uint32_t* filter_of, const float* queries, uint32_t n, uint32_t nprobe,
                                    uint32_t k, uint64_t reserve, float* distances, uint64_t* ids) {
    // search_prepared_multi's refusals, in its order
    for (uint32_t f = 0; f < n_filters; ++f) require(filters[f]->h == &h, "the filter belongs to another handle");
    require(k <= vdbk::kFilterMaxK, "search_prepared_multi_screened serves k <= 64", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, "search_prepared_multi_screened");
    for (uint32_t f = 0; f < n_filters; ++f)
        require(filter_live(*filters[f]),
                "the filter is stale: the handle's rows changed after it was prepared (prepare it again)", VDB_ERR_STATE);
    g_filter_screen_timing = FilterScreenTiming{};
    g_filter_timing = FilterTiming{};
    if (n == 0 || k == 0) return;
    const uint32_t P = exact_probes(h, nprobe);
    const bool empty = P == 0 || h.arena_blocks == 0 || h.total == 0;

    FilterScreenFacts rf;
    rf.screen_ready = h.screen_ready;
    rf.screen_stale = h.screen_stale;
    rf.buffers = h.screen_rows.p != nullptr && h.screen_sh.p != nullptr && h.screen_meta.p != nullptr &&
                 (!h.screen_fmt_i8 || h.screen_scale.p != nullptr);
    rf.metric = h.config_metric();
    rf.dp = h.dp;
    rf.i8 = h.screen_fmt_i8;
    rf.slots = h.arena_blocks * 64;
    if (empty || !filter_screen_serves(rf)) {
        search_prepared_multi(h, filters, n_filters, filter_of, queries, n, nprobe, k, distances, ids);
        if (!empty) {
            const uint32_t bmax = std::min(h.batch_cap(P, k), n);
            g_filter_screen_timing.exact_batches = (n + bmax - 1) / bmax;
        }
        return;
    }
    (void)resident_lists(h);  // (refused before any device work)

    // the scanned order, the queries in it, and the filters' tables
    const size_t nk = (size_t)n * k;
    const MultiFilterPlan plan = multi_filter_plan(filter_of, n, n_filters);
    std::vector<float> qp((size_t)n * h.dim);
    for (uint32_t j = 0; j < n; ++j)
        std::memcpy(qp.data() + (size_t)j * h.dim, queries + (size_t)plan.perm[j] * h.dim, (size_t)h.dim * 4);
    std::vector<const unsigned long long*> allow_tab(n_filters);
    std::vector<const uint32_t*> allowed_tab(n_filters);
    for (uint32_t f = 0; f < n_filters; ++f) {
        allow_tab[f] = filters[f]->allow.p;
        allowed_tab[f] = filters[f]->allowed.p;
        require(allow_tab[f] && allowed_tab[f], "search_prepared_multi_screened: no masks", VDB_ERR_STATE);
    }
    std::vector<float> out_d(nk);  // in the scanned order
    std::vector<uint64_t> out_i(nk);

    hipStream_t s = h.stream;
    DevBuf<const unsigned long long*> d_allow_tab;
    DevBuf<const uint32_t*> d_allowed_tab;
    DevBuf<uint32_t> d_qf, d_gate;
    DevBuf<uint64_t> d_out_i, d_slot_i, d_part_i, d_carry_i, d_cand, d_sorted;
    ScanGroupBufs grp;
    DevBuf<unsigned long long> d_pairs, d_ctrl;
    DevBuf<float> d_q, d_out_d, d_slot_d, d_part_d, d_carry_d, d_tau, d_tpart;
    DevBuf<unsigned char> d_temp;
    vdb_ivf::SearchSlot w;  // the call's own workspace, not one of the ring's
    Events ev;
    unsigned long long pairs = 0;
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

    HIPCHECK(hipMemcpyAsync(d_q.ensure((size_t)n * h.dim), qp.data(), (size_t)n * h.dim * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_qf.ensure(n), plan.qf.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_allow_tab.ensure(n_filters), allow_tab.data(), (size_t)n_filters * sizeof(void*),
                            hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_allowed_tab.ensure(n_filters), allowed_tab.data(), (size_t)n_filters * sizeof(void*),
                            hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(d_pairs.ensure(1), 0, 8, s));

    // a list longer than kScanSegBlocks blocks is cut into segments (the longest list's: the cap)
    const uint32_t segs = vdbk::scan_seg_cap(h.count.data(), h.owned.data(), h.nlist);

    const uint32_t bmax = std::min(h.batch_cap(P, k), n);
    h.ensure_workspace(w, bmax, P, k);
    const size_t bp = (size_t)bmax * P, BPk = bp * k;
    d_slot_d.ensure(BPk);
    d_slot_i.ensure(BPk);
    d_out_d.ensure(nk);
    d_out_i.ensure(nk);
    grp.ensure(h.nlist, bp);
    d_gate.ensure(bp);
    d_carry_d.ensure((size_t)P * k);
    HIPCHECK(hipMemsetAsync(d_carry_i.ensure((size_t)P * k), 0xFF, (size_t)P * k * 8, s));
    uint32_t carry_f = kNoCarry;  // the filter the carry belongs to
    // the pairs kernel writes into the call's own workspace
    w.qres.ensure(bp * h.dp);
    w.pst.ensure(bp);
    w.qscale.ensure(bp);
    w.thr4.ensure(4 * bp);
    // (what the pairs kernel resets for the deferred search: the int8 one writes them unguarded)
    w.scnt.ensure(bp);
    w.ovf.ensure(bp);
    w.ubcnt.ensure(bp);
    d_tau.ensure(bp);
    if (segs > 1) d_tpart.ensure(BPk * segs);
    const uint64_t cand_cap = filter_cand_cap(reserve, bmax, P, k);
    d_cand.ensure(cand_cap);
    d_sorted.ensure(cand_cap);
    size_t sort_bytes = 0;
    HIPCHECK(vdbk::filter_sort_temp_bytes((uint32_t)cand_cap, sort_bytes));
    d_temp.ensure(sort_bytes);
    d_ctrl.ensure(vdbk::kFsCtrlWords);

    for (uint32_t b0 = 0, B = bmax; b0 < n; b0 += B, B = std::min(B, n - b0)) {
        // 1. the handle's own coarse step: padded queries (w.q) and probes (w.probes)
        h.coarse_batch(w, d_q.p + (size_t)b0 * h.dim, B, P, s);
        HIPCHECK(hipGetLastError());
        // 2. the pairs gated by their own filter and grouped by list, one item per (list segment, 16 pairs)
        HIPCHECK(hipEventRecord(ev.e[0], s));
        vdbk::launch_pair_gate(w.probes.p, d_qf.p + b0, d_allowed_tab.p, B, P, d_gate.p, s);
        HIPCHECK(hipGetLastError());
        vdbk::launch_scan_group_pairs(w.probes.p, B * P, d_gate.p, h.d_count_local.p, h.nlist, segs,
                                      vdbk::kFilterScreenGroup, grp.cursor.p, grp.pair_start.p, grp.item_start.p,
                                      grp.inv.p, s);
        HIPCHECK(hipGetLastError());
        // 3. the pairs' A rows and norms
        HIPCHECK(hipEventRecord(ev.e[1], s));
        vdbk::launch_screen_pairs(h.metric, w.q, B, P, w.probes.p, h.cent_rm.p, h.dp, w.qres.p, w.pst.p, w.thr4.p, s,
                                  w.scnt.p, w.ovf.p, w.counters.p, w.ubcnt.p, rf.i8 ? w.qscale.p : nullptr);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev.e[2], s));
        // 4. and 5. tau per pair, then the rows it cannot discard
        vdbk::MultiFilterScreenArgs a;
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
        a.probes = w.probes.p;
        a.nlist = h.nlist;
        a.B = B;
        a.P = P;
        a.dp = h.dp;
        a.segs = segs;
        a.k = k;
        a.allow_tab = d_allow_tab.p;
        a.qf = d_qf.p + b0;
        a.gate = d_gate.p;
        a.part = d_tpart.p;
        a.tau = d_tau.p;
        a.cand = d_cand.p;
        a.cand_cap = cand_cap;
        a.ctrl = d_ctrl.p;
        require(vdbk::filter_screen_serves_shape(a),
                "search_prepared_multi_screened: the row padding does not fit the screen's k-steps", VDB_ERR_STATE);
        unsigned long long ctrl[vdbk::kFsCtrlWords] = {};
        HIPCHECK(hipMemsetAsync(d_ctrl.p, 0, sizeof(ctrl), s));
        vdbk::launch_filter_screen_thresh_multi(h.metric, a, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev.e[3], s));
        vdbk::launch_filter_screen_bound_multi(h.metric, a, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev.e[4], s));
        HIPCHECK(hipMemcpyAsync(ctrl, d_ctrl.p, sizeof(ctrl), hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        require(!(ctrl[vdbk::kFsStatus] & vdbk::kRangeUnserved),
                "search_prepared_multi_screened: a shadow kernel refused the launch's shape", VDB_ERR_STATE);
        const uint64_t ncand = ctrl[vdbk::kFsCursor];
        g_filter_screen_timing.pairs_bounded += ctrl[vdbk::kFsPairs];
        g_filter_screen_timing.candidates += ncand;
        if (!filter_falls_back(ncand, cand_cap)) {
            // 6. per pair the exact top-k of its candidates
            ++g_filter_screen_timing.screened_batches;
            if (ncand) HIPCHECK(vdbk::launch_filter_sort(d_temp.p, sort_bytes, d_cand.p, d_sorted.p, (uint32_t)ncand, s));
            vdbk::FilterSelectArgs r;
            r.cand = d_sorted.p;
            r.n = ncand;
            r.rows = (const float4*)h.screen_rows.p;
            r.ids = h.arena_ids.p;
            r.q = w.q;
            r.probes = w.probes.p;
            r.gate = d_gate.p;
            r.BP = B * P;
            r.P = P;
            r.d4 = h.d4;
            r.k = k;
            r.slot_d = d_slot_d.p;
            r.slot_i = d_slot_i.p;
            r.ctrl = d_ctrl.p;
            require(vdbk::filter_select_serves(r),
                    "search_prepared_multi_screened: the row padding does not fit the select's LDS tile", VDB_ERR_STATE);
            vdbk::launch_filter_screen_select(h.metric, r, s);
            HIPCHECK(hipGetLastError());
        } else {
            // a bound that keeps more than the buffer holds is not pruning: the masked exact scan
            // serves the batch, the pairs grouped again by four
            ++g_filter_screen_timing.exact_batches;
            if (segs > 1) {
                d_part_d.ensure(BPk * segs);  // (the stream is idle)
                d_part_i.ensure(BPk * segs);
            }
            vdbk::launch_scan_group_pairs(w.probes.p, B * P, d_gate.p, h.d_count_local.p, h.nlist, segs,
                                          vdbk::kFilterGroup, grp.cursor.p, grp.pair_start.p, grp.item_start.p,
                                          grp.inv.p, s);
            HIPCHECK(hipGetLastError());
            vdbk::MultiFilterScanArgs x;
            fill_scan_list_args(x, h, w, grp, B, P, segs);
            x.allow_tab = d_allow_tab.p;
            x.qf = d_qf.p + b0;
            x.k = k;
            x.part_d = segs > 1 ? d_part_d.p : d_slot_d.p;
            x.part_i = segs > 1 ? d_part_i.p : d_slot_i.p;
            vdbk::launch_filter_scan_multi(h.metric, x, s);
            HIPCHECK(hipGetLastError());
            if (segs > 1) {
                vdbk::launch_filter_fold_multi(d_part_d.p, d_part_i.p, w.probes.p, d_gate.p, h.d_count_local.p, B * P,
                                               segs, k, d_slot_d.p, d_slot_i.p, s);
                HIPCHECK(hipGetLastError());
            }
        }
        HIPCHECK(hipEventRecord(ev.e[5], s));
        // 7. the merge; the carry crosses the batches inside a filter, so results never depend on `batch`
        const int carry_same = carry_f == plan.qf[b0] ? 1 : 0;
        vdbk::launch_filter_merge_multi(d_gate.p, d_qf.p + b0, d_slot_d.p, d_slot_i.p, d_carry_d.p, d_carry_i.p,
                                        carry_same, B, P, k, h.stale, d_out_d.p + (size_t)b0 * k,
                                        d_out_i.p + (size_t)b0 * k, d_pairs.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev.e[6], s));
        carry_f = plan.qf[b0 + B - 1];
        HIPCHECK(hipMemcpyAsync(ctrl, d_ctrl.p, sizeof(ctrl), hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        require(!(ctrl[vdbk::kFsStatus] & vdbk::kRangeUnserved),
                "search_prepared_multi_screened: the select kernel refused the launch's shape", VDB_ERR_STATE);
        g_filter_screen_timing.pairs_ms += ev.ms(1, 2);
        g_filter_screen_timing.thresh_ms += ev.ms(2, 3);
        g_filter_screen_timing.bound_ms += ev.ms(3, 4);
        g_filter_screen_timing.select_ms += ev.ms(4, 5);
        g_filter_timing.scan_ms += ev.ms(0, 5);
        g_filter_timing.merge_ms += ev.ms(5, 6);
    }
    h.cos_finish(d_out_d.p, d_out_i.p, nk, s);  // (CosineDistance: after the last merge; the carry holds -dot)
    HIPCHECK(hipMemcpyAsync(out_d.data(), d_out_d.p, nk * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(out_i.data(), d_out_i.p, nk * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(&pairs, d_pairs.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    // back into request order (the outputs are written only now)
    for (uint32_t j = 0; j < n; ++j) {
        std::memcpy(distances + (size_t)plan.perm[j] * k, out_d.data() + (size_t)j * k, (size_t)k * 4);
        std::memcpy(ids + (size_t)plan.perm[j] * k, out_i.data() + (size_t)j * k, (size_t)k * 8);
    }
    g_filter_timing.pairs_scanned = pairs;
}

}  // namespace vdbe
