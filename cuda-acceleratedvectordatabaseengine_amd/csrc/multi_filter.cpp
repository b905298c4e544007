// multi_filter.cpp — vdb_ivf_search_prepared_multi on one handle: a batch whose queries each
// name their own prepared filter (a mixed-tenant batch), served by one masked exact scan.
//
// "The result of the mixed call" is the result of the per-filter calls scattered back into
// request order: for every filter index f the rows of the queries S_f that name it are, bit for
// bit, what vdb_ivf_search_prepared returns for filters[f] and the queries of S_f in call order.
// So the reference's stale-slot reuse stays inside a filter.
//
// Per call: the queries are put into the stable order by filter index (multi_filter_plan.hpp),
// which makes every S_f one contiguous run, and uploaded in that order with their filter
// indices (qf) and two small tables, the addresses of the filters' masks and of their per-list
// counts. Then per batch the handle's own coarse step, the per-pair gate (ivf_pair_gate: the
// rows the pair's own filter allows in its list), the pairs grouped by list under that gate
// (launch_scan_group_pairs), the scan with the mask looked up per query (ivf_filter_scan_multi)
// and the merge whose stale walk-back stops where the filter changes (ivf_filter_merge_multi).
// One carry of [P][k] crosses the batches; it belongs to the filter of the latest batch's last
// query and serves the next batch only while that batch begins with the same filter. The rows
// come back in the scanned order and are scattered into request order on the host.
//
// Free functions over vdb_ivf's public members, as filter.cpp and prepared.cpp are and for the
// same reason. Nothing here changes the handle or a filter; the workspace and the tables are
// the call's own and are gone when it returns.
#include "multi_filter.hpp"

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "exact_call.hpp"
#include "filter.hpp"
#include "multi_filter_kernels.hpp"
#include "multi_filter_plan.hpp"

namespace vdbe {

namespace {

// filter.cpp's BatchTimer: event pairs around the scan and the merge of every batch, summed.
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

void search_prepared_multi(vdb_ivf& h, const vdb_filter* const* filters, uint32_t n_filters, const uint32_t* filter_of,
                           const float* queries, uint32_t n, uint32_t nprobe, uint32_t k, float* distances,
                           uint64_t* ids) {
    // the refusals of search_prepared, in its order, for every filter of the table
    for (uint32_t f = 0; f < n_filters; ++f) require(filters[f]->h == &h, "the filter belongs to another handle");
    require(k <= vdbk::kFilterMaxK, "search_prepared_multi serves k <= 64", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, "search_prepared_multi");
    for (uint32_t f = 0; f < n_filters; ++f)
        require(filter_live(*filters[f]),
                "the filter is stale: the handle's rows changed after it was prepared (prepare it again)", VDB_ERR_STATE);
    g_filter_timing = FilterTiming{};
    if (n == 0 || k == 0) return;
    const uint32_t P = exact_probes(h, nprobe);
    const size_t nk = (size_t)n * k;
    if (P == 0 || h.arena_blocks == 0 || h.total == 0) {
        std::fill(distances, distances + nk, FLT_MAX);
        std::fill(ids, ids + nk, ~0ull);
        return;
    }
    (void)resident_lists(h);  // (refused before any device work)

    // the scanned order, the queries in it, and the filters' tables
    const MultiFilterPlan plan = multi_filter_plan(filter_of, n, n_filters);
    std::vector<float> qp((size_t)n * h.dim);
    for (uint32_t j = 0; j < n; ++j)
        std::memcpy(qp.data() + (size_t)j * h.dim, queries + (size_t)plan.perm[j] * h.dim, (size_t)h.dim * 4);
    std::vector<const unsigned long long*> allow_tab(n_filters);
    std::vector<const uint32_t*> allowed_tab(n_filters);
    for (uint32_t f = 0; f < n_filters; ++f) {
        allow_tab[f] = filters[f]->allow.p;
        allowed_tab[f] = filters[f]->allowed.p;
    }
    std::vector<float> out_d(nk);  // in the scanned order
    std::vector<uint64_t> out_i(nk);

    hipStream_t s = h.stream;
    DevBuf<const unsigned long long*> d_allow_tab;
    DevBuf<const uint32_t*> d_allowed_tab;
    DevBuf<uint32_t> d_qf, d_gate;
    DevBuf<uint64_t> d_out_i, d_slot_i, d_part_i, d_carry_i;
    ScanGroupBufs grp;
    DevBuf<unsigned long long> d_pairs;
    DevBuf<float> d_q, d_out_d, d_slot_d, d_part_d, d_carry_d;
    vdb_ivf::SearchSlot w;  // the call's own workspace, not one of the ring's
    BatchTimer timer;
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
    d_gate.ensure((size_t)bmax * P);
    d_carry_d.ensure((size_t)P * k);
    HIPCHECK(hipMemsetAsync(d_carry_i.ensure((size_t)P * k), 0xFF, (size_t)P * k * 8, s));
    uint32_t carry_f = kNoCarry;  // the filter the carry belongs to

    for (uint32_t b0 = 0, B = bmax; b0 < n; b0 += B, B = std::min(B, n - b0)) {
        // the handle's own coarse step: padded queries (w.q) and probes (w.probes)
        h.coarse_batch(w, d_q.p + (size_t)b0 * h.dim, B, P, s);
        HIPCHECK(hipGetLastError());
        hipEvent_t* ev = timer.take();
        // the masked exact scan: the pairs gated by their own filter and grouped by list, then one
        // item per (list segment, 4 pairs)
        HIPCHECK(hipEventRecord(ev[0], s));
        vdbk::launch_pair_gate(w.probes.p, d_qf.p + b0, d_allowed_tab.p, B, P, d_gate.p, s);
        HIPCHECK(hipGetLastError());
        vdbk::launch_scan_group_pairs(w.probes.p, B * P, d_gate.p, h.d_count_local.p, h.nlist, segs, vdbk::kFilterGroup,
                                      grp.cursor.p, grp.pair_start.p, grp.item_start.p, grp.inv.p, s);
        HIPCHECK(hipGetLastError());
        vdbk::MultiFilterScanArgs a;
        fill_scan_list_args(a, h, w, grp, B, P, segs);
        a.allow_tab = d_allow_tab.p;
        a.qf = d_qf.p + b0;
        a.k = k;
        a.part_d = segs > 1 ? d_part_d.p : d_slot_d.p;
        a.part_i = segs > 1 ? d_part_i.p : d_slot_i.p;
        vdbk::launch_filter_scan_multi(h.metric, a, s);
        HIPCHECK(hipGetLastError());
        if (segs > 1) {
            vdbk::launch_filter_fold_multi(d_part_d.p, d_part_i.p, w.probes.p, d_gate.p, h.d_count_local.p, B * P, segs,
                                           k, d_slot_d.p, d_slot_i.p, s);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipEventRecord(ev[1], s));
        // the merge; the carry crosses the batches inside a filter, so results never depend on `batch`
        const int carry_same = carry_f == plan.qf[b0] ? 1 : 0;
        vdbk::launch_filter_merge_multi(d_gate.p, d_qf.p + b0, d_slot_d.p, d_slot_i.p, d_carry_d.p, d_carry_i.p,
                                        carry_same, B, P, k, h.stale, d_out_d.p + (size_t)b0 * k,
                                        d_out_i.p + (size_t)b0 * k, d_pairs.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[2], s));
        carry_f = plan.qf[b0 + B - 1];
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
    timer.finish();
    g_filter_timing.scan_ms = timer.scan_ms;
    g_filter_timing.merge_ms = timer.merge_ms;
    g_filter_timing.pairs_scanned = pairs;
}

}  // namespace vdbe
