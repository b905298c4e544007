// exhaustive_screen.cpp — vdb_ivf_search_exhaustive_screened on one handle:
// vdb_ivf_search_exhaustive's result, bit for bit, reading the screen's shadow instead of every
// fp32 row.
//
// While the handle holds a live screen (exhaustive_screen_route.hpp), per tile of 32 queries:
//   1. launch_screen_pairs, the screened search's own kernel, with an identity probe table (every
//      (query, list) is a pair) into the call's own workspace;
//   2. ivf_exh_screen_thresh and ivf_exhaustive_merge: per query T_q, the k-th smallest upper
//      bound over distinct ids of every stored row;
//   3. ivf_exh_screen_bound: every stored row with !(lb > T_q) into the query's region of the
//      candidate buffer. k distinct ids have d <= ub <= T_q and a discarded row has
//      d >= lb > T_q, so no discarded row is among the first k distinct ids by (d, id);
//   4. ivf_exh_screen_select: the exact unique top-k of the query's candidates, from screen_rows.
// One upload, one download and one synchronisation per call. A tile in which a query kept more
// candidates than its region holds is then served by search_exhaustive (its select wrote
// nothing); without a live screen the whole call is search_exhaustive.
//
// A free function over vdb_ivf's public members, as exhaustive.cpp is. It calls nothing that
// changes the handle: no screen_update, screen_release, ensure_arena or upload_directory.
#include "exhaustive_screen.hpp"

#include <algorithm>
#include <vector>

#include "exact_call.hpp"
#include "exhaustive.hpp"
#include "exhaustive_kernels.hpp"
#include "exhaustive_screen_kernels.hpp"
#include "exhaustive_screen_route.hpp"
#include "unit_kernels.hpp"

namespace vdbe {

thread_local ExhScreenTiming g_exh_screen_timing;

namespace {

static_assert(kExhScreenTile == vdbk::kExsTile && kExhScreenMaxK == vdbk::kExsMaxK, "the route sizes the kernels' tile");

// Five events around the four steps of every tile, summed: a small ring, an entry read (after
// waiting for it) when its turn comes again.
struct StepTimer {
    static constexpr int kRing = 8, kEv = 5;
    hipEvent_t e[kRing][kEv] = {};
    bool live[kRing] = {};
    int next = 0;
    double ms[kEv - 1] = {};
    StepTimer() {
        for (auto& q : e)
            for (auto& x : q) HIPCHECK(hipEventCreate(&x));
    }
    ~StepTimer() {
        for (auto& q : e)
            for (auto& x : q)
                if (x) (void)hipEventDestroy(x);
    }
    void drain(int i) {
        if (!live[i]) return;
        HIPCHECK(hipEventSynchronize(e[i][kEv - 1]));
        for (int j = 0; j + 1 < kEv; ++j) {
            float t = 0.f;
            HIPCHECK(hipEventElapsedTime(&t, e[i][j], e[i][j + 1]));
            ms[j] += t;
        }
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

void search_exhaustive_screened(vdb_ivf& h, const float* queries, uint32_t n, uint32_t k, uint64_t reserve,
                                float* distances, uint64_t* ids) {
    // search_exhaustive's refusals, in its order
    require(k <= (uint32_t)vdbk::kMaxK, "k above 1024 is not supported", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, "search_exhaustive_screened");
    g_exh_screen_timing = ExhScreenTiming{};
    if (n == 0) return;

    ExhScreenFacts rf;
    rf.screen_ready = h.screen_ready;
    rf.screen_stale = h.screen_stale;
    rf.buffers = h.screen_rows.p != nullptr && h.screen_sh.p != nullptr && h.screen_meta.p != nullptr &&
                 h.screen_blist.p != nullptr && (!h.screen_fmt_i8 || h.screen_scale.p != nullptr);
    rf.metric = h.config_metric();
    rf.dp = h.dp;
    rf.i8 = h.screen_fmt_i8;
    rf.slots = h.arena_blocks * 64;
    const bool empty = h.arena_blocks == 0 || h.total == 0;
    if (empty || !exh_screen_serves(rf, k)) {
        search_exhaustive(h, queries, n, k, distances, ids);
        const uint32_t xt = vdbk::exhaustive_sizing(k).tile;
        g_exh_screen_timing.exact_tiles = (n + xt - 1) / xt;
        return;
    }
    require(h.arena_ids.p != nullptr && h.cent_rm.p != nullptr, "the handle holds no ids or centroids", VDB_ERR_STATE);

    hipStream_t s = h.stream;
    const uint64_t nb = h.arena_blocks;
    const uint32_t T = exh_screen_tile(h.nlist, h.dp, rf.i8);
    const uint64_t cap = exh_cand_cap(reserve, k);
    const size_t nk = (size_t)n * k, bp = (size_t)T * h.nlist;
    // the threshold pass: one workgroup per CU (its lists and tile take 128 KiB of LDS); the bound
    // pass: two. A wave takes about an eighth of its share of the blocks at a time.
    const uint64_t wg = (nb + vdbk::kExsWaves - 1) / vdbk::kExsWaves;
    const uint32_t grid_t = (uint32_t)std::min<uint64_t>(vdbk::kPersistentBlocks / 2, wg);
    const uint32_t grid_b = (uint32_t)std::min<uint64_t>(vdbk::kPersistentBlocks, wg);
    const uint32_t chunk_t = (uint32_t)std::clamp<uint64_t>(nb / ((uint64_t)grid_t * vdbk::kExsWaves * 8), 1, 32);
    const uint32_t chunk_b = (uint32_t)std::clamp<uint64_t>(nb / ((uint64_t)grid_b * vdbk::kExsWaves * 8), 1, 32);

    DevBuf<uint8_t> d_valid;
    DevBuf<float> d_q, d_qpad, d_qscale, d_part_d, d_thr_d, d_out_d;
    DevBuf<uint64_t> d_part_i, d_thr_i, d_out_i;
    DevBuf<uint16_t> d_qres;
    DevBuf<float4> d_pst;
    DevBuf<uint32_t> d_probes, d_thr4, d_scnt, d_ovf, d_ubcnt, d_counters, d_shared, d_cnt, d_cand;
    DevBuf<unsigned long long> d_ctrl;
    std::vector<uint32_t> cnt(n);
    unsigned long long ctrl[vdbk::kExsCtrlWords] = {};
    StepTimer timer;
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

    // 1. the queries up, padded (unit: normalised) rows [n][dp]; the valid rows of every block
    HIPCHECK(hipMemcpyAsync(d_q.ensure((size_t)n * h.dim), queries, (size_t)n * h.dim * 4, hipMemcpyHostToDevice, s));
    const float* qrows = d_q.p;
    if (h.unit_rows) {
        vdbk::launch_unit_rows(d_q.p, n, h.dim, h.dp, d_qpad.ensure((size_t)n * h.dp), s);
        qrows = d_qpad.p;
    } else if (h.dim != h.dp) {
        vdbk::launch_pad_rows(d_q.p, n, h.dim, h.dp, d_qpad.ensure((size_t)n * h.dp), s);
        qrows = d_qpad.p;
    }
    HIPCHECK(hipGetLastError());
    vdbk::launch_exh_block_valid(h.d_block_off.p, h.d_count_local.p, h.nlist, nb, d_valid.ensure(nb), s);
    HIPCHECK(hipGetLastError());

    // 2. the workspace, once per call
    vdbk::launch_exs_probes(d_probes.ensure(bp), T, h.nlist, s);
    HIPCHECK(hipGetLastError());
    d_qres.ensure(exh_pairs_bytes(T, h.nlist, h.dp, rf.i8) / 2);
    d_pst.ensure(bp);
    d_qscale.ensure(bp);
    d_thr4.ensure(4 * bp);
    // (what the pairs kernel resets for the deferred search: the int8 one writes them unguarded)
    d_scnt.ensure(bp);
    d_ovf.ensure(bp);
    d_ubcnt.ensure(bp);
    d_counters.ensure(vdbk::kCounters);
    d_shared.ensure(vdbk::kExsTile);
    d_cnt.ensure(n);
    d_cand.ensure((size_t)T * cap);
    d_part_d.ensure((size_t)grid_t * vdbk::kExsTile * k);
    d_part_i.ensure((size_t)grid_t * vdbk::kExsTile * k);
    d_thr_d.ensure((size_t)vdbk::kExsTile * k);
    d_thr_i.ensure((size_t)vdbk::kExsTile * k);
    d_out_d.ensure(nk);
    d_out_i.ensure(nk);
    HIPCHECK(hipMemsetAsync(d_ctrl.ensure(vdbk::kExsCtrlWords), 0, sizeof(ctrl), s));

    // 3. per tile: pairs, thresholds, bound, select
    for (uint32_t q0 = 0; q0 < n; q0 += T) {
        const uint32_t nq = std::min(T, n - q0);
        vdbk::launch_exs_stage(d_ctrl.p, d_shared.p, d_cnt.p + q0, nq, s);
        HIPCHECK(hipGetLastError());
        hipEvent_t* ev = timer.take();
        HIPCHECK(hipEventRecord(ev[0], s));
        vdbk::launch_screen_pairs(h.metric, qrows + (size_t)q0 * h.dp, nq, h.nlist, d_probes.p, h.cent_rm.p, h.dp,
                                  d_qres.p, d_pst.p, d_thr4.p, s, d_scnt.p, d_ovf.p, d_counters.p, d_ubcnt.p,
                                  rf.i8 ? d_qscale.p : nullptr);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[1], s));
        vdbk::ExhScreenArgs a;
        a.shadow = h.screen_sh.p;
        a.meta = h.screen_meta.p;
        a.sscale = rf.i8 ? h.screen_scale.p : nullptr;
        a.blist = h.screen_blist.p;
        a.valid = d_valid.p;
        a.ids = h.arena_ids.p;
        a.qres = d_qres.p;
        a.pst = d_pst.p;
        a.qscale = rf.i8 ? d_qscale.p : nullptr;
        a.nb = nb;
        a.nlist = h.nlist;
        a.dp = h.dp;
        a.k = k;
        a.nq = nq;
        a.ctrl = d_ctrl.p;
        a.shared_thr = d_shared.p;
        a.part_d = d_part_d.p;
        a.part_i = d_part_i.p;
        a.thr = d_thr_d.p;
        a.cand = d_cand.p;
        a.cnt = d_cnt.p + q0;
        a.cap = cap;
        a.chunk = chunk_t;
        a.lds = (uint32_t)vdbk::kExsThreshLds;
        vdbk::launch_exs_thresh(h.metric, a, grid_t, s);
        HIPCHECK(hipGetLastError());
        vdbk::launch_exh_merge(d_part_d.p, d_part_i.p, grid_t, vdbk::kExsTile, nq, k, d_thr_d.p, d_thr_i.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[2], s));
        a.chunk = chunk_b;
        a.lds = (uint32_t)vdbk::kExsTileLds;
        vdbk::launch_exs_bound(h.metric, a, grid_b, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[3], s));
        vdbk::ExhSelectArgs r;
        r.cand = d_cand.p;
        r.cnt = d_cnt.p + q0;
        r.cap = cap;
        r.rows = (const float4*)h.screen_rows.p;
        r.ids = h.arena_ids.p;
        r.q = qrows + (size_t)q0 * h.dp;
        r.d4 = h.d4;
        r.k = k;
        r.nq = nq;
        r.out_d = d_out_d.p + (size_t)q0 * k;
        r.out_i = d_out_i.p + (size_t)q0 * k;
        vdbk::launch_exs_select(h.metric, r, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[4], s));
    }
    h.cos_finish(d_out_d.p, d_out_i.p, nk, s);  // (CosineDistance: the lists are ordered by -dot)
    HIPCHECK(hipMemcpyAsync(distances, d_out_d.p, nk * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ids, d_out_i.p, nk * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctrl, d_ctrl.p, sizeof(ctrl), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    timer.finish();
    ExhScreenTiming t;
    t.pairs_ms = timer.ms[0];
    t.thresh_ms = timer.ms[1];
    t.bound_ms = timer.ms[2];
    t.select_ms = timer.ms[3];
    t.rows_bounded = ctrl[vdbk::kExsRows];
    // 4. a tile in which a query's bound kept more than its region holds: the exact scan's
    for (uint32_t q0 = 0; q0 < n; q0 += T) {
        const uint32_t nq = std::min(T, n - q0);
        bool over = false;
        for (uint32_t g = 0; g < nq; ++g) {
            t.candidates += cnt[q0 + g];
            over |= exh_falls_back(cnt[q0 + g], cap);
        }
        if (!over) {
            ++t.screened_tiles;
            continue;
        }
        ++t.exact_tiles;
        search_exhaustive(h, queries + (size_t)q0 * h.dim, nq, k, distances + (size_t)q0 * k, ids + (size_t)q0 * k);
    }
    g_exh_screen_timing = t;
}

}  // namespace vdbe
