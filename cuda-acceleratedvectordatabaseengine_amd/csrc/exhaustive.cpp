// exhaustive.cpp — vdb_ivf_search_exhaustive on one handle: the exact top-k over every stored
// row, one pass over the rows per tile of queries.
//
// Nothing moves and nothing is rebuilt. Per call: the per-block valid counts from the list
// directory (ivf_exh_valid_*), the queries padded (or, CosineDistance, normalised) once; then
// per tile of exhaustive_sizing(k).tile queries the stage (dimension-major queries, cursor
// reset), the scan (ivf_exhaustive_scan: a persistent grid over the arena's blocks in storage
// order) and the merge of the workgroups' partials (ivf_exhaustive_merge). The rows are read in
// the fp32 layout the handle holds at that moment: the interleaved arena, or the screen's
// row-major copy while the arena is dropped. No coarse step, no pair plan, no slots: centroids,
// list boundaries, `batch` and `stale_slots` never enter.
//
// A free function over vdb_ivf's public members, as filter.cpp is and for the same reason; what
// it shares with the other exact calls (the refusals, the layout choice, the fence) is
// exact_call.hpp.
#include "exhaustive.hpp"

#include <algorithm>
#include <cfloat>

#include "exact_call.hpp"
#include "exhaustive_kernels.hpp"
#include "unit_kernels.hpp"

namespace vdbe {

thread_local ExhaustiveTiming g_exhaustive_timing;

namespace {

// Event triples around the scan and the merge of every tile, summed: a small ring, an entry
// read (after waiting for it) when its turn comes again.
struct TileTimer {
    static constexpr int kRing = 16;
    hipEvent_t e[kRing][3] = {};  // scan begin, scan end = merge begin, merge end
    bool live[kRing] = {};
    int next = 0;
    double scan_ms = 0.0, merge_ms = 0.0;
    TileTimer() {
        for (auto& q : e)
            for (auto& x : q) HIPCHECK(hipEventCreate(&x));
    }
    ~TileTimer() {
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

void search_exhaustive(vdb_ivf& h, const float* queries, uint32_t n, uint32_t k, float* distances, uint64_t* ids) {
    require(k <= (uint32_t)vdbk::kMaxK, "k above 1024 is not supported", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, "search_exhaustive");
    g_exhaustive_timing = ExhaustiveTiming{};
    if (n == 0) return;
    const size_t nk = (size_t)n * k;
    if (h.arena_blocks == 0 || h.total == 0) {  // an empty index: every slot unfilled
        std::fill(distances, distances + nk, FLT_MAX);
        std::fill(ids, ids + nk, ~0ull);
        return;
    }
    const float4* lists = resident_lists(h);  // (refused before any device work)

    hipStream_t s = h.stream;
    const uint64_t nb = h.arena_blocks;
    const vdbk::ExhSizing z = vdbk::exhaustive_sizing(k);
    // One workgroup per CU (the lists take 96 KiB of its LDS), fewer where the arena has fewer
    // blocks than the grid has waves. A wave takes about an eighth of its share at a time.
    const uint32_t grid =
        (uint32_t)std::min<uint64_t>(vdbk::kPersistentBlocks / 2, (nb + vdbk::kExhWaves - 1) / vdbk::kExhWaves);
    const uint32_t chunk = (uint32_t)std::clamp<uint64_t>(nb / ((uint64_t)grid * vdbk::kExhWaves * 8), 1, 32);

    DevBuf<uint8_t> d_valid;
    DevBuf<float> d_q, d_qpad, d_qt, d_out_d, d_part_d;
    DevBuf<uint64_t> d_out_i, d_part_i;
    DevBuf<unsigned long long> d_cursor;
    TileTimer timer;
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

    // 2. the workspace, once per (tile, k): a k = 1024 call's partials are 256 x 2 x 1024 x 12 B
    // = 6 MiB, so the grid stays whole at every k
    d_qt.ensure((size_t)h.dp * z.tile);
    d_cursor.ensure(1);
    d_part_d.ensure((size_t)grid * z.tile * k);
    d_part_i.ensure((size_t)grid * z.tile * k);
    d_out_d.ensure(nk);
    d_out_i.ensure(nk);

    // 3. per tile: stage, scan, merge
    uint64_t tiles = 0;
    for (uint32_t q0 = 0; q0 < n; q0 += z.tile, ++tiles) {
        const uint32_t nq = std::min(z.tile, n - q0);
        vdbk::launch_exh_stage(qrows + (size_t)q0 * h.dp, nq, h.dp, z.tile, d_qt.p, d_cursor.p, s);
        HIPCHECK(hipGetLastError());
        hipEvent_t* ev = timer.take();
        HIPCHECK(hipEventRecord(ev[0], s));
        vdbk::ExhScanArgs a;
        a.lists = lists;
        a.ids = h.arena_ids.p;
        a.valid = d_valid.p;
        a.qt = d_qt.p;
        a.cursor = d_cursor.p;
        a.nb = nb;
        a.d4 = h.d4;
        a.k = k;
        a.nq = nq;
        a.chunk = chunk;
        a.rows = h.arena_dropped ? 1 : 0;
        a.lds = (uint32_t)z.lds;
        a.part_d = d_part_d.p;
        a.part_i = d_part_i.p;
        vdbk::launch_exh_scan(h.metric, a, grid, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[1], s));
        vdbk::launch_exh_merge(d_part_d.p, d_part_i.p, grid, z.tile, nq, k, d_out_d.p + (size_t)q0 * k,
                               d_out_i.p + (size_t)q0 * k, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[2], s));
    }
    h.cos_finish(d_out_d.p, d_out_i.p, nk, s);  // (CosineDistance: the lists are ordered by -dot)
    HIPCHECK(hipMemcpyAsync(distances, d_out_d.p, nk * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ids, d_out_i.p, nk * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    timer.finish();
    g_exhaustive_timing.scan_ms = timer.scan_ms;
    g_exhaustive_timing.merge_ms = timer.merge_ms;
    g_exhaustive_timing.rows_scanned = h.total * tiles;
    g_exhaustive_timing.pairs_computed = h.total * (uint64_t)n;
}

}  // namespace vdbe
