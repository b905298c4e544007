// scan_route.hpp — how a batch is scanned: host arithmetic only (no HIP), so the CPU tests
// check every decision on worked examples (tests/cpp/scan_route_test.cpp).
//
// The engine (engine.hpp) copies its options into ScanKnobs and the state of the handle into
// ScanFacts, asks the kernels' own fit tests (kernels.hpp) once per batch for ScanFits, and
// reads back plain structs:
//   * scan_directory: the segment size, the per-list counts and segment counts, the prefix of
//     the largest segment counts and the screened items' length, from the lists' sizes;
//   * batch_cap: queries per internal batch;
//   * scan_bounds: the item counts that size a slot's buffers AND the batch's launches;
//   * screen_width, floor_applies, scan_route: everything scan_batch decides before it
//     launches. The run-time floor (floor.hpp) is stateful and stays with the engine: it is
//     asked between screen_width and scan_route, exactly when floor_applies says so, and its
//     verdict is an input of the route.
// The constants of kernels.hpp the arithmetic needs come in as ScanConsts (kernels.hpp pulls
// in the HIP runtime; their values are written there only).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace vdbe {

struct ScanConsts {
    uint32_t merge_fan;          // vdbk::kMergeFan
    uint32_t plan_max_pairs;     // vdbk::kPlanMaxPairs
    uint32_t persistent_blocks;  // vdbk::kPersistentBlocks
    int diag;                    // VDB_SCAN_DIAG
};

// The options that shape a scan (engine.hpp documents each beside its member).
struct ScanKnobs {
    bool wide_scan;
    uint32_t wide_group;
    bool fused_scan;
    uint32_t scan_mfma_min, scan_blocks, segs_item_opt, narrow_blocks;
    uint32_t screen_group;
    bool screen_defer;
    int screen_i8;
    bool screen_recheck2;
    uint32_t screen_thr_every, screen_cand_cap;
    uint32_t tier_cand_cap;  // (grown by the tier's overflow re-runs)
};

// What the handle is at the moment of the batch.
struct ScanFacts {
    int metric;  // 0 L2, 1 IP, 2 Cosine
    uint32_t seg_blocks, screen_segs_auto;
    bool screen_ready, screen_fmt_i8, i8_vetoed, arena_dropped;
    bool tiered, file_home, force_exact, calibrating;
};

// The kernels' answers for this k (and the handle's dimension): vdbk::topk_regs,
// scan_wide_fits at 4 and 8 waves, scan_bounded_fits, scan_screen_fits at 16- and 32-query
// items (for the screen_defer in force).
struct ScanFits {
    int regs_k;
    bool wide4, wide8, bounded, screen16, screen32;
};

// ---- the list directory (upload_directory) ----
struct ScanDirectory {
    bool ok = true;  // false: a list of 2^32 vectors or more (nothing below is meaningful)
    uint32_t seg_blocks = 8;
    std::vector<uint32_t> count_local, count_global, nseg;  // per list
    uint64_t storable_n = 0;                                // non-empty lists stored here
    std::vector<uint64_t> nseg_prefix;                      // sum of the j largest local segment counts
    uint32_t screen_segs_auto = 4;
};

inline ScanDirectory scan_directory(const std::vector<uint64_t>& count, const std::vector<uint8_t>& owned,
                                    uint32_t seg_blocks_opt, bool screen_opt, int metric) {
    ScanDirectory d;
    const size_t nlist = count.size();
    // Segment size: the largest of 512/256/128/64 vectors that still cuts this
    // handle's lists into >= 4096 segments, so a shard of an 8-GPU node keeps
    // enough scan work items for load balance (measured on a 1/8 shard of the
    // 10M x 768 index: 256 beats 512 by 5 % and 64 by 9 %).
    uint64_t local = 0;
    for (size_t l = 0; l < nlist; ++l) local += owned[l] ? count[l] : 0;
    if (seg_blocks_opt) {
        d.seg_blocks = seg_blocks_opt;
    } else {
        d.seg_blocks = 8;  // 512 vectors at most by default (1024 is an explicit option)
        // (The screen keeps 512 at every shard size. 256-vector segments in items of 4 made
        // the 1/8 shard's one-in-flight scan faster (0.549 vs 0.575 ms) but its batches at
        // 3 in flight slower (0.47 vs 0.41 ms per step over the 8 emulated ranks: more
        // items, partials and merge work per batch), so throughput keeps 512.)
        const bool screen_may = screen_opt && metric != 2;
        while (!screen_may && d.seg_blocks > 1 && local / ((uint64_t)d.seg_blocks * 64) < 4096) d.seg_blocks >>= 1;
    }
    const uint64_t seg = (uint64_t)d.seg_blocks * 64;
    d.count_local.resize(nlist);
    d.count_global.resize(nlist);
    d.nseg.resize(nlist);
    for (size_t l = 0; l < nlist; ++l) {
        if (count[l] >= (1ull << 32)) {
            d.ok = false;
            return d;
        }
        d.count_global[l] = (uint32_t)count[l];
        d.count_local[l] = owned[l] ? (uint32_t)count[l] : 0u;
        d.storable_n += d.count_local[l] > 0;
        d.nseg[l] = (uint32_t)((d.count_local[l] + seg - 1) / seg);
    }
    // Screened items: a wave carries its top-k across the segments it takes from one item,
    // so items of long lists take more segments (its thresholds tighten over more
    // vectors); short lists keep 4 for parallelism. By the size-weighted mean segment
    // count of the stored lists (measured: iid 10M x 768, 40 per list: 8; the 1/8 shard
    // of 100M x 768, ~200: 16; the mixture, 5: 4).
    double wsum = 0.0, wseg = 0.0;
    for (size_t l = 0; l < nlist; ++l) {
        wsum += d.count_local[l];
        wseg += (double)d.count_local[l] * d.nseg[l];
    }
    const double mean_seg = wsum > 0 ? wseg / wsum : 0.0;
    d.screen_segs_auto = mean_seg < 16.0 ? 4u : (mean_seg < 96.0 ? 8u : 16u);
    std::vector<uint32_t> sorted(d.nseg);
    std::sort(sorted.begin(), sorted.end(), std::greater<uint32_t>());
    d.nseg_prefix.assign(nlist + 1, 0);
    for (size_t j = 0; j < nlist; ++j) d.nseg_prefix[j + 1] = d.nseg_prefix[j] + sorted[j];
    return d;
}

// ---- batch size and bounds ----
// Queries per internal batch: the option `batch`, bounded so that batch x nprobe fits the
// plan kernel (8192 pairs) and so that one slot's per-segment partials (B x the segments
// of the P largest lists x k x 12 bytes) stay within kPartialBytes: the exact path at
// k = 1000 on the 10M x 768 index would otherwise hold 1.5 GB of partials per slot.
// Results never depend on batch boundaries.
constexpr uint64_t kPartialBytes = 384ull << 20;
inline uint32_t batch_cap(const ScanConsts& c, uint32_t batch, const std::vector<uint64_t>& nseg_prefix, uint32_t P,
                          uint32_t k) {
    uint32_t b = std::max<uint32_t>(1, std::min<uint32_t>(batch, c.plan_max_pairs / P));
    const uint64_t per_query = (P < nseg_prefix.size() ? nseg_prefix[P] : 0) * (uint64_t)k * 12;
    if (per_query) b = std::max<uint32_t>(1, (uint32_t)std::min<uint64_t>(b, kPartialBytes / per_query));
    return b;
}

// The most a batch of B queries at nprobe P can need: (query, probe) pairs, scan items (one
// per pair and segment of the P largest lists), level-1 merge items and wide items. They size
// the slot's buffers (ensure_workspace) and the batch's launches (scan_batch) alike.
struct ScanBounds {
    uint64_t BP, max_items, max_l1, max_wide;
    bool ok() const { return max_items < (1ull << 32); }  // (item indices are 32-bit)
    // workgroups that leave no wide item and no group of 4 narrow items waiting
    uint64_t want() const { return std::max<uint64_t>(max_wide, (max_items + 3) / 4); }
};

inline ScanBounds scan_bounds(const ScanConsts& c, const std::vector<uint64_t>& nseg_prefix, uint32_t B, uint32_t P) {
    ScanBounds b;
    b.BP = (uint64_t)B * P;
    b.max_items = (uint64_t)B * nseg_prefix[P];
    b.max_l1 = b.max_items / c.merge_fan + b.BP;
    b.max_wide = b.max_items / 4 + b.BP + 1;
    return b;
}

// ---- the screen ----
// The deferred screen's shadow format (option screen_i8; engine.hpp): int8 or bf16.
inline bool want_i8(const ScanKnobs& kn, const ScanFacts& f) {
    if (!kn.screen_defer) return false;
    if (kn.screen_i8 != 2) return kn.screen_i8 == 1;
    return !f.tiered && !f.i8_vetoed;
}

// The screened scan's item width for a search (16 or 32 queries), or 0 when the screen
// does not serve it. ONE decision for scan_batch and for the tier's routing
// (screen_serves): a search the tier sends past its list cache is always screened.
// 32-query items (option screen_group; 0 = automatic: 32 from nprobe 64 up, where hub
// lists are probed by many queries of a batch: cfg4 shard collect 4.45 vs 4.69 ms; 16
// below: cfg3 2.54 vs 2.72 ms): the deferred kernel feeds each shadow tile to two A
// operands (its LDS is static: any k <= 64); the inline kernel splits its waves in two
// halves where the item's lists fit its LDS, else it runs 16-query items.
inline uint32_t screen_width(const ScanKnobs& kn, const ScanFacts& f, const ScanFits& fit, uint32_t P) {
    if (!f.screen_ready || f.metric == 2 || fit.regs_k != 1) return 0;
    if (f.tiered && !kn.screen_defer) return 0;           // (the tier's screen is the deferred one)
    if (!kn.screen_defer && f.screen_fmt_i8) return 0;    // (the inline kernel reads a bf16 shadow)
    const uint32_t want = kn.screen_group ? kn.screen_group : (kn.screen_defer && P >= 64 ? 32u : 16u);
    if (want == 32 && fit.screen32) return 32;
    return fit.screen16 ? 16 : 0;
}

// The run-time floor (floor.hpp) is asked about a batch the screen would serve, lists in HBM,
// deferred scan, and never about the calibration batch; its verdict goes into scan_route.
inline bool floor_applies(const ScanKnobs& kn, const ScanFacts& f, uint32_t swq) {
    return swq != 0 && !f.force_exact && !f.tiered && kn.screen_defer && !f.calibrating;
}

// ---- the route ----
enum class ScanShape {
    ScreenDeferred,  // collect, select, exact re-check of the survivors
    ScreenInline,    // one screened kernel that re-checks as candidates appear
    FusedWide,       // one persistent grid takes the wide and the narrow queue
    WideSide,        // wide items on the stream, narrow items on the slot's side stream
    Narrow,          // narrow items only
};

// The persistent collect grid of 16-query items: 320 workgroups, 1.25 per CU, not 2:
// the CU slots left over run the other batches in flight; measured on one box,
// 320 / 352 / 384 / 512: headline 28.5K / 28.2K / 28.1K / 27.4K QPS, mixture 53.6K /
// 53.9K / 54.0K / 52.0K, 1/8 shard at 3 in flight 184.5K / 182.7K / 181.8K / 174.4K.
constexpr uint32_t kCollectBlocks = 320;

struct ScanRoute {
    ScanShape shape;
    bool screened;        // the screened scan serves the batch
    uint32_t swq;         // ... in items of this many queries (screen_width)
    bool rows_l;          // the exact scan reads the row-major copy (ScanArgs::rows_layout)
    bool need_arena;      // ensure_arena() first: the bounded scan needs the interleaved layout
    int waves;            // workgroup shape of the wide scan (4 or 8)
    bool wide;            // wide items are planned
    uint32_t segs_item;   // segments per exact wide item
    uint32_t segs_screen; // segments per screened item
    uint32_t mfma_min;    // wide items of this many queries run the bounded scan (0: none)
    int plan_wide;        // queries per wide item the plan kernel forms (0: narrow items only)
    // screened:
    bool i8s;             // the collect reads an int8 shadow
    bool tier_file;       // the survivors' rows come from the tier's file home
    bool recheck2, tier2; // the two-pass re-check: rows in HBM / rows from the file
    uint32_t thr_every;   // blocks between re-reads of the shared thresholds
    uint32_t ccap;        // candidate capacity (the tier's overflow re-runs grow it)
    // grids (workgroups) and ScanArgs::fused (workgroups that start on the narrow queue):
    uint32_t fused;
    uint32_t grid_collect, grid_wide, grid_narrow;

    uint32_t segs() const { return screened ? segs_screen : segs_item; }  // (what the plan kernel cuts by)
};

// `swq`: screen_width of the search; `floor_ok`: the floor's verdict (true where
// floor_applies is false). No allocation: once per batch.
inline ScanRoute scan_route(const ScanConsts& c, const ScanKnobs& kn, const ScanFacts& f, const ScanFits& fit,
                            const ScanBounds& b, uint32_t swq, bool floor_ok) {
    ScanRoute r{};
    r.swq = swq;
    r.screened = swq != 0 && !f.force_exact && floor_ok;
    const bool wide_ok = fit.regs_k == 1 && kn.wide_scan && f.metric != 2;
    // Exact scans on lists in HBM whose interleaved arena was released read the row-major
    // copy (4-wave items); the opt-in bounded scan needs the interleaved layout back.
    r.rows_l = !r.screened && f.arena_dropped && !f.tiered;
    r.need_arena = r.rows_l && kn.scan_mfma_min && wide_ok;
    if (r.need_arena) r.rows_l = false;
    r.waves = kn.wide_group == 32 && !r.rows_l ? 8 : 4;
    // (Cosine: every CPU-path distance is 0.0f, A5; its lists scan as narrow items only)
    r.wide = wide_ok && (r.waves == 8 ? fit.wide8 : fit.wide4);
    // segments per item: one per wave (more adds tail latency, no throughput)
    r.segs_item = kn.segs_item_opt ? kn.segs_item_opt : (uint32_t)r.waves;
    // wide items of many queries: bounded on the matrix cores (L2 / IP, 16-query items)
    r.mfma_min = !r.screened && !r.rows_l && r.wide && r.waves == 4 && !(c.diag & 2) && fit.bounded ? kn.scan_mfma_min : 0u;
    r.plan_wide = r.screened ? (int)swq : (r.wide ? 4 * r.waves : 0);
    // (screened items: segs_per_item segments, default 4; a wave's top-k carries across
    // the segments it takes from one item)
    r.segs_screen = kn.segs_item_opt ? kn.segs_item_opt : f.screen_segs_auto;
    const uint32_t quads = (uint32_t)((b.max_items + 3) / 4);  // (narrow items run 4 to a workgroup)
    if (r.screened) {
        r.shape = kn.screen_defer ? ScanShape::ScreenDeferred : ScanShape::ScreenInline;
        r.i8s = kn.screen_defer && f.screen_fmt_i8;  // (int8 shadow: built only for the deferred scan)
        // (the tier's file home reads the survivors' rows on the host: the batch then
        // waits for its selection, and re-runs with a larger buffer if it overflowed)
        r.tier_file = f.tiered && f.file_home;
        r.recheck2 = kn.screen_recheck2 && !f.tiered;  // (rows in HBM, by slot)
        r.tier2 = kn.screen_recheck2 && r.tier_file;   // (rows from the file, two read phases)
        // candidates at most: every (query, vector) pair the batch can have (B queries x the
        // P largest stored lists), capped by the option
        r.ccap = (uint32_t)std::min<uint64_t>(kn.screen_cand_cap,
                                              std::max<uint64_t>(1024, b.max_items * f.seg_blocks * 64));
        if (r.tier_file) r.ccap = std::max(r.ccap, kn.tier_cand_cap);
        // (32-query items run one workgroup per CU, so a shared-threshold read's latency is
        // exposed: re-read every 4 blocks, cfg4 shard collect 4.14 -> 3.87 ms; 16-query
        // items hide it and keep the freshest value, 1/8 shard 0.543 vs 0.552 ms)
        r.thr_every = kn.screen_thr_every ? kn.screen_thr_every : (swq == 32 ? 4u : 1u);
        r.fused = std::max<uint32_t>(1, std::min<uint32_t>(kn.narrow_blocks, c.persistent_blocks / 2));
        const uint64_t cap = kn.scan_blocks ? kn.scan_blocks : (swq == 32 ? c.persistent_blocks / 2 : kCollectBlocks);
        r.grid_collect = (uint32_t)std::min<uint64_t>(b.want(), cap);
    } else if (r.wide && kn.fused_scan) {
        // one persistent grid takes both queues (no side stream, no fork/join)
        // (narrow_blocks counts 4-wave workgroups: as many waves start on the narrow queue)
        r.shape = ScanShape::FusedWide;
        const uint32_t grid_cap = r.waves == 8 ? c.persistent_blocks / 2 : c.persistent_blocks;
        r.fused = std::max<uint32_t>(1, std::min<uint32_t>(kn.narrow_blocks * 4 / r.waves, grid_cap / 2));
        r.grid_wide = (uint32_t)(kn.scan_blocks ? std::min<uint64_t>(b.want(), kn.scan_blocks) : b.want());
    } else if (r.wide) {
        // narrow items on the side stream fill the CUs the wide items leave idle
        r.shape = ScanShape::WideSide;
        r.grid_narrow = std::min<uint32_t>(quads, kn.narrow_blocks);
        r.grid_wide = (uint32_t)b.max_wide;
    } else {
        r.shape = ScanShape::Narrow;
        r.grid_narrow = quads;
    }
    return r;
}

}  // namespace vdbe
