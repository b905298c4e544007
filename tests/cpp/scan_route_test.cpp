// CPU unit test of the scan's routing and sizing (csrc/scan_route.hpp): the item width, the
// cases the screen does not serve, the exact path's layout and workgroup shape, the grids,
// the candidate cap, the shadow format, the batch bounds and cap, and the list directory.
// Every expected value is a literal worked out by hand from the rules the header states.
// Exit status 0 = every check passed. Built and run by tests/test_scan_route.py with g++
// (no GPU).
#include <cstdio>
#include <vector>

#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/scan_route.hpp"

using namespace vdbe;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                                   \
        }                                                                 \
    } while (0)
#define CHECK_EQ(a, b)                                                                                      \
    do {                                                                                                    \
        const long long va = (long long)(a), vb = (long long)(b);                                           \
        if (va != vb) {                                                                                     \
            std::printf("FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, va, vb);          \
            ++failures;                                                                                     \
        }                                                                                                   \
    } while (0)

// merge fan 32, 8192 pairs per plan launch, 512 persistent workgroups, no diagnostics
static const ScanConsts kC{32, 8192, 512, 0};

// the engine's defaults
static ScanKnobs knobs() {
    ScanKnobs kn{};
    kn.wide_scan = true;
    kn.wide_group = 16;
    kn.fused_scan = true;
    kn.scan_mfma_min = 0;
    kn.scan_blocks = 0;
    kn.segs_item_opt = 0;
    kn.narrow_blocks = 64;
    kn.screen_group = 0;
    kn.screen_defer = true;
    kn.screen_i8 = 2;
    kn.screen_recheck2 = true;
    kn.screen_thr_every = 0;
    kn.screen_cand_cap = 4u << 20;
    kn.tier_cand_cap = 0;
    return kn;
}
// an L2 index in HBM whose int8 screen is built (so the arena is released), 512-vector segments
static ScanFacts facts() {
    ScanFacts f{};
    f.metric = 0;
    f.seg_blocks = 8;
    f.screen_segs_auto = 8;
    f.screen_ready = true;
    f.screen_fmt_i8 = true;
    f.arena_dropped = true;
    return f;
}
static ScanFits fits_k10() { return ScanFits{1, true, true, true, true, true}; }
static ScanFits fits_k65() { return ScanFits{2, false, false, false, false, false}; }  // (every fit test refuses k > 64)

// every list `per` segments long: prefix[j] = per * j
static std::vector<uint64_t> prefix(uint64_t per, size_t nlist) {
    std::vector<uint64_t> p(nlist + 1);
    for (size_t j = 0; j <= nlist; ++j) p[j] = per * j;
    return p;
}

// the route the engine computes: width, the floor only where it applies, the route
static ScanRoute route(const ScanKnobs& kn, const ScanFacts& f, const ScanFits& fit, const ScanBounds& b, uint32_t P,
                       bool floor_verdict = true) {
    const uint32_t swq = screen_width(kn, f, fit, P);
    const bool ok = !floor_applies(kn, f, swq) || floor_verdict;
    return scan_route(kC, kn, f, fit, b, swq, ok);
}

static void test_bounds_and_batch_cap() {
    // 64 queries x nprobe 32 on lists of 40 segments: 2048 pairs, 64 * 1280 = 81920 items,
    // 81920 / 32 + 2048 = 4608 level-1 items, 81920 / 4 + 2048 + 1 = 22529 wide items
    const std::vector<uint64_t> p40 = prefix(40, 128);
    ScanBounds b = scan_bounds(kC, p40, 64, 32);
    CHECK_EQ(b.BP, 2048);
    CHECK_EQ(b.max_items, 81920);
    CHECK_EQ(b.max_l1, 4608);
    CHECK_EQ(b.max_wide, 22529);
    CHECK_EQ(b.want(), 22529);
    CHECK(b.ok());
    // odd sizes: 3 queries x nprobe 5, the 5 largest lists hold 37 segments
    std::vector<uint64_t> podd{0, 12, 21, 28, 33, 37, 40};
    b = scan_bounds(kC, podd, 3, 5);
    CHECK_EQ(b.BP, 15);
    CHECK_EQ(b.max_items, 111);
    CHECK_EQ(b.max_l1, 18);    // 111 / 32 = 3, + 15
    CHECK_EQ(b.max_wide, 43);  // 111 / 4 = 27, + 15 + 1
    CHECK_EQ(b.want(), 43);    // (111 + 3) / 4 = 28 < 43
    // item indices are 32-bit: 2^32 items are refused, 2^32 - 1 are not
    std::vector<uint64_t> pbig{0, 65536};
    CHECK(!scan_bounds(kC, pbig, 65536, 1).ok());
    pbig[1] = 65537;
    b = scan_bounds(kC, pbig, 65535, 1);
    CHECK_EQ(b.max_items, 4294967295ll);
    CHECK(b.ok());

    // batch_cap: the option, then 8192 pairs per plan launch
    const std::vector<uint64_t> empty_index(4097, 0);
    CHECK_EQ(batch_cap(kC, 256, empty_index, 32, 10), 256);  // 8192 / 32 = 256
    CHECK_EQ(batch_cap(kC, 256, empty_index, 64, 10), 128);
    CHECK_EQ(batch_cap(kC, 256, empty_index, 1024, 10), 8);
    CHECK_EQ(batch_cap(kC, 64, empty_index, 32, 10), 64);
    CHECK_EQ(batch_cap(kC, 256, empty_index, 3, 10), 256);  // 8192 / 3 = 2730
    // ... then 384 MiB of partials: k 1000 on lists of 40 segments at nprobe 32 is
    // 1280 * 1000 * 12 = 15,360,000 bytes per query; 402,653,184 / 15,360,000 = 26.2
    CHECK_EQ(batch_cap(kC, 256, p40, 32, 1000), 26);
    CHECK_EQ(batch_cap(kC, 16, p40, 32, 1000), 16);
    CHECK_EQ(batch_cap(kC, 256, p40, 32, 10), 256);  // 153,600 bytes per query: 2621 queries
    // a query whose partials alone exceed the cap still gets a batch of one
    CHECK_EQ(batch_cap(kC, 256, prefix(1250, 64), 32, 1000), 1);  // 40000 * 12000 = 480,000,000
    // nprobe beyond the prefix (no directory yet, or an nprobe above nlist): the pair bound only
    CHECK_EQ(batch_cap(kC, 256, prefix(40, 32), 33, 1000), 248);  // 8192 / 33
    CHECK_EQ(batch_cap(kC, 256, std::vector<uint64_t>(), 32, 1000), 256);
}

static void test_item_width() {
    const std::vector<uint64_t> p40 = prefix(40, 128);
    const ScanKnobs kn = knobs();
    const ScanFacts f = facts();
    // nprobe 32, k 10, deferred int8: 16-query items
    ScanRoute r = route(kn, f, fits_k10(), scan_bounds(kC, p40, 64, 32), 32);
    CHECK(r.screened);
    CHECK(r.shape == ScanShape::ScreenDeferred);
    CHECK_EQ(r.swq, 16);
    CHECK_EQ(r.plan_wide, 16);
    CHECK_EQ(r.grid_collect, 320);  // min(22529, 320)
    CHECK_EQ(r.thr_every, 1);
    CHECK_EQ(r.segs_screen, 8);
    CHECK_EQ(r.segs(), 8);
    CHECK_EQ(r.fused, 64);  // min(narrow_blocks 64, 512 / 2)
    CHECK(r.i8s && r.recheck2 && !r.tier2 && !r.tier_file);
    CHECK(!r.rows_l && !r.need_arena);
    CHECK_EQ(r.mfma_min, 0);
    CHECK_EQ(r.ccap, 4194304);  // 81920 items * 512 vectors = 41,943,040, capped by the option
    // a batch smaller than the grid: 1 query, lists of 2 segments: 64 items, 16 + 32 + 1 = 49 wide
    const std::vector<uint64_t> p2 = prefix(2, 128);
    r = route(kn, f, fits_k10(), scan_bounds(kC, p2, 1, 32), 32);
    CHECK_EQ(r.grid_collect, 49);
    CHECK_EQ(r.ccap, 32768);  // 64 * 512
    // nprobe 64: 32-query items; 163840 items, 40960 + 4096 + 1 = 45057 wide
    r = route(kn, f, fits_k10(), scan_bounds(kC, p40, 64, 64), 64);
    CHECK_EQ(r.swq, 32);
    CHECK_EQ(r.plan_wide, 32);
    CHECK_EQ(r.grid_collect, 256);  // min(45057, 512 / 2)
    CHECK_EQ(r.thr_every, 4);
    // screen_group forces the width either way
    ScanKnobs k2 = kn;
    k2.screen_group = 16;
    CHECK_EQ(screen_width(k2, f, fits_k10(), 64), 16);
    k2.screen_group = 32;
    CHECK_EQ(screen_width(k2, f, fits_k10(), 32), 32);
    // ... and 32 falls back to 16 where it does not fit, and to nothing where neither does
    ScanFits fit = fits_k10();
    fit.screen32 = false;
    CHECK_EQ(screen_width(k2, f, fit, 32), 16);
    CHECK_EQ(screen_width(kn, f, fit, 64), 16);
    fit.screen16 = false;
    CHECK_EQ(screen_width(kn, f, fit, 64), 0);
    CHECK_EQ(screen_width(kn, f, fit, 32), 0);
    // scan_blocks and screen_thr_every override the automatic values
    k2 = kn;
    k2.scan_blocks = 100;
    k2.screen_thr_every = 7;
    r = route(k2, f, fits_k10(), scan_bounds(kC, p40, 64, 32), 32);
    CHECK_EQ(r.grid_collect, 100);
    CHECK_EQ(r.thr_every, 7);
    r = route(k2, f, fits_k10(), scan_bounds(kC, p40, 64, 64), 64);
    CHECK_EQ(r.grid_collect, 100);
    CHECK_EQ(r.thr_every, 7);
    r = route(k2, f, fits_k10(), scan_bounds(kC, p2, 1, 32), 32);
    CHECK_EQ(r.grid_collect, 49);  // (never more workgroups than items)
    // segs_per_item overrides both item lengths
    k2 = kn;
    k2.segs_item_opt = 6;
    r = route(k2, f, fits_k10(), scan_bounds(kC, p40, 64, 32), 32);
    CHECK_EQ(r.segs_screen, 6);
    CHECK_EQ(r.segs_item, 6);
    // the inline kernel (screen_defer 0) on a bf16 shadow: 16-query items at any nprobe
    k2 = kn;
    k2.screen_defer = false;
    ScanFacts fb = f;
    fb.screen_fmt_i8 = false;
    r = route(k2, fb, fits_k10(), scan_bounds(kC, p40, 64, 64), 64);
    CHECK(r.screened);
    CHECK(r.shape == ScanShape::ScreenInline);
    CHECK_EQ(r.swq, 16);
    CHECK_EQ(r.grid_collect, 320);
    CHECK(!r.i8s);
    // the tier's screen: bf16 shadow resident, rows at the home
    fb.tiered = true;
    fb.arena_dropped = false;
    r = route(kn, fb, fits_k10(), scan_bounds(kC, p40, 64, 32), 32);
    CHECK(r.screened && !r.tier_file && !r.recheck2 && !r.tier2);  // (host home)
    fb.file_home = true;
    r = route(kn, fb, fits_k10(), scan_bounds(kC, p40, 64, 32), 32);
    CHECK(r.screened && r.tier_file && !r.recheck2 && r.tier2);
    k2 = kn;
    k2.screen_recheck2 = false;
    r = route(k2, fb, fits_k10(), scan_bounds(kC, p40, 64, 32), 32);
    CHECK(r.tier_file && !r.recheck2 && !r.tier2);
    r = route(k2, f, fits_k10(), scan_bounds(kC, p40, 64, 32), 32);
    CHECK(!r.recheck2 && !r.tier2);
}

static void test_not_screened() {
    const std::vector<uint64_t> p40 = prefix(40, 128);
    const ScanBounds b = scan_bounds(kC, p40, 64, 32);
    const ScanKnobs kn = knobs();
    const ScanFacts f = facts();
    // k 65 (two top-k registers), Cosine, and no screen built
    CHECK_EQ(screen_width(kn, f, fits_k65(), 32), 0);
    ScanFits two = fits_k10();
    two.regs_k = 2;
    CHECK_EQ(screen_width(kn, f, two, 32), 0);
    CHECK(!route(kn, f, fits_k65(), b, 32).screened);
    ScanFacts g = f;
    g.metric = 2;
    CHECK_EQ(screen_width(kn, g, fits_k10(), 32), 0);
    CHECK(!route(kn, g, fits_k10(), b, 32).screened);
    g = f;
    g.metric = 1;  // (IP is screened)
    CHECK_EQ(screen_width(kn, g, fits_k10(), 32), 16);
    g = f;
    g.screen_ready = false;
    CHECK_EQ(screen_width(kn, g, fits_k10(), 32), 0);
    CHECK(!route(kn, g, fits_k10(), b, 32).screened);
    // the tier's screen is the deferred one
    ScanKnobs inl = kn;
    inl.screen_defer = false;
    g = f;
    g.tiered = true;
    g.screen_fmt_i8 = false;
    CHECK_EQ(screen_width(inl, g, fits_k10(), 32), 0);
    CHECK(!route(inl, g, fits_k10(), b, 32).screened);
    // the inline kernel reads a bf16 shadow
    CHECK_EQ(screen_width(inl, f, fits_k10(), 32), 0);
    CHECK(!route(inl, f, fits_k10(), b, 32).screened);
    // force_exact: the width is unchanged (the tier's routing reads it), the batch is exact,
    // and the floor is not asked
    g = f;
    g.force_exact = true;
    CHECK_EQ(screen_width(kn, g, fits_k10(), 32), 16);
    CHECK(!floor_applies(kn, g, 16));
    CHECK(!route(kn, g, fits_k10(), b, 32).screened);
    // the floor's verdict
    CHECK(floor_applies(kn, f, 16));
    CHECK(floor_applies(kn, f, 32));
    CHECK(route(kn, f, fits_k10(), b, 32, true).screened);
    ScanRoute r = route(kn, f, fits_k10(), b, 32, false);
    CHECK(!r.screened);
    CHECK(r.rows_l);  // (the arena is released: the exact scan reads the rows)
    CHECK(r.shape == ScanShape::FusedWide);
    // ... which is asked only about a deferred screened batch of lists in HBM, and never
    // about the calibration batch
    CHECK(!floor_applies(kn, f, 0));
    g = f;
    g.tiered = true;
    CHECK(!floor_applies(kn, g, 16));
    CHECK(route(kn, g, fits_k10(), b, 32, false).screened);  // (a verdict nobody asked for is not read)
    g = f;
    g.calibrating = true;
    CHECK(!floor_applies(kn, g, 16));
    CHECK(!floor_applies(inl, f, 16));
}

static void test_exact_path() {
    const std::vector<uint64_t> p40 = prefix(40, 128);
    const ScanBounds b = scan_bounds(kC, p40, 64, 32);  // 81920 items, 22529 wide
    ScanKnobs kn = knobs();
    ScanFacts f = facts();
    f.force_exact = true;  // (k 10 through the exact scan)
    // the arena released: the row-major copy in 4-wave items, even at wide_group 32
    kn.wide_group = 32;
    ScanRoute r = route(kn, f, fits_k10(), b, 32);
    CHECK(!r.screened && r.rows_l && !r.need_arena);
    CHECK_EQ(r.waves, 4);
    CHECK(r.wide);
    CHECK_EQ(r.plan_wide, 16);
    CHECK_EQ(r.segs_item, 4);
    CHECK_EQ(r.segs(), 4);
    CHECK_EQ(r.mfma_min, 0);
    CHECK(r.shape == ScanShape::FusedWide);
    CHECK_EQ(r.fused, 64);          // min(64 * 4 / 4, 512 / 2)
    CHECK_EQ(r.grid_wide, 22529);   // max(22529, 20480)
    // the bounded scan needs the interleaved arena back
    kn = knobs();
    kn.scan_mfma_min = 8;
    r = route(kn, f, fits_k10(), b, 32);
    CHECK(r.need_arena && !r.rows_l);
    CHECK_EQ(r.mfma_min, 8);
    CHECK_EQ(r.waves, 4);
    ScanFits fit = fits_k10();
    fit.bounded = false;
    CHECK_EQ(route(kn, f, fit, b, 32).mfma_min, 0);
    CHECK_EQ(scan_route(ScanConsts{32, 8192, 512, 2}, kn, f, fits_k10(), b, 16, true).mfma_min, 0);  // (diagnostic bit 2)
    kn.wide_group = 32;  // 8-wave items are never bounded (the arena still comes back)
    r = route(kn, f, fits_k10(), b, 32);
    CHECK(r.need_arena && !r.rows_l);
    CHECK_EQ(r.waves, 8);
    CHECK_EQ(r.mfma_min, 0);
    // ... not where no wide item can exist (k 65)
    kn = knobs();
    kn.scan_mfma_min = 8;
    ScanFacts g = facts();
    r = route(kn, g, fits_k65(), b, 32);
    CHECK(r.rows_l && !r.need_arena && !r.wide);
    CHECK(r.shape == ScanShape::Narrow);
    CHECK_EQ(r.plan_wide, 0);
    CHECK_EQ(r.grid_narrow, 20480);  // (81920 + 3) / 4
    // the tier scans its cache, never the rows
    g = f;
    g.tiered = true;
    r = route(kn, g, fits_k10(), b, 32);
    CHECK(!r.rows_l && !r.need_arena);
    CHECK_EQ(r.mfma_min, 8);
    // Cosine: narrow items only
    kn = knobs();
    g = facts();
    g.metric = 2;
    g.screen_ready = false;
    g.arena_dropped = false;
    r = route(kn, g, fits_k10(), b, 32);
    CHECK(!r.screened && !r.wide && !r.rows_l);
    CHECK_EQ(r.plan_wide, 0);
    CHECK(r.shape == ScanShape::Narrow);
    CHECK_EQ(r.grid_narrow, 20480);
    CHECK_EQ(r.fused, 0);
    // wide_group 32 on the interleaved arena: 8-wave items of 32 queries
    kn.wide_group = 32;
    g = facts();
    g.screen_ready = false;
    g.arena_dropped = false;
    r = route(kn, g, fits_k10(), b, 32);
    CHECK_EQ(r.waves, 8);
    CHECK_EQ(r.plan_wide, 32);
    CHECK_EQ(r.segs_item, 8);
    CHECK(r.shape == ScanShape::FusedWide);
    CHECK_EQ(r.fused, 32);  // min(64 * 4 / 8, 256 / 2)
    CHECK_EQ(r.grid_wide, 22529);
    kn.narrow_blocks = 512;
    CHECK_EQ(route(kn, g, fits_k10(), b, 32).fused, 128);  // min(256, 256 / 2)
    kn.narrow_blocks = 0;
    CHECK_EQ(route(kn, g, fits_k10(), b, 32).fused, 1);
    kn.narrow_blocks = 64;
    kn.scan_blocks = 100;
    CHECK_EQ(route(kn, g, fits_k10(), b, 32).grid_wide, 100);
    fit = fits_k10();
    fit.wide8 = false;  // (the 8-wave item does not fit: narrow items; wide4 is not consulted)
    r = route(kn, g, fit, b, 32);
    CHECK(!r.wide);
    CHECK(r.shape == ScanShape::Narrow);
    // fused_scan off: narrow items on the side stream
    kn = knobs();
    kn.fused_scan = false;
    r = route(kn, g, fits_k10(), b, 32);
    CHECK(r.shape == ScanShape::WideSide);
    CHECK_EQ(r.waves, 4);
    CHECK_EQ(r.grid_narrow, 64);  // min(20480, narrow_blocks)
    CHECK_EQ(r.grid_wide, 22529);
    CHECK_EQ(r.fused, 0);
    r = route(kn, g, fits_k10(), scan_bounds(kC, prefix(2, 128), 1, 32), 32);
    CHECK_EQ(r.grid_narrow, 16);  // min((64 + 3) / 4, 64)
    CHECK_EQ(r.grid_wide, 49);
    kn.wide_group = 32;
    r = route(kn, g, fits_k10(), b, 32);
    CHECK(r.shape == ScanShape::WideSide);
    CHECK_EQ(r.waves, 8);
    // wide_scan off
    kn = knobs();
    kn.wide_scan = false;
    r = route(kn, g, fits_k10(), b, 32);
    CHECK(!r.wide);
    CHECK(r.shape == ScanShape::Narrow);
}

static void test_candidate_cap() {
    ScanKnobs kn = knobs();
    ScanFacts f = facts();
    const ScanBounds b = scan_bounds(kC, prefix(40, 128), 64, 32);  // 41,943,040 (query, vector) pairs
    kn.screen_cand_cap = 10000;
    CHECK_EQ(route(kn, f, fits_k10(), b, 32).ccap, 10000);
    // the lower clamp: one query, one list of one 64-vector segment
    kn = knobs();
    f.seg_blocks = 1;
    CHECK_EQ(route(kn, f, fits_k10(), scan_bounds(kC, prefix(1, 4), 1, 1), 1).ccap, 1024);
    CHECK_EQ(route(kn, f, fits_k10(), scan_bounds(kC, prefix(1, 4), 17, 1), 1).ccap, 1088);  // 17 * 64
    // the tier's file home keeps the capacity an overflow grew
    f = facts();
    f.screen_fmt_i8 = false;
    f.arena_dropped = false;
    f.tiered = f.file_home = true;
    kn.tier_cand_cap = 8000000;
    CHECK_EQ(route(kn, f, fits_k10(), b, 32).ccap, 8000000);
    kn.tier_cand_cap = 5000;
    CHECK_EQ(route(kn, f, fits_k10(), b, 32).ccap, 4194304);
    f.file_home = false;  // (host home: rows over PCIe, no re-run)
    kn.tier_cand_cap = 8000000;
    CHECK_EQ(route(kn, f, fits_k10(), b, 32).ccap, 4194304);
}

static void test_want_i8() {
    ScanKnobs kn = knobs();
    ScanFacts f = facts();
    for (int tiered = 0; tiered < 2; ++tiered)
        for (int vetoed = 0; vetoed < 2; ++vetoed) {
            f.tiered = tiered;
            f.i8_vetoed = vetoed;
            kn.screen_i8 = 0;
            CHECK(!want_i8(kn, f));
            kn.screen_i8 = 1;
            CHECK(want_i8(kn, f));
            kn.screen_i8 = 2;  // automatic: lists in HBM, unless the calibration vetoed it
            CHECK(want_i8(kn, f) == (!tiered && !vetoed));
        }
    f = facts();
    kn.screen_defer = false;  // (the inline kernel reads bf16)
    for (int v = 0; v < 3; ++v) {
        kn.screen_i8 = v;
        CHECK(!want_i8(kn, f));
    }
}

static void test_directory() {
    const std::vector<uint8_t> all4(4, 1);
    // the 4096-segment rule, the screen impossible (option off): 1,200,000 rows are 2343
    // segments of 512 and 4687 of 256
    ScanDirectory d = scan_directory(std::vector<uint64_t>(4, 300000), all4, 0, false, 0);
    CHECK(d.ok);
    CHECK_EQ(d.seg_blocks, 4);
    CHECK_EQ(d.nseg[0], 1172);  // ceil(300000 / 256)
    d = scan_directory(std::vector<uint64_t>(4, 150000), all4, 0, false, 0);  // 600,000: 4687 of 128
    CHECK_EQ(d.seg_blocks, 2);
    d = scan_directory(std::vector<uint64_t>(4, 1000), all4, 0, false, 0);  // 62 segments even of 64
    CHECK_EQ(d.seg_blocks, 1);
    CHECK_EQ(d.nseg[0], 16);
    d = scan_directory(std::vector<uint64_t>(4, 600000), all4, 0, false, 0);  // 2,400,000: 4687 of 512
    CHECK_EQ(d.seg_blocks, 8);
    d = scan_directory(std::vector<uint64_t>(4, 1000), all4, 0, true, 2);  // (no screen for Cosine)
    CHECK_EQ(d.seg_blocks, 1);
    // the screen keeps 512, and so does the option
    d = scan_directory(std::vector<uint64_t>(4, 1000), all4, 0, true, 0);
    CHECK_EQ(d.seg_blocks, 8);
    CHECK_EQ(d.nseg[0], 2);
    d = scan_directory(std::vector<uint64_t>(4, 1000), all4, 0, true, 1);
    CHECK_EQ(d.seg_blocks, 8);
    d = scan_directory(std::vector<uint64_t>(4, 1000), all4, 8, false, 0);
    CHECK_EQ(d.seg_blocks, 8);
    d = scan_directory(std::vector<uint64_t>(4, 1000), all4, 16, true, 0);
    CHECK_EQ(d.seg_blocks, 16);
    CHECK_EQ(d.nseg[0], 1);
    // only owned lists count locally (the rule sees 4 * 1000 rows, not 2,400,000)
    d = scan_directory({1000, 600000, 1000, 600000, 1000, 600000, 1000, 600000}, {1, 0, 1, 0, 1, 0, 1, 0}, 0, false, 0);
    CHECK_EQ(d.seg_blocks, 1);
    // an un-owned list: 0 locally, its global count kept (64-vector segments)
    d = scan_directory({1000, 700, 0, 130}, {1, 0, 1, 1}, 1, true, 0);
    CHECK(d.ok);
    CHECK((d.count_local == std::vector<uint32_t>{1000, 0, 0, 130}));
    CHECK((d.count_global == std::vector<uint32_t>{1000, 700, 0, 130}));
    CHECK((d.nseg == std::vector<uint32_t>{16, 0, 0, 3}));
    CHECK_EQ(d.storable_n, 2);
    CHECK((d.nseg_prefix == std::vector<uint64_t>{0, 16, 19, 19, 19}));
    // the prefix sums the largest segment counts first
    d = scan_directory({100, 1000, 65, 0, 640}, std::vector<uint8_t>(5, 1), 1, true, 0);
    CHECK((d.nseg == std::vector<uint32_t>{2, 16, 2, 0, 10}));
    CHECK((d.nseg_prefix == std::vector<uint64_t>{0, 16, 26, 28, 30, 30}));
    CHECK_EQ(d.storable_n, 4);
    // screened items' length by the size-weighted mean segment count: below 16, below 96, above
    const std::vector<uint8_t> one(1, 1);
    CHECK_EQ(scan_directory({960}, one, 1, true, 0).screen_segs_auto, 4);    // 15 segments
    CHECK_EQ(scan_directory({1024}, one, 1, true, 0).screen_segs_auto, 8);   // 16
    CHECK_EQ(scan_directory({6080}, one, 1, true, 0).screen_segs_auto, 8);   // 95
    CHECK_EQ(scan_directory({6144}, one, 1, true, 0).screen_segs_auto, 16);  // 96
    CHECK_EQ(scan_directory({0}, one, 1, true, 0).screen_segs_auto, 4);      // (nothing stored)
    CHECK_EQ(scan_directory({6144}, {0}, 1, true, 0).screen_segs_auto, 4);   // (nothing stored here)
    const std::vector<uint8_t> both(2, 1);
    CHECK_EQ(scan_directory({640, 960}, both, 1, true, 0).screen_segs_auto, 4);   // (640*10 + 960*15) / 1600 = 13
    CHECK_EQ(scan_directory({640, 1280}, both, 1, true, 0).screen_segs_auto, 8);  // (640*10 + 1280*20) / 1920 = 16.7
    CHECK_EQ(scan_directory({64, 6400}, both, 1, true, 0).screen_segs_auto, 16);  // (64 + 6400*100) / 6464 = 99.0
    // list counts are 32-bit on the device
    CHECK(!scan_directory({5, 1ull << 32}, both, 0, true, 0).ok);
    d = scan_directory({5, (1ull << 32) - 1}, both, 0, true, 0);
    CHECK(d.ok);
    CHECK_EQ(d.count_global[1], 4294967295ll);
    CHECK_EQ(d.nseg[1], 8388608);  // ceil((2^32 - 1) / 512)
    // an index not trained yet
    d = scan_directory({}, {}, 0, true, 0);
    CHECK(d.ok);
    CHECK((d.nseg_prefix == std::vector<uint64_t>{0}));
    CHECK_EQ(d.storable_n, 0);
}

int main() {
    test_bounds_and_batch_cap();
    test_item_width();
    test_not_screened();
    test_exact_path();
    test_candidate_cap();
    test_want_i8();
    test_directory();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
