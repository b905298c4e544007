// engine.hpp — the index handle of the MI355X IVF-Flat engine (host side): one handle =
// one index on one device; engine.cpp binds it to the C ABI of include/vdb_ivf.h and
// group.cpp adds the multi-GPU forms (RCCL exchange, one handle per device).
//
// One handle = one index on one device. The whole index is HBM-resident in an
// interleaved list arena (kernels.hpp); a search is a short sequence of kernels
// per batch of queries, all enqueued on one stream with no host synchronisation:
//   pad queries -> coarse distances -> probe selection -> probe inversion (plan)
//   -> ivf_scan -> per-(query, probe) top-k -> per-query merge -> slot carry.
// Build-side calls (train/add/set_shard) synchronise where the reference
// algorithm needs a host decision (k-means++ draws from std::mt19937 on the host,
// exactly as ivf_flat_index.cpp:53-92 does).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <map>
#include <memory>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <queue>
#include <random>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/vdb_ivf.h"
#include "kernels.hpp"
#include "floor.hpp"
#include "index_file.hpp"
#include "list_cache.hpp"
#include "row_reader.hpp"
#include "scan_route.hpp"
#include "unit_kernels.hpp"
#include "uring.hpp"

namespace vdbe {

extern thread_local std::string g_last_error;

struct VdbError : std::runtime_error {
    int code;
    VdbError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        int code = (e == hipErrorOutOfMemory) ? VDB_ERR_OUT_OF_MEMORY : VDB_ERR_DEVICE;
        (void)hipGetLastError();
        throw VdbError(code, std::string(what) + ": " + hipGetErrorString(e));
    }
}
#define HIPCHECK(x) check((x), #x)

inline void check_nccl(ncclResult_t r, const char* what) {
    if (r != ncclSuccess) throw VdbError(VDB_ERR_DEVICE, std::string(what) + ": " + ncclGetErrorString(r));
}
#define NCCLCHECK(x) check_nccl((x), #x)

inline void require(bool ok, const std::string& msg, int code = VDB_ERR_INVALID_ARGUMENT) {
    if (!ok) throw VdbError(code, msg);
}

template <class F>
int guarded(F&& f) {
    try {
        f();
        return VDB_OK;
    } catch (const VdbError& e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_last_error = "host allocation failed";
        return VDB_ERR_OUT_OF_MEMORY;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return VDB_ERR_DEVICE;
    }
}

// `bytes` bytes of an index file at `off`, or a state error.
inline void pread_exact(int fd, void* dst, size_t bytes, uint64_t off) {
    char* p = (char*)dst;
    while (bytes) {
        const ssize_t r = ::pread(fd, p, bytes, (off_t)off);
        require(r > 0, "short read from the list file", VDB_ERR_STATE);
        p += r;
        bytes -= (size_t)r;
        off += (uint64_t)r;
    }
}

// An open index file for index_file.hpp's reader: closed again unless its user takes fd.
// A regular file is assumed: size is fstat's st_size, so anything that reports none there (a
// block device, a failed fstat) has size 0 and is refused as truncated. bytes_read is what
// open_lists adds to the handle's file_bytes_read.
struct IndexFileFd {
    int fd;
    uint64_t size = 0, bytes_read = 0;
    explicit IndexFileFd(const char* path, int flags = 0) : fd(::open(path, O_RDONLY | O_CLOEXEC | flags)) {
        struct stat sb;
        if (fd >= 0 && ::fstat(fd, &sb) == 0) size = (uint64_t)sb.st_size;
    }
    IndexFileFd(const IndexFileFd&) = delete;
    ~IndexFileFd() {
        if (fd >= 0) ::close(fd);
    }
    void operator()(uint64_t off, void* dst, size_t n) {
        pread_exact(fd, dst, n, off);
        bytes_read += n;
    }
};

// Run f with index_file.hpp's refusals turned into the C ABI's errors.
template <class F>
void index_file_checked(F&& f) {
    try {
        f();
    } catch (const IndexFileTruncated& e) {
        throw VdbError(VDB_ERR_STATE, e.what());
    } catch (const IndexFileRefused& e) {
        throw VdbError(VDB_ERR_INVALID_ARGUMENT, e.what());
    }
}

// Stream-ordered device memory for the engine's long-lived buffers (list arena, HBM list
// cache, search workspaces): one hipMemPool per device whose release threshold keeps freed
// memory reserved for the process (288 GB of HBM3E: an add's relayout and a workspace's
// growth reuse it without driver calls), allocated and freed on a per-device allocation
// stream. hipFreeAsync never synchronises the device the way hipFree does; the engine only
// releases a pooled buffer once no queued work can read it (stream synchronised, searches
// quiesced, or the workspace slot's previous call done).
// Off by default: on ROCm 7 buffers from the pool serialised the three batches a device
// runs in flight (1/8-shard rehearsal, 3 in flight: 93.7K QPS before the pool, 81.3K with
// it, 0.68 -> 0.79 ms per batch at an unchanged scan time); plain hipMalloc buffers overlap.
#ifndef VDB_DEVICE_POOL
#define VDB_DEVICE_POOL 0
#endif
struct DevicePool {
    hipMemPool_t pool = nullptr;
    hipStream_t stream = nullptr;
};
inline DevicePool& device_pool(int dev) {
    static std::mutex mu;
    static DevicePool pools[64];
    std::lock_guard<std::mutex> g(mu);
    require(dev >= 0 && dev < 64, "device ordinal out of range", VDB_ERR_INVALID_ARGUMENT);
    DevicePool& dp = pools[dev];
    if (!dp.pool) {
        hipMemPoolProps props = {};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        HIPCHECK(hipMemPoolCreate(&dp.pool, &props));
        uint64_t keep = ~0ull;
        HIPCHECK(hipMemPoolSetAttribute(dp.pool, hipMemPoolAttrReleaseThreshold, &keep));
        HIPCHECK(hipStreamCreateWithFlags(&dp.stream, hipStreamNonBlocking));
    }
    return dp;
}

// Growable device buffer (capacity in elements).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    bool host = false;  // page-locked host memory the device reads and writes directly
    bool pooled = false;  // device memory from the device's stream-ordered pool
    int dev = 0;          // (pooled) the device the memory belongs to
    DevBuf() = default;
    explicit DevBuf(bool pool) : pooled(pool && VDB_DEVICE_POOL) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) {
            if (host) (void)hipHostFree(p);
            else if (pooled) (void)hipFreeAsync(p, device_pool(dev).stream);
            else (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
    }
    T* ensure(size_t n) {
        if (n <= cap && p) return p;
        release();
        size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (host) {
            HIPCHECK(hipHostMalloc((void**)&p, bytes, hipHostMallocMapped | hipHostMallocPortable));
        } else if (pooled) {
            HIPCHECK(hipGetDevice(&dev));
            DevicePool& dp = device_pool(dev);
            HIPCHECK(hipMallocFromPoolAsync((void**)&p, bytes, dp.pool, dp.stream));
            HIPCHECK(hipStreamSynchronize(dp.stream));  // usable from any stream right away
        } else {
            HIPCHECK(hipMalloc(&p, bytes));
        }
        cap = std::max<size_t>(n, 1);
        return p;
    }
    size_t device_bytes() const { return (p && !host) ? cap * sizeof(T) : 0; }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        std::swap(host, o.host);
        std::swap(pooled, o.pooled);
        std::swap(dev, o.dev);
    }
};

// Page-locked host buffer (fast device-to-host copies of build-time scratch).
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    explicit PinnedBuf(size_t n) { HIPCHECK(hipHostMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T))); }
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
};

inline uint64_t cdiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

struct EventSet {
    hipEvent_t begin, coarse_end, scan_begin, scan_end, end;
    hipEvent_t collect_begin, collect_end;  // deferred screened scan: around its collect kernel
    bool collected = false;
    hipEvent_t x_end, m_end;  // multi-GPU: the all-gather done (comm stream), the rank merge done
    bool xchg = false;        // this batch (or call) ended in an exchange
};

// One host-API search() call waiting in the coalescing queue.
struct PendingSearch {
    const float* q;
    uint32_t n, nprobe, k;
    float* dist;
    uint64_t* ids;
    int rc = 1;  // 1 = pending, then a VDB_* code
    std::string err;
};

// Request coalescing (the reference's intent: QueryServiceImpl::Config max_batch_size /
// coalesce_window_ms, query_service.h:25-31, never implemented there): concurrent
// vdb_ivf_search callers enqueue; a dispatcher thread takes every compatible waiting call
// (same nprobe and k), up to max_queries, stages the queries in page-locked memory and
// enqueues ONE device search on a staging slot's own stream (H2D, search, D2H), then
// goes straight on to the next batch: up to kHostSlots batches are in flight, so one
// batch's copies and coarse step overlap the previous batch's scan (the pipelining the
// reference's DoubleBuffer / StreamScheduler intended, transfer_manager.h:168-239). A
// completion thread waits for each batch in issue order and hands the results back.
// Per-call slot semantics stay exact (request boundaries, kernels' req_start).
struct HostBatch {
    std::vector<PendingSearch*> reqs;
    uint32_t nq = 0, P = 0, K = 0;
    DevBuf<float> hq, hd;     // page-locked staging
    DevBuf<uint64_t> hi;
    DevBuf<uint32_t> hreq;
    DevBuf<float> dq, dd;     // device
    DevBuf<uint64_t> di;
    DevBuf<uint32_t> dreq;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    int rc = VDB_OK;
    std::string err;
    HostBatch() { hq.host = hd.host = hi.host = hreq.host = true; }
};

struct Coalescer {
    static constexpr int kHostSlots = 3;
    std::mutex m;
    std::condition_variable wake, done, slot_free, issued;
    std::deque<PendingSearch*> queue;
    std::deque<HostBatch*> inflight;  // issue order
    std::vector<HostBatch*> free_slots;
    HostBatch slots[kHostSlots];
    std::thread dispatcher, completer;
    bool stop = false, dispatch_done = false;
    uint64_t batches = 0, requests = 0;
};

}  // namespace vdbe

using namespace vdbe;

#ifndef VDB_SLOTS
#define VDB_SLOTS 3  // 4 measured slower at the 1/8 shard: 108K QPS at 4 in flight, 90K at 3, vs 128K (3 slots, 3 in flight)
#endif

struct vdb_ivf {
    uint32_t dim = 0, nlist = 0, dp = 0, d4 = 0;
    int metric = 0;
    // Metric::CosineDistance (3): an inner-product handle (metric = kIP: no kernel dispatch ever
    // sees a 3) over unit rows. Every ingested row is normalised once in padded_rows, every
    // batch's queries in stage_queries (launch_unit_rows), and a call's final distances are
    // mapped by 1.0f + d (cos_finish). Lists, save files and the tier's homes hold unit rows.
    bool unit_rows = false;
    // Rows that are unit rows already (vdb_ivf_load feeds a file's stored rows back through
    // add_to_lists_host): unit() is not idempotent bit for bit, so they are only padded.
    bool ingest_stored = false;
    // What the handle was configured with (save header, load / open_lists checks, attach_comm).
    int config_metric() const { return unit_rows ? 3 : metric; }
    int device = 0;
    uint64_t max_gpu_memory = 0;
    hipStream_t stream = nullptr;
    mutable std::mutex mu;

    DevBuf<float> cent_rm;   // [nlist][dp], zero pads
    DevBuf<float4> cent_il;  // [ceil(nlist/64)][d4][64]

    std::vector<uint64_t> count;      // per list, global (emptiness semantics)
    std::vector<uint8_t> owned;       // lists this handle scans
    std::vector<uint64_t> block_off;  // arena block offset per owned list
    uint64_t arena_blocks = 0;
    DevBuf<float4> arena{true};
    DevBuf<uint64_t> arena_ids{true};
    DevBuf<uint64_t> d_block_off;
    DevBuf<uint32_t> d_count_local, d_count_global, d_nseg;
    std::vector<uint64_t> nseg_prefix;  // sum of the j largest local segment counts
    uint64_t total = 0;
    uint32_t rank = 0, world = 1;
    uint32_t batch = 256;
    int stale = 1;
    bool wide_scan = true;
    int coarse_mode = 1;  // 1: MFMA bounds + exact re-rank (L2/IP); 0: exact VALU distances
    uint32_t wide_stride = 1;  // wide-item dispatch permutation (1 = plan order; measured best)
    uint32_t seg_blocks = 8;  // current segment size (blocks of 64 vectors; upload_directory sets it)
    uint32_t seg_blocks_opt = 0;                // 0 = automatic (upload_directory)
    bool bounded_stats = false;                 // count the bounded scan's re-ranks and blocks (profile_read)
    // wide items of at least this many queries are bounded on the matrix cores and
    // re-ranked exactly (ivf_scan_bounded); 0 = never. Off by default: on the bench
    // workloads the exact re-ranks (per-list top-k insertions, ~5% of pairs, each a
    // gathered re-read of an evicted vector) cost more than the VALU it saves
    // (DESIGN.md "Bounded scan: measured and rejected as default").
    uint32_t scan_mfma_min = 0;
    // persistent scan grid in workgroups (0: 2 per CU on the whole chip)
    uint32_t scan_blocks = 0;
    uint32_t segs_item_opt = 0;   // segments per wide item (0: one per wave, taken dynamically)
    uint32_t wide_group = 16;     // queries per wide item at most: 16 (4-wave workgroups) or 32 (8-wave)
    bool fused_scan = true;       // narrow items inside the wide scan's grid (option fused_scan; +2-3 %)
    bool fused_merge = true;      // the four per-batch merges as one launch (option fused_merge)
    // At most this many scans of batches in flight overlap (0: no limit): a batch's scan
    // waits for the scan issued `scan_window` batches earlier to finish, so the GPU serves
    // batches closer to issue order (latency spread at several batches in flight).
    uint32_t scan_window = 0;
    uint64_t scan_seq = 0;
    int scan_hist[8] = {};  // slot index of the scans issued, by sequence number
    uint32_t narrow_blocks = 64;  // persistent narrow-scan workgroups beside the wide scan (1/8 shard: +1.5 % vs 512)

    // Screened scan (screen.hip, option "screen", on by default): every (query, vector)
    // distance is bounded on the matrix cores from a bf16 shadow of the lists and computed
    // exactly (the reference's sequential fp32 sum) only where it can reach the list's
    // top-k; results are bit-identical to the exact scan. Built from the arena by the first
    // search after the lists change: the shadow in MFMA operand order (half the arena's
    // bytes), the fp32 rows in slot order (then the lists' only fp32 copy: the arena is
    // released and rebuilt from them on demand), per-slot norms. The tier keeps the shadow,
    // norms and ids of every stored list resident (screen_update_tier). Not built for
    // Cosine, or when an allocation fails (the exact scan serves); max_gpu_memory caps list
    // bytes only.
    bool screen_opt = true;
    bool screen_ready = false;
    bool screen_stale = false;  // lists or centroids changed since the last build
    uint32_t screen_segs_auto = 4;  // segments per screened wide item (upload_directory; option segs_per_item)
    uint32_t screen_group = 0;      // queries per screened wide item at most: 16 or 32, 0 = automatic (option screen_group)
    // Shadow format of the deferred screen (option screen_i8): 1 = int8 with a per-vector scale
    // (half the bf16 shadow's bytes, a ~4.6x wider bound); 0 = bf16. The inline kernel
    // (screen_defer 0) always uses bf16.
    // 2 (default) = automatic (want_i8): int8 for lists in HBM, at both item widths (16- and
    // 32-query items), kept unless the calibration batch at the build vetoes it
    // (screen_calibrate: survivors beyond k per pair above 1.5 % of the pairs, or an overflow:
    // a regime where its wider bound re-checks more than its smaller stream saves); bf16 in the
    // tier (each survivor is a row read from the home). Round 5, same box: cfg3 collect 1.40
    // vs 2.43 ms (bf16), cfg4 shard 2.15 vs 3.38 ms; the mixture is vetoed (6.2 % excess).
    int screen_i8 = 2;
    bool i8_vetoed = false;  // (automatic: the calibration vetoed int8 for this handle)
    uint32_t last_P = 0;     // the nprobe of the search that triggers a screen build
    bool want_i8() const { return vdbe::want_i8(knobs(), facts()); }
    uint32_t screen_thr_every = 0;  // deferred collect: blocks between re-reads of the shared thresholds, 0 = automatic (option screen_thr_every)
    // Deferred re-checks (option screen_defer, default 1): the scan only collects candidates
    // against upper-bound thresholds; survivors of each pair's final threshold are re-checked
    // exactly afterwards from the arena (screen.hip ivf_screen_collect). 0: the inline kernel
    // (re-checks as candidates appear, from a row-major fp32 copy of the lists).
    bool screen_defer = true;
    uint32_t screen_cand_cap = 4u << 20;  // collected candidates per batch (an overflowing pair is recomputed whole)
    // Two-pass exact re-check (option screen_recheck2, default on; rows in HBM): per pair first the k
    // survivors of smallest lower bound, then only the others whose lower bound is not above
    // the k-th exact distance so far (screen.hip ivf_screen_recheck2); 0: every survivor of the
    // final threshold (ivf_screen_exact_lane + ivf_screen_pair_topk). Results are identical.
    bool screen_recheck2 = true;
    // One fp32 copy of the lists in HBM: while the screen is built, the row-major copy
    // (screen_rows, slot order: what the exact re-checks read) is the only one and the
    // interleaved arena is released (arena_dropped). Exact-path searches (k > 64, the
    // run-time floor's batches) scan the row-major copy itself (ScanArgs::rows_layout: no
    // rebuild, no quiesce, no second copy); what needs the interleaved layout (an add /
    // relayout, the screen off, the opt-in bounded scan, Cosine) rebuilds it from the rows
    // first (ensure_arena: one interleave pass). Footprint while screening: rows + shadow +
    // norms + ids ~ 1.5x the lists, whatever k the searches ask for.
    bool arena_dropped = false;
    // The screen in the list-cache tier (an index larger than HBM, configs[4]): the shadow,
    // norms and ids of EVERY stored list stay HBM-resident (half the fp32 list bytes), packed
    // by sblock_off; the fp32 rows stay at the home and only the survivors' rows are read per
    // batch: straight from the page-locked host arena over PCIe, or, from a file home, by
    // io_uring into page-locked staging and one copy to HBM (fetch_rows; the read loop itself
    // is host-only code of its own, row_reader.hpp). No list is loaded into the cache for such
    // a batch (the cache serves the exact-path searches).
    std::vector<uint64_t> sblock_off;  // tier: per stored list its first shadow block
    std::vector<uint32_t> sblist_host; // tier, file home: per shadow block its list
    uint64_t sblocks = 0;
    DevBuf<uint64_t> d_sblock_off;
    DevBuf<uint64_t> screen_ids;       // tier: the ids in shadow slot order
    DevBuf<float> fetch_stage;         // tier, file home: page-locked staging of the survivors' rows
    DevBuf<char> fetch_bounce;         // ... O_DIRECT reads: 4 KiB-aligned supersets, one slot per read in flight
    bool tier_row_direct = true;       // option tier_row_direct: survivor rows with O_DIRECT (no page cache)
    uint32_t tier_row_qd = 256;        // option tier_row_qd: survivor-row reads in flight (their own ring)
    RowReader row_reader;              // ... the reads themselves (its own ring)
    DevBuf<float> fetch_dev;           // ... on the device ([n][dim], padded into the slot's srows)
    std::vector<uint2> fetch_surv;     // ... their (slot, pair)
    uint64_t screen_rows_fetched = 0, screen_row_bytes = 0, screen_tier_batches = 0, screen_reruns = 0;
    uint64_t screen_rows_cached = 0;   // ... survivor rows copied from the HBM cache instead
    bool tier_row_cache = true;        // option tier_row_cache: the idle cache holds the largest lists' rows
    DevBuf<ulonglong2> cache_src;      // ... per batch {row index, cache slot} of those survivors
    std::vector<ulonglong2> cache_src_host;
    uint32_t tier_cand_cap = 0;        // ... a candidate capacity grown by an overflow
    // ... at most this many candidates per batch (option tier_cand_max; never below
    // screen_cand_cap): a batch that needs more is served by the exact list-cache path
    uint32_t tier_cand_max = 32u << 20;
    // (option collect_stamps, diagnostics) timeline records of the collect kernel's items
    DevBuf<unsigned long long> stamps_buf;
    uint32_t stamps_cap = 0, stamp_batch = 0;
    // (vdb_ivf_screen_snapshot, diagnostics) the most recently issued batch: the slot that
    // holds its buffers and the scalars its collect ran with; ok only for the deferred
    // screened route with rows in HBM
    struct ScreenSnap {
        bool ok = false;
        int slot = -1;
        uint32_t B = 0, P = 0, k = 0, segs_item = 0, wide_q = 0, cand_cap = 0, i8 = 0, grid = 0;
    } snap;
    uint64_t screen_tier_fallbacks = 0;
    bool force_exact = false;          // (that path's batches: never screened)
    // Run-time floor under the screen (lists in HBM; floor.hpp): every deferred batch reports
    // its survivors (or an overflow of its candidate buffer), its (query, vector) pairs and k x
    // its valid (query, list) pairs into a ring of page-locked host memory, read without
    // synchronisation when a later batch is planned. A batch whose survivors beyond those
    // exceed screen_floor_ppm of its pairs (a regime where the bound is wider than the
    // distance spread) sends the next batches to the exact scan, with backoff, then one
    // probe batch retries the screen. (Break-even at cfg3: the exact scan 4.9 ms against the
    // screen's 2.7 ms plus ~4.6 ns per survivor, ~9 % of the batch's 5.0M pairs; 5 % leaves
    // room for the retries.) Results are the same either way; only speed changes.
    ScreenFloor floor;
    DevBuf<uint4> floor_host;  // page-locked: ScreenFloor::kRing report entries
    const volatile uint32_t* floor_entry(uint32_t i) const { return (const volatile uint32_t*)(floor_host.p + i); }
    DevBuf<uint4> screen_sh;
    DevBuf<float> screen_rows;
    DevBuf<float4> screen_meta;
    DevBuf<float> screen_scale;  // int8 shadow: per slot s_b
    bool screen_fmt_i8 = false;  // the shadow built is int8 (else bf16)
    DevBuf<uint32_t> screen_blist;  // the list of every arena block (residuals against its centroid)

    // List-cache tier (option list_cache_bytes > 0), the reference's residency model
    // (load_list_to_gpu on first touch under a byte cap, evict_list_from_gpu,
    // ivf_flat_index.cpp:387-471) for indexes larger than HBM: the arena then lives in
    // page-locked host memory and HBM holds a cache of whole lists. Before a batch is
    // planned, every list it probes is made resident (DMA of its blocks), evicting the
    // least recently used lists the batch does not probe; the scan reads the cache
    // through the same directory (d_block_off), so the kernels are unchanged. Where the
    // lists sit in the cache, which leave and how a call is cut: list_cache.hpp.
    ListCache lc;  // (capacity 0: tier off, the arena is in HBM)
    DevBuf<float4> cache{true};
    DevBuf<uint64_t> cache_ids{true};
    uint64_t storable_n = 0;  // non-empty lists stored here
    DevBuf<uint32_t> probe_stage;  // pinned: the batch's probes, read by the host
    DevBuf<uint64_t> dir_stage;    // pinned: directory upload source
    // Recorded after every cache load and directory upload, on the stream that made
    // them. Every tier-mode batch waits for it before it plans and scans, so a search
    // on another stream whose lists are all cached never reads blocks or directory
    // entries still in flight (a miss quiesces the other streams first, so the latest
    // recording covers every earlier load).
    hipEvent_t tier_ev = nullptr;
    bool tier_ev_used = false;

    // File home for the tier (vdb_ivf_open_lists): the lists stay in an index file written
    // by vdb_ivf_save and are read into the cache on demand: io_uring reads (O_DIRECT when
    // the file system allows it) into a ring of page-locked staging buffers, H2D copies,
    // then pad + interleave kernels into the cache's block layout.
    int home_fd = -1;
    int home_fd_direct = -1;         // O_DIRECT descriptor of the same file (or -1: buffered)
    // O_DIRECT granule the file system accepts for offsets and sizes, probed at open: 512 on
    // most (a 3,072-B survivor row then reads 3,072 or 3,584 B), else 4096 (4 KiB-aligned
    // supersets, 1.5-2 pages per row)
    uint32_t dio_align = 4096;
    IndexFileDirectory home;         // where the file keeps each list (index_file.hpp)
    struct Stage {                   // one page-locked staging buffer of the read ring
        DevBuf<char> buf;
        hipEvent_t copied = nullptr;  // its H2D copies are done: the buffer may be refilled
        bool copying = false;
        int reads = 0;                // reads in flight
        uint64_t m = 0, dst_block = 0;
        size_t ids_delta = 0, vec_delta = 0;
    };
    static constexpr int kStages = 8;
    Stage stages[kStages];
    std::unique_ptr<UringReader> uring;
    DevBuf<float> drows, dpad;       // device: a chunk's rows, then zero-padded to dp (search stream)
    DevBuf<float> drows_cs, dpad_cs; // the same for loads on copy_stream (they may run concurrently)
    uint64_t file_bytes_read = 0;
    // tier pipeline: loads for the next sub-batch run on copy_stream beside the scan
    hipStream_t copy_stream = nullptr;
    hipEvent_t sb_done[2] = {nullptr, nullptr}, load_ev = nullptr, tier_call_ev = nullptr;
    bool tier_call_used = false;
    uint64_t tier_prefetches = 0, tier_sync_loads = 0, tier_subbatches = 0;

    // Search workspaces: a ring of slots so that searches issued on different streams
    // run concurrently (one batch's small kernels and scan tail overlap the next
    // batch's scan). A call takes the next slot; its stream first waits for the
    // slot's previous batch (slot.done), wherever that ran.
    struct SearchSlot {
        DevBuf<float> qpad{true}, cd{true}, cdelta{true}, part_d{true}, slot_d{true}, carry_d{true}, carry2_d{true};
        DevBuf<uint64_t> part_i{true}, slot_i{true}, carry_i{true}, carry2_i{true};
        uint32_t carry_sel = 0;  // fused merge: the carry buffer the call's next batch reads (ping-pong)
        uint64_t xfill = 0;      // (exchange_emulate_world) the record size the other ranks' empty records were filled for
        const float* q = nullptr;  // the batch's zero-padded queries: qpad, or the caller's rows when dim == dp
        DevBuf<uint32_t> probes{true}, nseg_qp{true}, pbqp{true}, sorted_pair{true}, pbs{true}, counters{true},
            l1base{true}, cand{true}, thr{true};
        DevBuf<uint2> l1_items{true};
        DevBuf<float> l1_d{true};
        DevBuf<uint64_t> l1_i{true};
        DevBuf<vdbk::ScanItem> items{true}, items_w{true};
        DevBuf<uint16_t> qres{true};  // screened scan: per (query, probe) bf16 A rows [B * P][dp]
        DevBuf<float4> pst{true};     // ... and their norms
        DevBuf<float> qscale{true};   // ... and (int8 shadow) their scales
        DevBuf<uint32_t> thr4{true};  // ... and, per sorted pair, 4 quarter-list thresholds
        // deferred screened scan: collected candidates, per sorted pair survivor counts, offsets and
        // overflow marks, the survivors' slots grouped per pair, and (tier) their fetched rows
        DevBuf<uint4> scand{true};
        DevBuf<uint32_t> scnt{true}, soff{true}, ovf{true}, ubcnt{true};
        DevBuf<uint2> surv{true};
        DevBuf<float> ublist{true}, sdist{true};
        DevBuf<float> srows{true};
        DevBuf<float> slb{true};         // screened tier, two-pass: the survivors' lower bounds
        DevBuf<uint8_t> smark{true};     // ... their pass marks (1 A, 2 B)
        DevBuf<uint32_t> rowmap{true};   // ... survivor -> compact fetched row
        DevBuf<uint8_t> xrec{true}, xgat{true};  // multi-GPU: this rank's packed partials, the gathered records
        DevBuf<float> gq{true};            // group member: the call's queries on this device
        DevBuf<uint32_t> greq{true};       // group member: the call's request starts on this device
        hipStream_t side = nullptr;  // narrow-item scan, concurrent with the wide items
        hipStream_t gstream = nullptr;  // group member: the stream this slot's searches run on
        hipEvent_t x_ready = nullptr, x_done = nullptr;  // fences around this slot's collectives
        hipEvent_t fork = nullptr, join = nullptr, done = nullptr;
        hipEvent_t scan_done = nullptr;  // (scan_window) this slot's latest scan has finished
        bool used = false;
        uint64_t device_bytes() const {
            uint64_t b = 0;
            for (uint64_t x : {qpad.device_bytes(), cd.device_bytes(), cdelta.device_bytes(), part_d.device_bytes(),
                               slot_d.device_bytes(), carry_d.device_bytes(), carry2_d.device_bytes(),
                               part_i.device_bytes(), slot_i.device_bytes(), carry_i.device_bytes(),
                               carry2_i.device_bytes(), probes.device_bytes(), nseg_qp.device_bytes(), pbqp.device_bytes(),
                               sorted_pair.device_bytes(), pbs.device_bytes(), counters.device_bytes(),
                               l1base.device_bytes(), cand.device_bytes(), thr.device_bytes(), l1_items.device_bytes(),
                               l1_d.device_bytes(), l1_i.device_bytes(), items.device_bytes(), items_w.device_bytes(),
                               qres.device_bytes(), pst.device_bytes(), qscale.device_bytes(), thr4.device_bytes(), scand.device_bytes(),
                               scnt.device_bytes(), soff.device_bytes(), ovf.device_bytes(), ubcnt.device_bytes(),
                               surv.device_bytes(), ublist.device_bytes(), sdist.device_bytes(), srows.device_bytes(),
                               slb.device_bytes(), smark.device_bytes(), rowmap.device_bytes(),
                               xrec.device_bytes(), xgat.device_bytes(), gq.device_bytes(), greq.device_bytes()})
                b += x;
            return b;
        }
    };
    static constexpr int kSlots = VDB_SLOTS;  // workspace slots: batches one handle runs concurrently
    SearchSlot slots[kSlots];
    uint32_t next_slot = 0;

    // ---- multi-GPU: lists sharded over ranks (LPT), every rank runs the
    // coarse step for the whole batch, scans its own lists and merges its slots into ONE
    // packed record per batch (f32 dist[B][k] | pad | u64 ids[B][k]); one RCCL all-gather
    // of the records over xGMI, then the on-device unique-id merge. The communicator is
    // attached (one process per GPU, vdb_ivf_attach_comm) or owned by a group handle
    // (one process, one member handle per device, vdb_ivf_create_group).
    ncclComm_t comm = nullptr;
    bool comm_owned = false;
    uint32_t comm_rank = 0, comm_world = 1;
    // (option exchange_emulate_world, diagnostics) a communicator of world 1 exchanges records
    // the size of W ranks' (the batch's record plus W - 1 empty records of the same layout) and
    // merges W records: the per-batch cost of an 8-GPU node's exchange and rank merge on one
    // rank's timeline (one GPU cannot hold 8 ranks: RCCL refuses two ranks on one device); the
    // results stay this handle's own exact answer
    uint32_t xchg_emulate = 0;
    uint32_t xchg_records() const { return comm_world > 1 ? comm_world : std::max<uint32_t>(1, xchg_emulate); }
    // Every collective of the communicator runs on this one stream, fenced by events
    // against the search stream that produced / consumes its buffers: with several
    // batches in flight on several streams, every rank then executes its collectives in
    // the same (issue) order whatever the library does across streams.
    hipStream_t comm_stream = nullptr;

    // Order a collective on comm_stream after the work queued on s (returns comm_stream).
    void make_comm_stream() {  // with the communicator (the device must be current)
        // (high priority: a queue of its own, apart from the 4 the search streams share —
        // profiles/r05_hw_queue_probe.txt — and the exchange dispatched ahead of scan work)
        if (!comm_stream) {
            int lo = 0, hi = 0;
            HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIPCHECK(hipStreamCreateWithPriority(&comm_stream, hipStreamNonBlocking, hi));
        }
    }
    hipStream_t comm_enter(SearchSlot& w, hipStream_t s) {
        if (!w.x_ready) {
            HIPCHECK(hipEventCreateWithFlags(&w.x_ready, hipEventDisableTiming));
            HIPCHECK(hipEventCreateWithFlags(&w.x_done, hipEventDisableTiming));
        }
        HIPCHECK(hipEventRecord(w.x_ready, s));
        HIPCHECK(hipStreamWaitEvent(comm_stream, w.x_ready, 0));
        return comm_stream;
    }
    // ... and the work queued on s next after it.
    void comm_leave(SearchSlot& w, hipStream_t s) {
        HIPCHECK(hipEventRecord(w.x_done, comm_stream));
        HIPCHECK(hipStreamWaitEvent(s, w.x_done, 0));
    }
    // Group handle: members[m] holds the lists owner[l] == m places on its device; the
    // group itself holds only the host-API staging on members[0]'s device.
    std::vector<std::unique_ptr<vdb_ivf>> members;
    std::vector<uint32_t> owner;  // per list: member storing it, or kUnplaced
    static constexpr uint32_t kUnplaced = 0xFFFFFFFFu;
    bool group_rccl = false;      // members on distinct devices: RCCL; else device copies (rehearsal)
    std::vector<hipEvent_t> gev;  // group call fences, 2 per member
    bool is_group() const { return !members.empty(); }
    vdb_ivf* head() { return is_group() ? members[0].get() : this; }
    // the handle storing list l (a group member, or this handle)
    vdb_ivf* store_of(uint32_t l) {
        if (!is_group()) return this;
        return owner[l] == kUnplaced ? members[0].get() : members[owner[l]].get();
    }
    DevBuf<float> out_d, qin;  // host-API staging (synchronous calls)
    DevBuf<uint64_t> out_i;
    DevBuf<uint32_t> d_req;    // coalesced calls: request start per query
    std::unique_ptr<Coalescer> co;
    std::mutex co_init_mu;
    bool coalesce = true;
    uint32_t coalesce_max_queries = 1024;
    uint32_t coalesce_window_us = 0;
    DevBuf<unsigned long long> stats, stats_scratch;

    bool prof = false;
    std::vector<EventSet> events;
    size_t events_used = 0;

    ~vdb_ivf() {
        stop_coalescer();
        // An exchange that missed its deadline never completes: nothing is waited for and
        // the communicator is left to the process's exit (destroying or aborting it could
        // hang, or free what a still-queued collective reads).
        const bool failed = comm_failed();
        stop_watch();
        members.clear();  // each member waits for and frees its own device work
        (void)hipSetDevice(device);
        if (!failed) {
            try {
                quiesce();  // pooled buffers are freed stream-ordered: no search may still read them
            } catch (...) {
            }
            if (stream) (void)hipStreamSynchronize(stream);
            for (auto& sl : slots)
                if (sl.gstream) (void)hipStreamSynchronize(sl.gstream);
        }
        if (comm) {
            if (comm_owned && !failed) (void)ncclCommDestroy(comm);
            comm = nullptr;
        }
        for (auto& e : gev) (void)hipEventDestroy(e);
        if (home_fd >= 0) ::close(home_fd);
        if (copy_stream) (void)hipStreamSynchronize(copy_stream);
        for (auto& st : stages)
            if (st.copied) (void)hipEventDestroy(st.copied);
        for (hipEvent_t e : {sb_done[0], sb_done[1], load_ev, tier_call_ev, tier_ev})
            if (e) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        if (home_fd_direct >= 0) ::close(home_fd_direct);
        for (auto& e : events)
            for (hipEvent_t x : {e.begin, e.coarse_end, e.scan_begin, e.scan_end, e.end, e.x_end, e.m_end, e.collect_begin, e.collect_end})
                (void)hipEventDestroy(x);
        for (auto& sl : slots) {
            if (sl.fork) (void)hipEventDestroy(sl.fork);
            if (sl.join) (void)hipEventDestroy(sl.join);
            if (sl.done) (void)hipEventDestroy(sl.done);
            if (sl.scan_done) (void)hipEventDestroy(sl.scan_done);
            if (sl.side) (void)hipStreamDestroy(sl.side);
            if (sl.gstream) (void)hipStreamDestroy(sl.gstream);
            if (sl.x_ready) (void)hipEventDestroy(sl.x_ready);
            if (sl.x_done) (void)hipEventDestroy(sl.x_done);
        }
        if (comm_stream) (void)hipStreamDestroy(comm_stream);
        if (stream) (void)hipStreamDestroy(stream);
    }

    void set_device() { HIPCHECK(hipSetDevice(device)); }

    // Every byte of device memory the handle holds (vdb_ivf_gpu_bytes_allocated): lists in
    // whatever layouts exist (arena, row-major copy, bf16 shadow, norms, ids, list cache),
    // centroids, directories, the search workspaces of every slot and the staging buffers.
    uint64_t device_footprint() const {
        uint64_t b = 0;
        for (uint64_t x : {cent_rm.device_bytes(), cent_il.device_bytes(), arena.device_bytes(), arena_ids.device_bytes(),
                           d_block_off.device_bytes(), d_count_local.device_bytes(), d_count_global.device_bytes(),
                           d_nseg.device_bytes(), screen_sh.device_bytes(), screen_rows.device_bytes(),
                           screen_meta.device_bytes(), screen_blist.device_bytes(), screen_scale.device_bytes(),
                           screen_ids.device_bytes(), d_sblock_off.device_bytes(), cache_src.device_bytes(),
                           cache.device_bytes(),
                           cache_ids.device_bytes(), drows.device_bytes(), dpad.device_bytes(), drows_cs.device_bytes(),
                           dpad_cs.device_bytes(), out_d.device_bytes(), qin.device_bytes(), out_i.device_bytes(),
                           d_req.device_bytes(), stats.device_bytes()})
            b += x;
        for (const auto& w : slots) b += w.device_bytes();
        if (co)
            for (const HostBatch& hb : co->slots)
                b += hb.dq.device_bytes() + hb.dd.device_bytes() + hb.di.device_bytes() + hb.dreq.device_bytes();
        return b;
    }

    // ---- host-API search: direct, or through the coalescing queue ----
    void search_host(const float* q, uint32_t n, uint32_t nprobe, uint32_t k, float* dist, uint64_t* ids,
                     const uint32_t* h_req_start) {
        set_device();
        HIPCHECK(hipMemcpyAsync(qin.ensure((size_t)n * dim), q, (size_t)n * dim * 4, hipMemcpyHostToDevice, stream));
        const uint32_t* dr = nullptr;
        if (h_req_start) {
            HIPCHECK(hipMemcpyAsync(d_req.ensure(n), h_req_start, (size_t)n * 4, hipMemcpyHostToDevice, stream));
            dr = d_req.p;
        }
        search_device(qin.p, n, nprobe, k, out_d.ensure((size_t)n * k), out_i.ensure((size_t)n * k), stream, dr);
        HIPCHECK(hipMemcpyAsync(dist, out_d.p, (size_t)n * k * 4, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipMemcpyAsync(ids, out_i.p, (size_t)n * k * 8, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }

    void start_coalescer() {
        if (co) return;
        co.reset(new Coalescer());
        set_device();
        for (HostBatch& hb : co->slots) {
            HIPCHECK(hipStreamCreateWithFlags(&hb.stream, hipStreamNonBlocking));
            HIPCHECK(hipEventCreateWithFlags(&hb.done, hipEventDisableTiming));
            co->free_slots.push_back(&hb);
        }
        co->dispatcher = std::thread([this] { dispatch_loop(); });
        co->completer = std::thread([this] { complete_loop(); });
    }

    void stop_coalescer() {
        if (!co) return;
        {
            std::lock_guard<std::mutex> g(co->m);
            co->stop = true;
        }
        co->wake.notify_all();
        co->slot_free.notify_all();
        if (co->dispatcher.joinable()) co->dispatcher.join();
        if (co->completer.joinable()) co->completer.join();
        (void)hipSetDevice(device);
        for (HostBatch& hb : co->slots) {
            if (hb.stream) (void)hipStreamDestroy(hb.stream);
            if (hb.done) (void)hipEventDestroy(hb.done);
        }
        co.reset();
    }

    void dispatch_loop() {
        Coalescer& c = *co;
        (void)hipSetDevice(device);
        for (;;) {
            HostBatch* hb = nullptr;
            {
                std::unique_lock<std::mutex> lk(c.m);
                c.wake.wait(lk, [&] { return c.stop || !c.queue.empty(); });
                if (c.queue.empty()) break;  // stop requested and nothing left
                // a free staging slot: at most kHostSlots batches in flight (calls keep
                // queueing meanwhile, so the next batch grows while the device is busy)
                c.slot_free.wait(lk, [&] { return !c.free_slots.empty(); });
                if (coalesce_window_us)
                    c.wake.wait_for(lk, std::chrono::microseconds(coalesce_window_us), [&] {
                        uint64_t t = 0;
                        for (auto* r : c.queue) t += r->n;
                        return c.stop || t >= coalesce_max_queries;
                    });
                hb = c.free_slots.back();
                c.free_slots.pop_back();
                hb->reqs.clear();
                hb->nq = 0;
                hb->P = c.queue.front()->nprobe;
                hb->K = c.queue.front()->k;
                for (auto it = c.queue.begin(); it != c.queue.end();) {
                    PendingSearch* r = *it;
                    if (r->nprobe == hb->P && r->k == hb->K && (hb->reqs.empty() || hb->nq + r->n <= coalesce_max_queries)) {
                        hb->reqs.push_back(r);
                        hb->nq += r->n;
                        it = c.queue.erase(it);
                    } else {
                        ++it;
                    }
                }
                c.batches++;
                c.requests += hb->reqs.size();
            }
            hb->rc = VDB_OK;
            hb->err.clear();
            try {
                const uint32_t nq = hb->nq, K = hb->K;
                float* hq = hb->hq.ensure((size_t)nq * dim);
                uint32_t* hr = hb->reqs.size() > 1 ? hb->hreq.ensure(nq) : nullptr;
                uint32_t o = 0;
                for (PendingSearch* r : hb->reqs) {
                    std::memcpy(hq + (size_t)o * dim, r->q, (size_t)r->n * dim * 4);
                    if (hr)
                        for (uint32_t i = 0; i < r->n; ++i) hr[o + i] = o;
                    o += r->n;
                }
                hb->hd.ensure((size_t)nq * K);
                hb->hi.ensure((size_t)nq * K);
                std::lock_guard<std::mutex> g(mu);  // held only while the batch is enqueued
                set_device();
                HIPCHECK(hipMemcpyAsync(hb->dq.ensure((size_t)nq * dim), hq, (size_t)nq * dim * 4, hipMemcpyHostToDevice,
                                        hb->stream));
                const uint32_t* dr = nullptr;
                if (hr) {
                    HIPCHECK(hipMemcpyAsync(hb->dreq.ensure(nq), hr, (size_t)nq * 4, hipMemcpyHostToDevice, hb->stream));
                    dr = hb->dreq.p;
                }
                search_device(hb->dq.p, nq, hb->P, K, hb->dd.ensure((size_t)nq * K), hb->di.ensure((size_t)nq * K),
                              hb->stream, dr);
                HIPCHECK(hipMemcpyAsync(hb->hd.p, hb->dd.p, (size_t)nq * K * 4, hipMemcpyDeviceToHost, hb->stream));
                HIPCHECK(hipMemcpyAsync(hb->hi.p, hb->di.p, (size_t)nq * K * 8, hipMemcpyDeviceToHost, hb->stream));
                HIPCHECK(hipEventRecord(hb->done, hb->stream));
            } catch (const VdbError& e) {
                hb->rc = e.code;
                hb->err = e.what();
            } catch (const std::exception& e) {
                hb->rc = VDB_ERR_DEVICE;
                hb->err = e.what();
            }
            {
                std::lock_guard<std::mutex> g(c.m);
                c.inflight.push_back(hb);
            }
            c.issued.notify_one();
        }
        {
            std::lock_guard<std::mutex> g(c.m);
            c.dispatch_done = true;
        }
        c.issued.notify_one();
    }

    void complete_loop() {
        Coalescer& c = *co;
        (void)hipSetDevice(device);
        for (;;) {
            HostBatch* hb = nullptr;
            {
                std::unique_lock<std::mutex> lk(c.m);
                c.issued.wait(lk, [&] { return !c.inflight.empty() || c.dispatch_done; });
                if (c.inflight.empty()) return;
                hb = c.inflight.front();
                c.inflight.pop_front();
            }
            if (hb->rc == VDB_OK) {
                const hipError_t e = hipEventSynchronize(hb->done);
                if (e != hipSuccess) {
                    hb->rc = VDB_ERR_DEVICE;
                    hb->err = std::string("search batch: ") + hipGetErrorString(e);
                }
            }
            if (hb->rc == VDB_OK) {
                uint32_t o = 0;
                for (PendingSearch* r : hb->reqs) {
                    std::memcpy(r->dist, hb->hd.p + (size_t)o * hb->K, (size_t)r->n * hb->K * 4);
                    std::memcpy(r->ids, hb->hi.p + (size_t)o * hb->K, (size_t)r->n * hb->K * 8);
                    o += r->n;
                }
            }
            {
                std::lock_guard<std::mutex> g(c.m);
                for (PendingSearch* r : hb->reqs) {
                    r->err = hb->err;
                    r->rc = hb->rc;
                }
                hb->reqs.clear();
                c.free_slots.push_back(hb);
            }
            c.done.notify_all();
            c.slot_free.notify_one();
        }
    }

    void search_coalesced(const float* q, uint32_t n, uint32_t nprobe, uint32_t k, float* dist, uint64_t* ids) {
        PendingSearch r{q, n, nprobe, k, dist, ids};
        {
            // not `mu`: the dispatcher takes that to enqueue a batch, and callers must be
            // able to queue meanwhile
            std::lock_guard<std::mutex> g(co_init_mu);
            start_coalescer();
        }
        std::unique_lock<std::mutex> lk(co->m);
        co->queue.push_back(&r);
        co->wake.notify_one();
        co->done.wait(lk, [&] { return r.rc != 1; });
        if (r.rc != VDB_OK) throw VdbError(r.rc, r.err);
    }

    // Wait for every search still in flight on any stream before the index changes
    // under it (buffers freed, lists moved, centroids rewritten).
    void quiesce() {
        for (auto& sl : slots)
            if (sl.used) HIPCHECK(hipEventSynchronize(sl.done));
    }

    // Upload the list directory and recompute the segment-count prefix.
    void upload_directory() {
        quiesce();
        // (segment size, counts, segment counts and the screened items' length: scan_route.hpp)
        ScanDirectory dir = scan_directory(count, owned, seg_blocks_opt, screen_opt, metric);
        require(dir.ok, "list longer than 2^32 vectors", VDB_ERR_UNSUPPORTED);
        seg_blocks = dir.seg_blocks;
        storable_n = dir.storable_n;
        screen_segs_auto = dir.screen_segs_auto;
        nseg_prefix = std::move(dir.nseg_prefix);
        upload_scan_directory(stream);
        HIPCHECK(hipMemcpyAsync(d_count_local.ensure(nlist), dir.count_local.data(), nlist * 4, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(d_count_global.ensure(nlist), dir.count_global.data(), nlist * 4, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(d_nseg.ensure(nlist), dir.nseg.data(), nlist * 4, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipStreamSynchronize(stream));  // (dir's vectors are stack-owned)
        screen_stale = true;  // rebuilt by the next search (a bulk add appends in many calls)
    }

    // The interleaved arena back from the row-major copy (identical contents: the copy holds
    // every slot of every block, pads included) plus its zeroed slack block.
    void ensure_arena() {
        if (!arena_dropped) return;
        quiesce();
        const size_t vec4 = (size_t)(arena_blocks + 1) * d4 * 64;
        arena.ensure(vec4);
        HIPCHECK(hipMemsetAsync(arena.p + (size_t)arena_blocks * d4 * 64, 0, (size_t)d4 * 64 * sizeof(float4), stream));
        vdbk::launch_interleave(screen_rows.p, arena_blocks * 64, dp, arena.p, stream);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(stream));
        arena_dropped = false;
    }
    // Drop the screen's data (the arena made whole first: the rows may be its only copy).
    void screen_release() {
        ensure_arena();
        screen_ready = false;
        screen_sh.release();
        screen_rows.release();
        screen_meta.release();
        screen_scale.release();
        screen_blist.release();
        screen_ids.release();
        d_sblock_off.release();
        sblocks = 0;
    }

    // (Re)build the screened scan's data from the arena, or drop it. Called by the first
    // search after the lists or centroids change (every search issued before the change
    // was quiesced by it, and none since has read the data) and by the options that
    // decide whether it exists.
    void screen_update() {
        screen_stale = false;
        ensure_arena();  // (the build reads the arena)
        screen_ready = false;
        // (Config::max_gpu_memory caps the resident list bytes, as the reference's
        // gpu_memory_used_ does; the screen's shadow is not list data and is not counted)
        if (tiered()) {
            screen_update_tier();
            return;
        }
        const bool want = screen_opt && metric != 2 && !arena.host && arena_blocks > 0;
        if (!want) {
            screen_release();
            return;
        }
        std::vector<uint32_t> blist(arena_blocks, 0);
        for (uint32_t l = 0; l < nlist; ++l)
            if (owned[l])
                for (uint64_t b = 0; b < list_blocks(l); ++b) blist[block_off[l] + b] = l;
        for (bool i8 = want_i8();; i8 = false) {
            if (i8 != screen_fmt_i8) {  // (a shadow of the other format: its buffers are sized for that)
                screen_sh.release();
                screen_scale.release();
            }
            screen_fmt_i8 = i8;
            try {
                screen_sh.ensure(vdbk::screen_shadow_u4(arena_blocks, d4, i8));
                // (+ one slack block: the exact scans' tile pipeline reads one block past a segment)
                screen_rows.ensure((size_t)(arena_blocks + 1) * 64 * dp);
                screen_meta.ensure((size_t)arena_blocks * 64);
                screen_blist.ensure(arena_blocks);
                if (i8) screen_scale.ensure((size_t)arena_blocks * 64);
            } catch (const VdbError&) {  // no room for it: the exact scan serves
                (void)hipGetLastError();
                screen_release();
                return;
            }
            HIPCHECK(hipMemcpyAsync(screen_blist.p, blist.data(), arena_blocks * 4, hipMemcpyHostToDevice, stream));
            HIPCHECK(hipMemsetAsync(screen_rows.p + (size_t)arena_blocks * 64 * dp, 0, (size_t)64 * dp * 4, stream));
            vdbk::launch_screen_build(arena.p, arena_blocks, d4, screen_blist.p, cent_rm.p, screen_sh.p, screen_rows.p,
                                      screen_meta.p, stream, i8 ? screen_scale.p : nullptr);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(stream));
            screen_ready = true;
            floor.reset_state();  // (trips of a previous shadow say nothing about this one)
            if (!i8 || screen_i8 != 2 || screen_calibrate()) break;
            i8_vetoed = true;  // (the automatic format: int8 re-checks too much here, bf16 instead)
        }
        // the row-major copy is now the lists' fp32 copy: release the arena
        arena.release();
        arena_dropped = true;
    }

    // The automatic shadow format's calibration (option screen_i8 = 2), at the build: one
    // screened batch of (up to) 64 of the index's own vectors (one from each of 64 blocks spread
    // over the lists) as queries, at the nprobe of the search that triggered the build and k = 10.
    // int8 stays unless its survivors beyond k per valid (query, list) pair exceed
    // kCalibPpm of the (query, vector) pairs, or the candidates overflowed: a regime where
    // its ~5x wider bound re-checks more rows than its half-size stream saves (the two-level
    // mixture: 6.2 % and 44.4K vs 52.2K QPS; iid data: 0.3 %, 27.3K vs 25.3K).
    static constexpr uint64_t kCalibPpm = 15000;
    bool screen_calibrate() {
        const uint32_t P = std::min<uint32_t>(nlist, last_P ? last_P : 32), k = 10;
        // (at most one batch's queries at this nprobe: the plan kernel takes kPlanMaxPairs pairs)
        const uint32_t B = std::min<uint32_t>(64, batch_cap(P, k));
        if (!arena_blocks || vdbk::topk_regs(k) != 1) return true;
        DevBuf<float> q, od;
        DevBuf<uint64_t> oi;
        q.ensure((size_t)B * dim);
        od.ensure((size_t)B * k);
        oi.ensure((size_t)B * k);
        for (uint32_t j = 0; j < B; ++j) {  // (slot 0 of a block always holds a vector)
            const uint64_t slot = (uint64_t)(j * arena_blocks / B) * 64;
            HIPCHECK(hipMemcpyAsync(q.p + (size_t)j * dim, screen_rows.p + slot * dp, (size_t)dim * 4,
                                    hipMemcpyDeviceToDevice, stream));
        }
        SearchSlot w;
        ensure_workspace(w, B, P, k);
        if (!stats.p) {
            stats.ensure(16);
            HIPCHECK(hipMemsetAsync(stats.p, 0, 128, stream));
        }
        HIPCHECK(hipMemsetAsync(w.carry_i.p, 0xFF, (size_t)P * k * 8, stream));
        const bool prof0 = prof;
        prof = false;
        calibrating = true;  // (no floor report: the calibration batch never trips the floor)
        try {
            run_batch(w, q.p, B, P, k, od.p, oi.p, stream, nullptr, 0);
        } catch (...) {
            prof = prof0;
            calibrating = false;
            throw;
        }
        prof = prof0;
        calibrating = false;
        uint32_t hc[vdbk::kCounters];
        HIPCHECK(hipMemcpyAsync(hc, w.counters.p, sizeof(hc), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        const uint64_t surv = hc[vdbk::kCtrSurv], pairs = hc[vdbk::kCtrPairs], kvalid = (uint64_t)k * hc[vdbk::kCtrValid];
        const bool overflow = hc[vdbk::kCtrOvf] != 0;
        calib_excess_ppm = pairs ? (surv > kvalid ? surv - kvalid : 0) * 1000000ull / pairs : 0;
        return !overflow && calib_excess_ppm <= kCalibPpm;
    }
    uint64_t calib_excess_ppm = 0;
    bool calibrating = false;

    // The tier's screen: shadow + norms + ids of every stored list in HBM (the deferred scan
    // only: its re-checks read the survivors' rows from the home). Host home: built from the
    // page-locked arena over PCIe. File home: the lists streamed through the io_uring read
    // pipeline once, a group of lists at a time, into a device block buffer, built from there.
    void screen_update_tier() {
        screen_release();
        if (!(screen_opt && screen_defer && metric != 2 && dp % 64 == 0)) return;
        sblock_off.assign(nlist, 0);
        uint64_t nb = 0;
        for (uint32_t l = 0; l < nlist; ++l) {
            if (!owned[l] || count[l] == 0) continue;
            sblock_off[l] = file_home() ? nb : block_off[l];
            nb = std::max<uint64_t>(nb, sblock_off[l] + list_blocks(l));
        }
        if (nb == 0) return;
        std::vector<uint32_t> blist(nb, 0);
        for (uint32_t l = 0; l < nlist; ++l)
            if (owned[l] && count[l])
                for (uint64_t b = 0; b < list_blocks(l); ++b) blist[sblock_off[l] + b] = l;
        const bool i8 = want_i8();
        screen_fmt_i8 = i8;
        try {
            screen_sh.ensure(vdbk::screen_shadow_u4(nb, d4, i8));
            if (i8) screen_scale.ensure((size_t)nb * 64);
            screen_meta.ensure((size_t)nb * 64);
            screen_blist.ensure(nb);
            screen_ids.ensure((size_t)(nb + 1) * 64);
            d_sblock_off.ensure(nlist);
        } catch (const VdbError&) {  // no room: the tier's exact path serves
            (void)hipGetLastError();
            screen_release();
            return;
        }
        HIPCHECK(hipMemcpyAsync(screen_blist.p, blist.data(), nb * 4, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(d_sblock_off.p, sblock_off.data(), nlist * 8, hipMemcpyHostToDevice, stream));
        if (!file_home()) {
            vdbk::launch_screen_build(arena.p, nb, d4, screen_blist.p, cent_rm.p, screen_sh.p, nullptr, screen_meta.p,
                                      stream, i8 ? screen_scale.p : nullptr);
            HIPCHECK(hipMemcpyAsync(screen_ids.p, arena_ids.p, nb * 64 * 8, hipMemcpyHostToDevice, stream));
        } else {
            // groups of consecutive stored lists through a device block buffer of <= 1 GiB
            const uint64_t gcap = std::max<uint64_t>(cdiv(*std::max_element(count.begin(), count.end()), 64),
                                                     (1ull << 30) / ((uint64_t)d4 * 64 * 16 + 512));
            DevBuf<float4> tv;
            DevBuf<uint64_t> ti;
            tv.ensure((gcap + 1) * d4 * 64);
            ti.ensure((gcap + 1) * 64);
            std::vector<std::pair<uint32_t, uint64_t>> loads;
            uint64_t g0 = 0, gend = 0;
            auto flush = [&]() {
                if (loads.empty()) return;
                HIPCHECK(hipMemsetAsync(tv.p, 0, (gend - g0) * d4 * 64 * sizeof(float4), stream));
                load_lists(loads, stream, tv.p, ti.p);
                vdbk::launch_screen_build(tv.p, gend - g0, d4, screen_blist.p + g0, cent_rm.p,
                                          screen_sh.p + g0 * (uint64_t)d4 * (i8 ? 16 : 32), nullptr, screen_meta.p + g0 * 64,
                                          stream, i8 ? screen_scale.p + g0 * 64 : nullptr);
                HIPCHECK(hipGetLastError());
                HIPCHECK(hipMemcpyAsync(screen_ids.p + g0 * 64, ti.p, (gend - g0) * 64 * 8, hipMemcpyDeviceToDevice,
                                        stream));
                HIPCHECK(hipStreamSynchronize(stream));  // (the buffers are refilled by the next group)
                loads.clear();
            };
            for (uint32_t l = 0; l < nlist; ++l) {
                if (!owned[l] || count[l] == 0) continue;
                if (!loads.empty() && sblock_off[l] + list_blocks(l) - g0 > gcap) flush();
                if (loads.empty()) g0 = sblock_off[l];
                loads.push_back({l, sblock_off[l] - g0});
                gend = sblock_off[l] + list_blocks(l);
            }
            flush();
            sblist_host = blist;
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(stream));
        sblocks = nb;
        screen_ready = true;
        if (file_home() && tier_row_cache) fill_row_cache();
    }

    // Screened tier, file home: the k <= 64 searches never use the list cache, so it is filled
    // with lists whose survivors' rows are then copied from HBM instead of read from the
    // file: by default the largest stored lists (on iid data also the most probed); with
    // weights (vdb_ivf_fill_row_cache: per list its expected survivor rows, e.g. the
    // histogram of the batches served so far, vdb_ivf_survivor_histogram) the lists that save
    // the most row reads per cached byte, by weight / length. The lists stay ordinary cached
    // lists: a k > 64 search may evict them.
    std::vector<double> row_cache_weight;  // (empty: by size)
    std::vector<uint64_t> surv_hist;       // per list: survivor rows of the tier's screened batches
    void fill_row_cache() {
        if (!tiered()) return;
        std::vector<uint32_t> order;
        for (uint32_t l = 0; l < nlist; ++l)
            if (owned[l] && count[l] && !lc.resident(l)) order.push_back(l);
        if (row_cache_weight.size() == nlist)
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
                const double wx = row_cache_weight[x] / (double)count[x], wy = row_cache_weight[y] / (double)count[y];
                return wx != wy ? wx > wy : count[x] > count[y];
            });
        else
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return count[x] > count[y]; });
        std::vector<ListCache::Load> loads;
        for (uint32_t l : order) {
            const uint64_t off = lc.place(l, list_blocks(l));
            if (off != ListCache::kAbsent) loads.push_back({l, off});  // (else a smaller list may still fit)
        }
        if (loads.empty()) return;
        load_lists(loads, stream);
        upload_scan_directory(stream);
        HIPCHECK(hipStreamSynchronize(stream));
    }

    // Tier, file home: the survivors' rows of a screened batch, read from the file (or copied
    // from the HBM cache) for the exact re-check. Three steps shared by the one-pass and the
    // two-pass re-check, which differ only in how they lay the rows out:
    //
    // fetch_head: the batch's counters after the deferred scan's selection. False (need: the
    // reserved candidate slots) when the candidate buffer overflowed: the caller re-runs the
    // batch with a larger one. Else the survivors' download is queued on s (fetch_surv).
    bool fetch_head(SearchSlot& w, uint32_t& n, uint32_t& need, hipStream_t s) {
        uint32_t hc[vdbk::kCounters];
        HIPCHECK(hipMemcpyAsync(hc, w.counters.p, sizeof(hc), hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        if (hc[vdbk::kCtrOvf]) {  // (some candidate fell beyond the buffer)
            need = hc[vdbk::kCtrCand];
            return false;
        }
        n = hc[vdbk::kCtrSurv];
        fetch_surv.resize(n);
        if (n) HIPCHECK(hipMemcpyAsync(fetch_surv.data(), w.surv.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        return true;
    }

    // fetch_rows: bring the rows of `want` ({shadow slot, staging row}; `nrows` staging rows)
    // to the slot's device rows row0 .. row0 + nrows, padded to dp (`nsurv`: the batch's
    // survivors, the capacity of the device buffers). A row whose list is in the HBM cache is
    // copied from there (after the upload: it overwrites that row's unused staging content);
    // the others are read from the file in slot order, O_DIRECT (where the file system allows
    // it and option tier_row_direct asks for it) or buffered, so that hot rows stay in the
    // page cache; a slot wanted for several staging rows is read once and copied to the
    // others. Returns the device rows, the stream synchronized (the staging and the cache's
    // contents are reused later).
    std::vector<std::pair<uint64_t, uint32_t>> fetch_want;
    float* fetch_rows(SearchSlot& w, uint32_t row0, uint32_t nrows, uint32_t nsurv, hipStream_t s) {
        const uint64_t row_bytes = (uint64_t)dim * 4;
        cache_src_host.clear();
        std::vector<std::pair<uint64_t, uint32_t>> file;
        file.reserve(fetch_want.size());
        for (const auto& sr : fetch_want) {
            const uint32_t l = sblist_host[sr.first >> 6];
            if (tier_row_cache && lc.resident(l))
                cache_src_host.push_back({(unsigned long long)(row0 + sr.second),
                                          (unsigned long long)(lc.offset(l) * 64 + (sr.first - sblock_off[l] * 64))});
            else
                file.push_back(sr);
        }
        std::sort(file.begin(), file.end());
        std::vector<RowReader::Req> reqs;
        std::vector<std::pair<uint32_t, uint32_t>> dups;  // (staging row, the row its slot was read to)
        reqs.reserve(file.size());
        for (size_t t = 0; t < file.size(); ++t) {
            if (t && file[t].first == file[t - 1].first) {
                dups.push_back({file[t].second, reqs.back().row});
                continue;
            }
            const uint32_t l = sblist_host[file[t].first >> 6];
            reqs.push_back({home.row_offset(l, file[t].first - sblock_off[l] * 64), file[t].second});
        }
        fetch_stage.host = true;
        float* st = fetch_stage.ensure((size_t)std::max<uint32_t>(nrows, 1) * dim);
        const bool direct = tier_row_direct && home_fd_direct >= 0;
        char* bounce = nullptr;
        if (direct) {
            fetch_bounce.host = true;
            bounce = fetch_bounce.ensure(row_reader.bounce_bytes(tier_row_qd, row_bytes));
        }
        try {
            // (with O_DIRECT: the aligned supersets the device delivered)
            file_bytes_read += row_reader.read_rows(home_fd, direct ? home_fd_direct : -1, dio_align, tier_row_qd, row_bytes,
                                                    reqs, (char*)st, bounce);
        } catch (const RowReader::ShortRead& e) {
            throw VdbError(VDB_ERR_STATE, e.what());
        }
        for (const auto& d : dups) std::memcpy(st + (size_t)d.first * dim, st + (size_t)d.second * dim, row_bytes);
        screen_rows_fetched += reqs.size();
        screen_row_bytes += reqs.size() * row_bytes;
        screen_rows_cached += cache_src_host.size();
        float* rows = slot_buf(w, w.srows, (size_t)std::max<uint32_t>(nsurv, 1) * dp);
        if (nrows) {
            if (dim == dp) {
                HIPCHECK(hipMemcpyAsync(rows + (size_t)row0 * dp, st, (size_t)nrows * row_bytes, hipMemcpyHostToDevice, s));
            } else {
                HIPCHECK(hipMemcpyAsync(fetch_dev.ensure((size_t)std::max<uint32_t>(nsurv, 1) * dim), st,
                                        (size_t)nrows * row_bytes, hipMemcpyHostToDevice, s));
                vdbk::launch_pad_rows(fetch_dev.p, nrows, dim, dp, rows + (size_t)row0 * dp, s);
                HIPCHECK(hipGetLastError());
            }
        }
        if (!cache_src_host.empty()) {
            // (a k > 64 call may have loaded lists into the cache asynchronously: its loads end
            // before its last sub-batch, whose completion tier_call_ev marks)
            if (tier_call_used) HIPCHECK(hipEventSynchronize(tier_call_ev));
            const uint32_t nc = (uint32_t)cache_src_host.size();
            HIPCHECK(hipMemcpyAsync(cache_src.ensure(nc), cache_src_host.data(), (size_t)nc * sizeof(ulonglong2),
                                    hipMemcpyHostToDevice, s));
            vdbk::launch_gather_cache_rows(cache.p, d4, cache_src.p, nc, rows, s);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipStreamSynchronize(s));
        return rows;
    }

    // ONE-PASS re-check: one staging row per survivor, indexed by survivor (a row surviving for
    // several queries is read once and copied; from the cache it is gathered once per survivor).
    // Returns the rows ([survivor][dp]) for the exact pass, or nullptr when the candidate
    // buffer overflowed (the caller re-runs the batch with a larger one).
    const float* fetch_survivor_rows(SearchSlot& w, uint32_t& need, hipStream_t s) {
        uint32_t n = 0;
        if (!fetch_head(w, n, need, s)) return nullptr;
        HIPCHECK(hipStreamSynchronize(s));
        if (surv_hist.size() != nlist) surv_hist.assign(nlist, 0);
        fetch_want.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            ++surv_hist[sblist_host[fetch_surv[i].x >> 6]];
            fetch_want[i] = {fetch_surv[i].x, i};
        }
        return fetch_rows(w, 0, n, n, s);
    }

    // TWO-PASS re-check (option screen_recheck2): the rows of the batch's survivors marked
    // `phase` (1: pass A, each pair's k smallest lower bounds; 2: pass B, the others not above
    // pass A's k-th exact distance; launch_tier_recheck) go into the slot's compact device
    // rows, after those of the earlier phase; a row needed again (the same vector surviving for
    // another query, or in both phases) is fetched once. The survivor -> row map is uploaded.
    // Phase 1 returns false (need: the reserved candidate slots) when the candidate buffer
    // overflowed: the caller re-runs the batch with a larger one.
    std::vector<uint8_t> fetch_mark;
    std::vector<uint32_t> fetch_rowmap;
    std::unordered_map<uint64_t, uint32_t> fetch_slot_row;
    uint32_t fetch_n = 0, fetch_rows_n = 0;
    bool fetch_rows_phase(SearchSlot& w, int phase, uint32_t& need, hipStream_t s) {
        if (phase == 1) {
            if (!fetch_head(w, fetch_n, need, s)) return false;
            fetch_rows_n = 0;
            fetch_slot_row.clear();
            fetch_rowmap.assign(fetch_n, 0u);
        }
        const uint32_t n = fetch_n;
        fetch_mark.resize(n);
        if (n) HIPCHECK(hipMemcpyAsync(fetch_mark.data(), w.smark.p, n, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        if (surv_hist.size() != nlist) surv_hist.assign(nlist, 0);
        // this phase's survivors: a slot fetched before maps to its row; new slots get rows j0 ..
        const uint32_t j0 = fetch_rows_n;
        fetch_want.clear();
        for (uint32_t i = 0; i < n; ++i) {
            if (fetch_mark[i] != (uint8_t)phase) continue;
            const uint64_t slot = fetch_surv[i].x;
            ++surv_hist[sblist_host[slot >> 6]];
            const auto ins = fetch_slot_row.emplace(slot, fetch_rows_n);
            fetch_rowmap[i] = ins.first->second;
            if (ins.second) fetch_want.push_back({slot, fetch_rows_n++ - j0});
        }
        if (n) HIPCHECK(hipMemcpyAsync(w.rowmap.p, fetch_rowmap.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        (void)fetch_rows(w, j0, fetch_rows_n - j0, n, s);  // (its closing sync covers the map's upload)
        return true;
    }

    // Rebuild the arena so list l holds `keep[l]` of its current blocks at new
    // offsets sized for `new_count[l]` vectors (0 for lists this handle drops).
    void relayout(const std::vector<uint64_t>& new_count, const std::vector<uint8_t>& new_owned) {
        relayout(new_count, new_owned, arena.host);
    }
    void relayout(const std::vector<uint64_t>& new_count, const std::vector<uint8_t>& new_owned, bool host_arena) {
        quiesce();
        // the screen's data describes the old lists: drop it before the new arena is
        // allocated (peak HBM old + new arena, not that plus the shadow and rows); the next
        // search rebuilds it
        screen_release();
        screen_stale = true;
        std::vector<uint64_t> new_off(nlist, 0), old_off(nlist, 0);
        std::vector<uint32_t> nblocks(nlist, 0);
        uint64_t blocks = 0;
        for (uint32_t l = 0; l < nlist; ++l) {
            new_off[l] = blocks;
            if (new_owned[l]) blocks += cdiv(new_count[l], 64);
            if (owned[l] && new_owned[l] && count[l] > 0) {
                nblocks[l] = (uint32_t)cdiv(count[l], 64);
                old_off[l] = block_off[l];
            }
        }
        DevBuf<float4> na{!host_arena};
        DevBuf<uint64_t> ni{!host_arena};
        na.host = ni.host = host_arena;
        // one slack block past the last list: the scan prefetches one chunk and one
        // block of ids beyond the segment it streams
        const size_t vec4 = (size_t)(blocks + 1) * d4 * 64;
        na.ensure(vec4);
        ni.ensure((size_t)(blocks + 1) * 64);
        if (blocks) {
            HIPCHECK(hipMemsetAsync(na.p, 0, vec4 * sizeof(float4), stream));
            HIPCHECK(hipMemsetAsync(ni.p, 0xFF, (size_t)(blocks + 1) * 64 * 8, stream));
        }
        if (arena_blocks && blocks) {
            DevBuf<uint64_t> doo, dno;
            DevBuf<uint32_t> dnb;
            HIPCHECK(hipMemcpyAsync(doo.ensure(nlist), old_off.data(), nlist * 8, hipMemcpyHostToDevice, stream));
            HIPCHECK(hipMemcpyAsync(dno.ensure(nlist), new_off.data(), nlist * 8, hipMemcpyHostToDevice, stream));
            HIPCHECK(hipMemcpyAsync(dnb.ensure(nlist), nblocks.data(), nlist * 4, hipMemcpyHostToDevice, stream));
            vdbk::launch_copy_lists(arena.p, arena_ids.p, doo.p, dno.p, dnb.p, nlist, d4, na.p, ni.p, stream);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(stream));
        }
        HIPCHECK(hipStreamSynchronize(stream));
        arena.swap(na);
        arena_ids.swap(ni);
        arena_blocks = blocks;
        block_off = new_off;
        owned = new_owned;
        lc.reset(nlist, lc.capacity());  // list contents or offsets changed: nothing cached stays valid
    }

    // ---- list-cache tier ----
    bool tiered() const { return lc.capacity() > 0; }
    uint64_t list_blocks(uint32_t l) const { return cdiv(count[l], 64); }
    static uint64_t block_bytes(uint32_t dp_) { return 64ull * ((uint64_t)dp_ * 4 + 8); }

    ListSizes list_sizes() const { return ListSizes{count, owned}; }

    // Scan directory: home offsets, or cache offsets in the tier (absent lists: 0,
    // never read: a list is made resident before any batch that probes it is planned).
    void upload_scan_directory(hipStream_t s) {
        const uint64_t* src = block_off.data();
        if (tiered()) {
            // the previous upload's source must have been read before it is rewritten
            if (tier_ev_used) HIPCHECK(hipEventSynchronize(tier_ev));
            dir_stage.host = true;
            uint64_t* st = dir_stage.ensure(nlist);
            for (uint32_t l = 0; l < nlist; ++l) st[l] = lc.resident(l) ? lc.offset(l) : 0;
            src = st;
        }
        HIPCHECK(hipMemcpyAsync(d_block_off.ensure(nlist), src, nlist * 8, hipMemcpyHostToDevice, s));
        if (!tiered()) {
            HIPCHECK(hipStreamSynchronize(s));  // src is the host vector
            return;
        }
        if (!tier_ev) HIPCHECK(hipEventCreateWithFlags(&tier_ev, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(tier_ev, s));  // covers the loads queued on s before it
        tier_ev_used = true;
    }

    // Make `lists` resident on stream s (warmup and single lists): LRU eviction.
    // False if together they exceed the cache.
    bool make_resident(const uint32_t* lists, size_t n, hipStream_t s) {
        const ListSizes sz = list_sizes();
        std::vector<uint8_t> mark(nlist, 0);
        const std::vector<uint32_t> want = sz.unique(lists, n, mark);
        lc.touch(want);
        std::vector<uint8_t> protect(nlist, 0);
        for (uint32_t l : want) protect[l] = 1;
        bool miss = false;
        for (uint32_t l : want) miss |= !lc.resident(l);
        if (miss) quiesce();  // searches on other streams may still read the lists evicted below
        std::vector<ListCache::Load> loads;
        if (!lc.plan_loads(want, protect, sz, [](uint32_t) { return uint64_t(0); }, true, loads)) return false;
        if (loads.empty()) return true;
        load_lists(loads, s);
        upload_scan_directory(s);
        return true;
    }

    bool file_home() const { return home_fd >= 0; }

    void pread_all(void* dst, size_t bytes, uint64_t off) {
        pread_exact(home_fd, dst, bytes, off);
        file_bytes_read += bytes;
    }

    // Copy planned lists into their cache blocks, ordered on stream s. Host-memory home:
    // one DMA per list. File home: every list is cut into chunks of whole 64-row blocks;
    // each chunk's ids and rows are read (io_uring, up to kStages chunks in flight) into
    // a page-locked staging buffer, copied to HBM, padded to dp and interleaved into the
    // cache's block layout; a buffer is refilled once its copies have landed.
    void load_lists(const std::vector<ListCache::Load>& loads, hipStream_t s,
                    float4* dst_v = nullptr, uint64_t* dst_i = nullptr) {
        float4* const tv = dst_v ? dst_v : cache.p;  // (the cache, or a caller's block buffer)
        uint64_t* const ti = dst_i ? dst_i : cache_ids.p;
        if (!file_home()) {
            for (auto& ld : loads) {
                const uint32_t l = ld.first;
                const uint64_t off = ld.second, nb = list_blocks(l);
                HIPCHECK(hipMemcpyAsync(tv + off * d4 * 64, arena.p + block_off[l] * d4 * 64,
                                        nb * d4 * 64 * sizeof(float4), hipMemcpyHostToDevice, s));
                HIPCHECK(hipMemcpyAsync(ti + off * 64, arena_ids.p + block_off[l] * 64, nb * 64 * 8,
                                        hipMemcpyHostToDevice, s));
            }
            return;
        }
        const uint64_t rows = std::max<uint64_t>(64, ((32ull << 20) / ((uint64_t)dim * 4)) / 64 * 64);
        const size_t ids_cap = (rows * 8 + 8192 + 4095) / 4096 * 4096;
        const size_t vec_cap = (rows * dim * 4 + 8192 + 4095) / 4096 * 4096;
        if (!uring) uring.reset(new UringReader(64));
        for (Stage& st : stages) {
            if (!st.copied) HIPCHECK(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
            st.buf.host = true;
            st.buf.ensure(ids_cap + vec_cap);
        }
        // loads on the copy stream may overlap loads on a search stream: separate device staging
        DevBuf<float>& rows_d = s == copy_stream ? drows_cs : drows;
        DevBuf<float>& pad_d = s == copy_stream ? dpad_cs : dpad;
        rows_d.ensure(rows * dim);
        pad_d.ensure(rows * dp);
        struct Chunk {
            uint32_t l;
            uint64_t r0, m, dst_block;
        };
        std::vector<Chunk> chunks;
        for (auto& ld : loads)
            for (uint64_t r0 = 0; r0 < count[ld.first]; r0 += rows)
                chunks.push_back({ld.first, r0, std::min(rows, count[ld.first] - r0), ld.second + r0 / 64});
        const bool direct = home_fd_direct >= 0;
        // one read; with O_DIRECT the aligned superset of [off, off + len)
        auto read_into = [&](int si, char* dst, uint64_t off, uint64_t len, int part) -> size_t {
            const uint64_t tag = ((uint64_t)si << 1) | (uint64_t)part;
            if (!direct) {
                uring->read(home_fd, dst, (uint32_t)len, off, tag);
                return 0;
            }
            uint64_t a0, a1;
            aligned_superset(off, len, 4096, a0, a1);
            uring->read(home_fd_direct, dst, (uint32_t)(a1 - a0), a0, tag);
            return (size_t)(off - a0);
        };
        size_t next = 0;
        int reading = 0;
        try {
            while (next < chunks.size() || reading > 0) {
                for (int si = 0; si < kStages && next < chunks.size(); ++si) {
                    Stage& st = stages[si];
                    if (st.reads) continue;
                    if (st.copying) {
                        const hipError_t q = hipEventQuery(st.copied);
                        if (q == hipErrorNotReady) continue;
                        HIPCHECK(q);
                        st.copying = false;
                    }
                    const Chunk& c = chunks[next++];
                    st.m = c.m;
                    st.dst_block = c.dst_block;
                    st.ids_delta = read_into(si, st.buf.p, home.ids_offset(c.l, c.r0), c.m * 8, 0);
                    st.vec_delta = read_into(si, st.buf.p + ids_cap, home.row_offset(c.l, c.r0), c.m * dim * 4, 1);
                    st.reads = 2;
                    ++reading;
                    file_bytes_read += c.m * 8 + c.m * dim * 4;
                }
                if (reading == 0) {  // every buffer waits for its copies: wait for one
                    for (Stage& st : stages)
                        if (st.copying) {
                            HIPCHECK(hipEventSynchronize(st.copied));
                            st.copying = false;
                            break;
                        }
                    continue;
                }
                for (const UringReader::Done& d : uring->wait(1)) {
                    Stage& st = stages[d.tag >> 1];
                    const bool vec = d.tag & 1;
                    const int64_t want = (int64_t)((vec ? st.vec_delta : st.ids_delta) + st.m * (vec ? (uint64_t)dim * 4 : 8));
                    require(d.result >= want, "short read from the list file" +
                                                  (d.result < 0 ? std::string(": ") + std::strerror((int)-d.result) : ""),
                            VDB_ERR_STATE);
                    if (--st.reads) continue;
                    --reading;
                    HIPCHECK(hipMemcpyAsync(ti + st.dst_block * 64, st.buf.p + st.ids_delta, st.m * 8,
                                            hipMemcpyHostToDevice, s));
                    HIPCHECK(hipMemcpyAsync(rows_d.p, st.buf.p + ids_cap + st.vec_delta, st.m * dim * 4,
                                            hipMemcpyHostToDevice, s));
                    HIPCHECK(hipEventRecord(st.copied, s));
                    st.copying = true;
                    vdbk::launch_pad_rows(rows_d.p, st.m, dim, dp, pad_d.p, s);
                    vdbk::launch_interleave(pad_d.p, st.m, dp, tv + st.dst_block * d4 * 64, s);
                    HIPCHECK(hipGetLastError());
                }
            }
        } catch (...) {
            // A failed read (or submission) leaves other reads in flight: reap them and
            // reset the staging ring, and forget the cache map (the lists planned for this
            // load may be partly written), so the next load starts clean.
            uring->drain();
            for (Stage& st : stages) st.reads = 0;
            lc.reset(nlist, lc.capacity());
            throw;
        }
    }

    // Serve the lists from an index file (vdb_ivf_save format) through the tier.
    void open_lists(const char* path) {
        require(tiered(), "open_lists needs the list-cache tier (set list_cache_bytes first)", VDB_ERR_STATE);
        quiesce();
        // All or nothing: the file is opened, read and judged through locals, so a refusal or
        // a read error closes them and leaves the handle serving what it served before.
        IndexFileFd f(path);
        require(f.fd >= 0, std::string("cannot open ") + path, VDB_ERR_STATE);
        // lists are read with O_DIRECT where the file system allows it (no page-cache copy)
        IndexFileFd fdirect(path, O_DIRECT);
        uint32_t align = 4096;
        if (fdirect.fd >= 0) {  // (a 512-B read at a 512-B offset: accepted or EINVAL)
            void* pb = nullptr;
            if (posix_memalign(&pb, 4096, 4096) == 0) {
                if (::pread(fdirect.fd, pb, 512, 512) == 512) align = 512;
                std::free(pb);
            }
        }
        IndexFileDirectory d;
        index_file_checked([&] {
            const IndexFileHeader hd = read_index_file_header(f, f.size);
            require(!(hd.shard && unit_rows), "opening a shard file is not available with VDB_METRIC_COSINE_DISTANCE",
                    VDB_ERR_UNSUPPORTED);
            hd.require_config(dim, nlist, config_metric());
            d = read_index_file_lists(hd, f, f.size);
        });
        std::vector<float> c((size_t)nlist * dim);
        f(d.centroids_off, c.data(), d.centroid_bytes());
        // accepted: the handle's old home goes (the locals close it), everything is replaced
        std::swap(home_fd, f.fd);
        std::swap(home_fd_direct, fdirect.fd);
        dio_align = align;
        file_bytes_read += f.bytes_read;
        HIPCHECK(hipMemcpy2DAsync(cent_rm.p, dp * 4, c.data(), dim * 4, dim * 4, nlist, hipMemcpyHostToDevice, stream));
        refresh_centroid_layout();
        total = 0;
        for (uint32_t l = 0; l < nlist; ++l) {
            count[l] = d.lists[l].count;
            owned[l] = d.owned(l);
            total += count[l];
        }
        rank = d.header.rank;
        world = d.header.world;
        home = std::move(d);
        screen_ready = false;  // (everything is replaced: no arena rebuild for the old lists)
        arena_dropped = false;
        screen_sh.release();
        screen_rows.release();
        screen_meta.release();
        screen_blist.release();
        arena.release();  // no home copy in memory: the file is the home
        arena_ids.release();
        arena_blocks = 0;
        block_off.assign(nlist, 0);
        lc.reset(nlist, lc.capacity());
        upload_directory();
    }

    // Turn the tier on (bytes > 0: HBM cache of that many bytes, arena moved to host
    // memory) or off (arena back in HBM).
    void set_list_cache(uint64_t bytes) {
        quiesce();
        const uint64_t nb = bytes / block_bytes(dp);
        require(bytes == 0 || nb > 0, "list_cache_bytes is below one block of 64 vectors");
        require(nb > 0 || !file_home(), "lists served from a file need the list-cache tier", VDB_ERR_STATE);
        cache.release();
        cache_ids.release();
        lc.reset(nlist, 0);
        if (!file_home() && (nb > 0) != arena.host) relayout(count, owned, nb > 0);  // moves the arena
        if (nb) {  // one slack block: the scan prefetches past a segment's end
            cache.ensure((nb + 1) * d4 * 64);
            cache_ids.ensure((nb + 1) * 64);
        }
        lc.reset(nlist, nb);
        upload_directory();
    }

    // Config::max_gpu_memory: the reference caps the bytes of GPU-resident lists
    // (count * (dim * 4 + 8) each, gpu_memory_used_) and searches lists beyond the cap on
    // the CPU (ivf_flat_index.cpp:398-402, 526-530). Here, once the stored lists outgrow
    // the cap, the handle switches to the list-cache tier with an HBM cache of that many
    // bytes: lists home in page-locked host memory and the lists a batch probes are made
    // resident before it scans, so results are unchanged. 0 = no cap.
    uint64_t stored_list_bytes(const std::vector<uint64_t>& cnt) const {
        uint64_t b = 0;
        for (uint32_t l = 0; l < nlist; ++l)
            if (owned[l]) b += cnt[l] * ((uint64_t)dim * 4 + 8);
        return b;
    }
    bool tier_by_cap = false;  // the tier was entered because the lists outgrew max_gpu_memory
    void apply_memory_cap(const std::vector<uint64_t>& cnt) {
        if (file_home()) return;
        if (tier_by_cap && (max_gpu_memory == 0 || stored_list_bytes(cnt) <= max_gpu_memory)) {
            set_list_cache(0);  // the cap was lifted or raised above the lists: back to HBM
            tier_by_cap = false;
            return;
        }
        if (max_gpu_memory == 0 || max_gpu_memory == ~0ull || tiered()) return;
        if (stored_list_bytes(cnt) <= max_gpu_memory) return;
        require(max_gpu_memory >= block_bytes(dp),
                "max_gpu_memory is below one block of 64 vectors (set 0 for no cap)", VDB_ERR_OUT_OF_MEMORY);
        set_list_cache(max_gpu_memory);
        tier_by_cap = true;
    }

    // Row-major [n][dim] device input -> zero-padded [n][dp] (or the input itself). With
    // unit_rows: the unit rows, always in tmp (the caller's buffer is never written).
    const float* padded_rows(const float* d_v, uint64_t n, DevBuf<float>& tmp) {
        if (unit_rows && !ingest_stored) {
            vdbk::launch_unit_rows(d_v, n, dim, dp, tmp.ensure(n * dp), stream);
            HIPCHECK(hipGetLastError());
            return tmp.p;
        }
        if (dp == dim) return d_v;
        vdbk::launch_pad_rows(d_v, n, dim, dp, tmp.ensure(n * dp), stream);
        HIPCHECK(hipGetLastError());
        return tmp.p;
    }

    // Caller holds mu. Host centroids [nlist][dim] in (zero pads kept).
    void set_centroids_host(const float* c) {
        quiesce();
        HIPCHECK(hipMemcpy2DAsync(cent_rm.p, dp * 4, c, dim * 4, dim * 4, nlist, hipMemcpyHostToDevice, stream));
        refresh_centroid_layout();
        HIPCHECK(hipStreamSynchronize(stream));
    }

    // Caller holds mu. Append host rows to the given lists (input order per list).
    void add_to_lists_host(const float* v, const uint64_t* ids, const uint32_t* lists, uint64_t n) {
        if (n == 0) return;
        for (uint64_t i = 0; i < n; ++i) require(lists[i] < nlist, "list id out of range");
        DevBuf<float> dv, tmp;
        DevBuf<uint64_t> di;
        DevBuf<uint32_t> dl;
        HIPCHECK(hipMemcpyAsync(dv.ensure(n * dim), v, n * dim * 4, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(di.ensure(n), ids, n * 8, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(dl.ensure(n), lists, n * 4, hipMemcpyHostToDevice, stream));
        append(padded_rows(dv.p, n, tmp), di.p, dl.p, n);
        HIPCHECK(hipStreamSynchronize(stream));
    }

    // Caller holds mu. Centroids row-major [nlist][dim] into host memory.
    void export_centroids(float* c) {
        HIPCHECK(hipMemcpy2DAsync(c, dim * 4, cent_rm.p, dp * 4, dim * 4, nlist, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }

    // Caller holds mu. List l row-major (count x dim) with its ids, in add order.
    void export_list(uint32_t l, float* vectors, uint64_t* ids) {
        const uint64_t c = count[l];
        if (c == 0) return;
        require(owned[l], "list is not stored on this shard", VDB_ERR_STATE);
        if (file_home()) {  // the file holds the list row-major, as returned
            if (ids) pread_all(ids, c * 8, home.ids_offset(l, 0));
            if (vectors) pread_all(vectors, c * dim * 4, home.row_offset(l, 0));
            return;
        }
        if (arena_dropped) {  // the row-major copy holds the list in slot (= add) order
            if (vectors)
                HIPCHECK(hipMemcpy2DAsync(vectors, (size_t)dim * 4, screen_rows.p + block_off[l] * 64 * dp, (size_t)dp * 4,
                                          (size_t)dim * 4, c, hipMemcpyDeviceToHost, stream));
            if (ids) HIPCHECK(hipMemcpyAsync(ids, arena_ids.p + block_off[l] * 64, c * 8, hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            return;
        }
        DevBuf<float> dv;
        DevBuf<uint64_t> di;
        vdbk::launch_export_list(arena.p, arena_ids.p, block_off[l], (uint32_t)c, dim, d4, dv.ensure(c * dim),
                                 di.ensure(c), stream);
        HIPCHECK(hipGetLastError());
        if (vectors) HIPCHECK(hipMemcpyAsync(vectors, dv.p, c * dim * 4, hipMemcpyDeviceToHost, stream));
        if (ids) HIPCHECK(hipMemcpyAsync(ids, di.p, c * 8, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }

    void refresh_centroid_layout() {
        quiesce();
        vdbk::launch_interleave(cent_rm.p, nlist, dp, cent_il.p, stream);
        HIPCHECK(hipGetLastError());
        screen_stale = true;  // the shadow holds residuals against the centroids
    }

    // assign_to_lists (cpp:259-295): exact argmin with ties to the lowest centroid. For
    // L2 / IP it is the coarse step's top-1: MFMA distance bounds, then the exact
    // sequential distances of every centroid that can still be the minimum
    // (ivf_assign_rerank: candidates whose lower bound <= the smallest upper bound; NaN
    // orders last, so an all-NaN row goes to list 0 as with the strict '<').
    // Rows are processed in chunks whose bound matrices fit a fixed workspace.
    void assign(const float* vpad, uint64_t n, uint32_t* out) {
        if (coarse_mode == 1 && metric != 2 && vdbk::rerank_rows(dp, 1) > 0) {
            const uint64_t budget = 1024ull << 20;  // bytes of the two bound matrices per chunk
            uint64_t chunk = std::max<uint64_t>(256, budget / ((uint64_t)nlist * 8) / 16 * 16);
            chunk = std::min<uint64_t>(chunk, n);
            DevBuf<float> ap, de;
            ap.ensure(chunk * nlist);
            de.ensure(chunk * nlist);
            for (uint64_t r0 = 0; r0 < n; r0 += chunk) {
                const uint32_t b = (uint32_t)std::min<uint64_t>(chunk, n - r0);
                vdbk::launch_coarse_mfma(metric, cent_rm.p, nlist, dp, vpad + r0 * dp, b, ap.p, de.p, stream);
                vdbk::launch_assign_rerank(metric, ap.p, de.p, cent_rm.p, nlist, dp, vpad + r0 * dp, b, out + r0, stream);
                HIPCHECK(hipGetLastError());
            }
            HIPCHECK(hipStreamSynchronize(stream));  // the chunk buffers are freed on return
            return;
        }
        vdbk::launch_assign(metric, vpad, n, dp, cent_il.p, nlist, out, stream);
        HIPCHECK(hipGetLastError());
    }

    // Stable grouping of row indices by key (input order kept within a key).
    void group_by_key(const uint32_t* keys, uint64_t n, DevBuf<uint32_t>& sorted_keys, DevBuf<uint32_t>& order) {
        require(n < (1ull << 31), "batch larger than 2^31 vectors", VDB_ERR_UNSUPPORTED);
        DevBuf<uint32_t> iota;
        vdbk::launch_iota(iota.ensure(n), n, stream);
        int bits = 1;
        while ((1ull << bits) < nlist) ++bits;
        size_t tb = 0;
        HIPCHECK(vdbk::radix_sort_pairs(nullptr, tb, keys, sorted_keys.ensure(n), iota.p, order.ensure(n), n, bits, stream));
        DevBuf<unsigned char> temp;
        temp.ensure(tb);
        HIPCHECK(vdbk::radix_sort_pairs(temp.p, tb, keys, sorted_keys.p, iota.p, order.p, n, bits, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }

    std::vector<uint32_t> key_counts(const uint32_t* keys, uint64_t n, DevBuf<uint32_t>& d_counts) {
        HIPCHECK(hipMemsetAsync(d_counts.ensure(nlist), 0, nlist * 4, stream));
        vdbk::launch_histogram(keys, n, d_counts.p, stream);
        HIPCHECK(hipGetLastError());
        std::vector<uint32_t> h(nlist);
        HIPCHECK(hipMemcpyAsync(h.data(), d_counts.p, nlist * 4, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        return h;
    }

    // ---- train: ivf_flat_index.cpp:49-145 ----
    void train(const float* d_v, uint64_t n) {
        require(n > 0, "train needs at least one vector");
        DevBuf<float> tmp, mind;
        const float* vpad = padded_rows(d_v, n, tmp);
        DevBuf<float4> v_il;
        vdbk::launch_interleave(vpad, n, dp, v_il.ensure(cdiv(n, 64) * d4 * 64), stream);
        HIPCHECK(hipGetLastError());

        std::mt19937 gen(42);
        std::uniform_int_distribution<uint64_t> pick(0, n - 1);
        const uint64_t first = pick(gen);
        HIPCHECK(hipMemcpyAsync(cent_rm.p, vpad + first * dp, dp * 4, hipMemcpyDeviceToDevice, stream));

        vdbk::launch_mindist_init(mind.ensure(n), n, stream);
        // The min-distance update (n x dim work) runs on the device; the two serial
        // float sums of cpp:87 and cpp:95-96 (n dependent adds each, inherently
        // sequential) run on the host over a pinned copy, in the reference's order.
        PinnedBuf<float> hmind(n);
        for (uint32_t c = 1; c < nlist; ++c) {
            vdbk::launch_mindist_update(v_il.p, n, d4, cent_rm.p + (size_t)(c - 1) * dp, mind.p, stream);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(hmind.p, mind.p, n * sizeof(float), hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            const float* md = hmind.p;
            float tot = 0.0f;
            for (uint64_t v = 0; v < n; ++v) tot += md[v];
            std::uniform_real_distribution<float> prob(0.0f, tot);
            const float target = prob(gen);
            float cumsum = 0.0f;
            for (uint64_t v = 0; v < n; ++v) {
                cumsum += md[v];
                if (cumsum >= target) {
                    HIPCHECK(hipMemcpyAsync(cent_rm.p + (size_t)c * dp, vpad + v * dp, dp * sizeof(float),
                                            hipMemcpyDeviceToDevice, stream));
                    break;
                }
            }
        }

        DevBuf<uint32_t> asg, skeys, order, counts, offsets;
        asg.ensure(n);
        for (int it = 0; it < 10; ++it) {
            refresh_centroid_layout();
            assign(vpad, n, asg.p);
            group_by_key(asg.p, n, skeys, order);
            std::vector<uint32_t> h = key_counts(asg.p, n, counts);
            std::vector<uint32_t> off(nlist, 0);
            for (uint32_t l = 1; l < nlist; ++l) off[l] = off[l - 1] + h[l - 1];
            HIPCHECK(hipMemcpyAsync(offsets.ensure(nlist), off.data(), nlist * 4, hipMemcpyHostToDevice, stream));
            vdbk::launch_centroid_update(vpad, dp, order.p, offsets.p, counts.p, nlist, dim, cent_rm.p, stream);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(stream));
        }
        if (unit_rows) {
            // spherical k-means' last step: the final centroids to unit length, by the rows'
            // kernel (the +0 pads add nothing to a sum: the bits are those of the dim-long row);
            // a zero centroid stays zero
            DevBuf<float> cu;
            vdbk::launch_unit_rows(cent_rm.p, nlist, dp, dp, cu.ensure((size_t)nlist * dp), stream);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(cent_rm.p, cu.p, (size_t)nlist * dp * 4, hipMemcpyDeviceToDevice, stream));
            HIPCHECK(hipStreamSynchronize(stream));  // (cu goes on return)
        }
        refresh_centroid_layout();
        HIPCHECK(hipStreamSynchronize(stream));
    }

    // ---- add: ivf_flat_index.cpp:148-202 ----
    void add(const float* d_v, const uint64_t* d_ids, uint64_t n) {
        if (n == 0) return;
        require(!file_home(), "lists are served from a file (vdb_ivf_open_lists): the index is read-only",
                VDB_ERR_STATE);
        DevBuf<float> tmp;
        const float* vpad = padded_rows(d_v, n, tmp);
        DevBuf<uint32_t> asg;
        assign(vpad, n, asg.ensure(n));
        append(vpad, d_ids, asg.p, n);
    }

    // Append rows to the given lists, keeping input order within each list
    // (cpp:160-192). `asg` holds one list id per row (device).
    void append(const float* vpad, const uint64_t* d_ids, const uint32_t* asg, uint64_t n) {
        require(!file_home(), "lists are served from a file (vdb_ivf_open_lists): the index is read-only",
                VDB_ERR_STATE);
        DevBuf<uint32_t> skeys, order, counts;
        group_by_key(asg, n, skeys, order);
        std::vector<uint32_t> added = key_counts(asg, n, counts);

        std::vector<uint64_t> new_count(count);
        for (uint32_t l = 0; l < nlist; ++l) new_count[l] += added[l];
        const std::vector<uint64_t> old_count = count;
        apply_memory_cap(new_count);  // (before the relayout: the arena moves home at most once)
        relayout(new_count, owned);

        std::vector<uint64_t> group_start(nlist, 0), base(nlist, ~0ull);
        for (uint32_t l = 1; l < nlist; ++l) group_start[l] = group_start[l - 1] + added[l - 1];
        for (uint32_t l = 0; l < nlist; ++l)
            if (owned[l]) base[l] = block_off[l] * 64 + old_count[l];
        DevBuf<uint64_t> d_gs, d_base, dest;
        HIPCHECK(hipMemcpyAsync(d_gs.ensure(nlist), group_start.data(), nlist * 8, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(d_base.ensure(nlist), base.data(), nlist * 8, hipMemcpyHostToDevice, stream));
        vdbk::launch_slots_from_order(skeys.p, n, d_gs.p, d_base.p, dest.ensure(n), stream);
        vdbk::launch_scatter_rows(vpad, d_ids, order.p, n, dp, dest.p, arena.p, arena_ids.p, stream);
        HIPCHECK(hipGetLastError());
        count = new_count;
        total += n;
        upload_directory();  // also waits for the stream before tmp buffers go
    }

    // owner: the plan (every list's rank), identical on every rank; null = the LPT plan
    // of vdb_shard_plan over the current list sizes.
    void set_shard(uint32_t r, uint32_t w, const uint32_t* owner_in = nullptr) {
        std::vector<uint32_t> owner(nlist);
        if (owner_in) std::copy(owner_in, owner_in + nlist, owner.begin());
        else vdb_shard_plan(count.data(), nlist, w, owner.data());
        std::vector<uint8_t> new_owned(nlist);
        for (uint32_t l = 0; l < nlist; ++l) {
            require(owner[l] < w, "shard plan names a rank outside the world");
            new_owned[l] = owner[l] == r;
        }
        // Lists this handle no longer scans must have been stored here before.
        for (uint32_t l = 0; l < nlist; ++l)
            require(!new_owned[l] || owned[l] || count[l] == 0, "shard needs a list this handle dropped", VDB_ERR_STATE);
        if (file_home()) {  // nothing in memory to move: the file holds every list
            quiesce();
            owned = new_owned;
            lc.reset(nlist, lc.capacity());
        } else {
            relayout(count, new_owned);
        }
        rank = r;
        world = w;
        upload_directory();
    }

    // Group member: store exactly the lists `new_owned` marks (placement by the group).
    // A list may only move here while empty; lists leaving are dropped.
    void set_owned(const std::vector<uint8_t>& new_owned) {
        for (uint32_t l = 0; l < nlist; ++l)
            require(!new_owned[l] || owned[l] || count[l] == 0, "a placed list cannot move between members",
                    VDB_ERR_STATE);
        if (new_owned == owned) return;
        relayout(count, new_owned);
        upload_directory();
    }

    // Sharded build, for an index larger than one GPU (100M x 768 = 307 GB): the final
    // list sizes (from an assignment pass) fix this handle's lists before any add, so
    // appends store only the owned lists' rows and count the rest. The plan is the same
    // LPT as set_shard, so a later set_shard(r, w) keeps the same lists.
    void plan_shard(uint32_t r, uint32_t w, const uint64_t* final_sizes, const uint32_t* owner_in = nullptr) {
        require(total == 0, "plan_shard needs an empty index (call it between train and add)", VDB_ERR_STATE);
        require(!file_home(), "lists are served from a file (vdb_ivf_open_lists)", VDB_ERR_STATE);
        std::vector<uint32_t> owner(nlist);
        if (owner_in) std::copy(owner_in, owner_in + nlist, owner.begin());
        else vdb_shard_plan(final_sizes, nlist, w, owner.data());
        std::vector<uint8_t> new_owned(nlist);
        for (uint32_t l = 0; l < nlist; ++l) {
            require(owner[l] < w, "shard plan names a rank outside the world");
            new_owned[l] = owner[l] == r;
        }
        relayout(count, new_owned);
        rank = r;
        world = w;
        upload_directory();
    }

    // Probe census for a probe-weighted shard plan: counts[l] += how many of the n device
    // rows (a query-like sample) probe list l, by the exact probe selection of search.
    void probe_census(const float* d_rows, uint64_t n, uint32_t nprobe, uint64_t* counts) {
        const uint32_t P = std::min(nprobe, nlist);
        if (n == 0 || P == 0) return;
        quiesce();
        SearchSlot w;
        const uint32_t bmax = batch_cap(P, 1);
        ensure_workspace(w, (uint32_t)std::min<uint64_t>(bmax, n), P, 1);
        DevBuf<uint32_t> d_counts;
        HIPCHECK(hipMemsetAsync(d_counts.ensure(nlist), 0, nlist * 4, stream));
        for (uint64_t b0 = 0; b0 < n; b0 += bmax) {
            const uint32_t B = (uint32_t)std::min<uint64_t>(bmax, n - b0);
            coarse_batch(w, d_rows + b0 * dim, B, P, stream);
            vdbk::launch_histogram(w.probes.p, (uint64_t)B * P, d_counts.p, stream);
            HIPCHECK(hipGetLastError());
        }
        std::vector<uint32_t> h(nlist);
        HIPCHECK(hipMemcpyAsync(h.data(), d_counts.p, nlist * 4, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        for (uint32_t l = 0; l < nlist; ++l) counts[l] += h[l];
    }

    EventSet& next_events() {
        if (events_used == events.size()) {
            EventSet e;
            for (hipEvent_t* p : {&e.begin, &e.coarse_end, &e.scan_begin, &e.scan_end, &e.end, &e.x_end, &e.m_end,
                                  &e.collect_begin, &e.collect_end})
                HIPCHECK(hipEventCreate(p));
            events.push_back(e);
        }
        events[events_used].xchg = false;
        events[events_used].collected = false;
        return events[events_used++];
    }

    // Size every per-batch buffer of a slot for B queries up front; growing a buffer
    // frees the old one, so first wait for the slot's previous batch.
    void ensure_workspace(SearchSlot& w, uint32_t B, uint32_t P, uint32_t k) {
        const ScanBounds bd = scan_bounds(kScanConsts, nseg_prefix, B, P);  // (what scan_batch launches by)
        const size_t BP = bd.BP, max_items = bd.max_items, max_l1 = bd.max_l1, max_wide = bd.max_wide;
        const bool grow = w.items_w.cap < max_wide || w.qpad.cap < (size_t)B * dp || w.cd.cap < (size_t)B * nlist ||
                          w.cdelta.cap < (size_t)B * nlist || w.cand.cap < (size_t)B * nlist ||
                          w.probes.cap < BP || w.thr.cap < BP || w.items.cap < max_items || w.part_d.cap < max_items * k ||
                          w.slot_d.cap < BP * k || w.carry_d.cap < (size_t)P * k || w.carry2_d.cap < (size_t)P * k ||
                          w.l1_items.cap < max_l1 ||
                          w.l1_d.cap < max_l1 * k;
        if (!grow) return;
        if (w.used) HIPCHECK(hipEventSynchronize(w.done));
        w.qpad.ensure((size_t)B * dp);
        w.cd.ensure((size_t)B * nlist);
        w.cdelta.ensure((size_t)B * nlist);
        w.cand.ensure((size_t)B * nlist);
        w.probes.ensure(BP);
        w.nseg_qp.ensure(BP);
        w.pbqp.ensure(BP);
        w.sorted_pair.ensure(BP);
        w.pbs.ensure(BP);
        w.counters.ensure(vdbk::kCounters);
        w.l1base.ensure(BP);
        w.thr.ensure(BP);
        w.l1_items.ensure(max_l1);
        w.l1_d.ensure(max_l1 * k);
        w.l1_i.ensure(max_l1 * k);
        w.items.ensure(max_items);
        w.items_w.ensure(max_wide);
        w.part_d.ensure(max_items * k);
        w.part_i.ensure(max_items * k);
        w.slot_d.ensure(BP * k);
        w.slot_i.ensure(BP * k);
        w.carry_d.ensure((size_t)P * k);
        w.carry_i.ensure((size_t)P * k);
        w.carry2_d.ensure((size_t)P * k);
        w.carry2_i.ensure((size_t)P * k);
    }

    // ---- search: ivf_flat_index.cpp:205-256, one batch of B queries ----
    // The batch's queries as the kernels read them, zero-padded rows [B][dp]: when dim is
    // already a multiple of the padding (768) the caller's rows are used in place (they
    // stay valid until the stream passes the search, as for any asynchronous call), else
    // a padded copy in w.qpad.
    // With unit_rows: the unit queries, always in w.qpad (ensure_workspace sizes it [B][dp]
    // whatever dim is); the caller's rows are only read.
    void stage_queries(SearchSlot& w, const float* d_q, uint32_t B, hipStream_t s) {
        if (unit_rows) {
            vdbk::launch_unit_rows(d_q, B, dim, dp, w.qpad.p, s);
            w.q = w.qpad.p;
            return;
        }
        if (dim == dp && ((uintptr_t)d_q & 15) == 0) {  // (rows are read as float4)
            w.q = d_q;
            return;
        }
        vdbk::launch_pad_rows(d_q, B, dim, dp, w.qpad.p, s);
        w.q = w.qpad.p;
    }

    // Coarse step (select_nprobe_lists, cpp:298-336): padded queries into w.qpad, the
    // first min(nprobe, nlist) lists by (dist, list) into w.probes.
    void coarse_batch(SearchSlot& w, const float* d_q, uint32_t B, uint32_t P, hipStream_t s) {
        const int regs_p = vdbk::topk_regs(P);
        stage_queries(w, d_q, B, s);
        if (coarse_mode == 1 && metric != 2 && vdbk::rerank_rows(dp, regs_p) > 0) {
            vdbk::launch_coarse_mfma(metric, cent_rm.p, nlist, dp, w.q, B, w.cd.p, w.cdelta.p, s);
            vdbk::launch_select_rerank(metric, regs_p, w.cd.p, w.cdelta.p, cent_rm.p, nlist, dp, w.q, B, P,
                                       w.cand.p, w.probes.p, s);
        } else {
            vdbk::launch_coarse(metric, cent_il.p, nlist, d4, w.q, B, w.cd.p, s);
            vdbk::launch_select(regs_p, w.cd.p, nlist, B, P, w.probes.p, s);
        }
    }

    // Probe inversion, fine scan (search_list_cpu, cpp:339-384) and merges
    // (merge_results, cpp:474-518) of a batch whose padded queries are in w.qpad and
    // probes in w.probes.
    // Returns false (nothing merged) only for a screened batch of the tier's file home whose
    // candidates would need a buffer above tier_cand_max: the caller serves it through the
    // exact list-cache path instead (run_batch).
    bool scan_batch(SearchSlot& w, uint32_t B, uint32_t P, uint32_t k, float* out_d_, uint64_t* out_i_, hipStream_t s,
                    const uint32_t* req_start, uint32_t b0, EventSet* ev) {
        const ScanBounds bd = scan_bounds(kScanConsts, nseg_prefix, B, P);  // (what ensure_workspace sized by)
        require(bd.ok(), "batch too large", VDB_ERR_UNSUPPORTED);
        const uint32_t BP = (uint32_t)bd.BP;
        // (tier: lists and directory entries another stream loaded must have landed)
        if (tiered() && tier_ev_used) HIPCHECK(hipStreamWaitEvent(s, tier_ev, 0));
        last_P = P;
        snap.ok = false;  // (set below by the deferred screened route with rows in HBM)
        if (screen_stale) screen_update();
        // The route (scan_route.hpp): screened (default, L2 / IP, k <= 64) in items of swq
        // queries unless the run-time floor (lists in HBM only) sends the batch to the exact
        // scan; then every size and grid of the launches below.
        const ScanKnobs kn = knobs();
        const ScanFacts fa = facts();
        const ScanFits fit = fits(k);
        const int regs_k = fit.regs_k;
        const uint32_t swq = vdbe::screen_width(kn, fa, fit, P);
        uint32_t floor_seq = 0;
        const bool floor_ok =
            !floor_applies(kn, fa, swq) || floor.plan([this](uint32_t i) { return floor_entry(i); }, &floor_seq);
        const ScanRoute r = scan_route(kScanConsts, kn, fa, fit, bd, swq, floor_ok);
        if (r.need_arena) ensure_arena();
        auto plan = [&](unsigned long long* st) {
            vdbk::launch_plan(w.probes.p, d_nseg.p, d_count_local.p, B, P, (uint32_t)vdbk::scan_group(regs_k), r.plan_wide,
                              r.segs(), w.items.p, w.items_w.p, w.counters.p, w.sorted_pair.p, w.pbs.p, w.pbqp.p,
                              w.nseg_qp.p, w.l1base.p, w.l1_items.p, st, w.thr.p, r.mfma_min, s);
        };
        // (the automatic shadow's calibration batch counts into scratch: profile_read reports
        // the caller's batches only)
        plan(calibrating ? stats_scratch.ensure(16) : stats.p);
        const bool in_ring = &w >= slots && &w < slots + kSlots;
        if (scan_window && in_ring && scan_seq >= scan_window) {  // the scan issued scan_window batches ago
            const SearchSlot& prev = slots[scan_hist[(scan_seq - scan_window) % 8]];
            if (prev.scan_done) HIPCHECK(hipStreamWaitEvent(s, prev.scan_done, 0));
        }
        if (ev) HIPCHECK(hipEventRecord(ev->scan_begin, s));
        const float4* lists = tiered() ? cache.p : r.rows_l ? (const float4*)screen_rows.p : arena.p;
        vdbk::ScanArgs sa{lists, tiered() ? cache_ids.p : arena_ids.p, d_block_off.p, d_count_local.p, w.q, w.items.p, w.items_w.p,
                                w.counters.p, w.sorted_pair.p, w.pbs.p, w.part_d.p, w.part_i.p, d4, k,
                                wide_stride, w.counters.p + 4, seg_blocks, r.segs(), 0, w.thr.p,
                                r.mfma_min, bounded_stats && !calibrating ? stats.p + 5 : nullptr};
        sa.rows_layout = r.rows_l ? 1u : 0u;
        // the bounded items first (the batch's most-probed lists), on the same stream
        if (r.mfma_min) vdbk::launch_scan_bounded(metric, (uint32_t)bd.max_wide, sa, s);
        if (r.screened) {
            const bool defer = r.shape == ScanShape::ScreenDeferred;
            const bool i8s = r.i8s, tier_file = r.tier_file;
            uint32_t ccap = r.ccap;  // (an overflow re-run grows it)
            auto alloc_defer = [&]() {
                slot_buf(w, w.scnt, BP);
                slot_buf(w, w.ovf, BP);
                slot_buf(w, w.soff, (size_t)BP + 1);
                slot_buf(w, w.scand, ccap);
                slot_buf(w, w.surv, ccap);
                slot_buf(w, w.sdist, ccap);
                slot_buf(w, w.ubcnt, BP);
                slot_buf(w, w.ublist, (size_t)BP * vdbk::kUbLists * k);
                if (r.tier2) {
                    slot_buf(w, w.slb, ccap);
                    slot_buf(w, w.smark, ccap);
                    slot_buf(w, w.rowmap, ccap);
                }
            };
            auto pairs = [&]() {
                vdbk::launch_screen_pairs(metric, w.q, B, P, w.probes.p, cent_rm.p, dp,
                                          slot_buf(w, w.qres, (size_t)BP * dp), slot_buf(w, w.pst, BP),
                                          slot_buf(w, w.thr4, (size_t)BP * 4), s, defer ? w.scnt.p : nullptr,
                                          defer ? w.ovf.p : nullptr, defer ? w.counters.p : nullptr,
                                          defer ? w.ubcnt.p : nullptr, i8s ? slot_buf(w, w.qscale, BP) : nullptr);
            };
            if (defer) alloc_defer();
            pairs();
            sa.thr4 = w.thr4.p;
            sa.shadow = screen_sh.p;
            sa.rows = screen_rows.p;
            sa.meta = screen_meta.p;
            sa.sscale = i8s ? screen_scale.p : nullptr;
            sa.qscale = i8s ? w.qscale.p : nullptr;
            sa.qres = w.qres.p;
            sa.pst = w.pst.p;
            sa.dp = dp;
            sa.P = P;
            sa.wide_q = r.swq;
            sa.thr_every = r.thr_every;
            sa.fused = r.fused;
            if (tiered()) {  // the resident shadow's packing and ids; rows from the home
                sa.block_off = d_sblock_off.p;
                sa.ids = screen_ids.p;
                sa.rows = nullptr;
                sa.arena = file_home() ? nullptr : arena.p;  // (host home: page-locked, read over PCIe)
            }
            if (defer) {
                const float* fetched = nullptr;
                const bool recheck2 = r.recheck2, tier2 = r.tier2;
                for (int pass = 0;; ++pass) {
                    if (pass) {  // a re-run after an overflow (tier, file home): plan and pairs reset the state
                        alloc_defer();
                        plan(stats_scratch.ensure(16));  // (statistics of the batch are counted once)
                        pairs();
                    }
                    sa.cand = w.scand.p;
                    sa.cand_cap = ccap;
                    sa.ccount = w.counters.p + vdbk::kCtrCand;
                    sa.ovf = w.ovf.p;
                    sa.ublist = w.ublist.p;
                    sa.ubcnt = w.ubcnt.p;
                    if (floor_seq) {  // (its own ring entry, whatever slot or stream runs it)
                        if (!floor_host.p) {
                            floor_host.host = true;
                            std::memset(floor_host.ensure(ScreenFloor::kRing), 0, ScreenFloor::kRing * sizeof(uint4));
                        }
                        sa.floor_out = floor_host.p + floor_seq % ScreenFloor::kRing;
                        sa.floor_seq = floor_seq;
                    }
                    sa.mstats = bounded_stats && !pass && !calibrating ? stats.p + 8 : nullptr;
                    if (stamps_cap) {
                        sa.stamps = stamps_buf.p;
                        sa.stamps_cap = stamps_cap;
                        sa.stamp_batch = stamp_batch++;
                    }
                    if (ev) HIPCHECK(hipEventRecord(ev->collect_begin, s));
                    vdbk::launch_screen_collect(metric, r.grid_collect, sa, s);
                    if (ev) {
                        HIPCHECK(hipEventRecord(ev->collect_end, s));
                        ev->collected = true;
                    }
                    // (the two-pass re-check, rows in HBM: the survivors' lower bounds go where the
                    // one-pass path keeps their exact distances)
                    vdbk::launch_screen_select(sa, BP, w.scnt.p, w.soff.p, w.surv.p, w.ovf.p, s,
                                               recheck2 ? w.sdist.p : tier2 ? w.slb.p : nullptr);
                    if (!tier_file) break;
                    uint32_t need = 0;
                    if (tier2) {  // (pass A marked, its rows read; pass B after the loop)
                        vdbk::launch_tier_recheck(0, metric, sa, BP, w.nseg_qp.p, w.soff.p, w.scnt.p, w.surv.p, w.slb.p,
                                                  w.smark.p, nullptr, nullptr, nullptr, s);
                        if (fetch_rows_phase(w, 1, need, s)) {
                            fetched = w.srows.p;
                            break;
                        }
                    } else {
                        fetched = fetch_survivor_rows(w, need, s);
                        if (fetched) break;
                    }
                    const uint64_t grow = std::max<uint64_t>((uint64_t)need + need / 2, (uint64_t)ccap + 1024);
                    if (grow > std::max<uint64_t>(tier_cand_max, screen_cand_cap)) {
                        // (a regime where the bound is wider than the distance spread: the
                        // survivors' rows would cost more than the lists)
                        ++screen_tier_fallbacks;
                        return false;
                    }
                    ccap = (uint32_t)grow;
                    tier_cand_cap = ccap;  // (kept for the next batches)
                    ++screen_reruns;
                }
                if (tiered()) ++screen_tier_batches;
                if (!tiered() && sa.rows && in_ring) {  // (what vdb_ivf_screen_snapshot reads)
                    const uint32_t gmax = r.swq > 16 ? vdbk::kPersistentBlocks / 2 : vdbk::kPersistentBlocks;
                    snap = ScreenSnap{true, (int)(&w - slots), B, P, k, r.segs(), r.swq, ccap, i8s ? 1u : 0u,
                                      std::min<uint32_t>(r.grid_collect, gmax)};
                }
                if (tier2) {  // pass A's exact distances and pass B's marks; its rows; the pairs' top-k
                    vdbk::launch_tier_recheck(1, metric, sa, BP, w.nseg_qp.p, w.soff.p, w.scnt.p, w.surv.p, w.slb.p,
                                              w.smark.p, w.rowmap.p, w.srows.p, w.sdist.p, s);
                    uint32_t need = 0;
                    (void)fetch_rows_phase(w, 2, need, s);
                    vdbk::launch_tier_recheck(2, metric, sa, BP, w.nseg_qp.p, w.soff.p, w.scnt.p, w.surv.p, w.slb.p,
                                              w.smark.p, w.rowmap.p, w.srows.p, w.sdist.p, s);
                    HIPCHECK(hipGetLastError());
                } else {
                    vdbk::launch_screen_recheck(metric, sa, BP, w.probes.p, w.nseg_qp.p, w.soff.p, w.scnt.p, w.surv.p,
                                                w.ovf.p, fetched, w.sdist.p, ccap, (uint32_t)nseg_prefix[1], s,
                                                recheck2 ? w.sdist.p : nullptr);
                }
            } else {
                vdbk::launch_scan_screen(metric, r.grid_collect, sa, s);
            }
        } else if (r.shape == ScanShape::FusedWide) {
            sa.fused = r.fused;
            vdbk::launch_scan_wide(metric, r.grid_wide, sa, s, r.waves);
        } else if (r.shape == ScanShape::WideSide) {
            HIPCHECK(hipEventRecord(w.fork, s));
            HIPCHECK(hipStreamWaitEvent(w.side, w.fork, 0));
            vdbk::launch_scan_narrow(metric, regs_k, r.grid_narrow, sa, w.side);
            HIPCHECK(hipEventRecord(w.join, w.side));
            vdbk::launch_scan_wide(metric, r.grid_wide, sa, s, r.waves);
            HIPCHECK(hipStreamWaitEvent(s, w.join, 0));
        } else {
            vdbk::launch_scan_narrow(metric, regs_k, r.grid_narrow, sa, s);
        }
        if (ev) HIPCHECK(hipEventRecord(ev->scan_end, s));
        if (scan_window && in_ring) {
            if (!w.scan_done) HIPCHECK(hipEventCreateWithFlags(&w.scan_done, hipEventDisableTiming));
            HIPCHECK(hipEventRecord(w.scan_done, s));
            scan_hist[scan_seq % 8] = (int)(&w - slots);
            ++scan_seq;
        }
        if (fused_merge) {
            // one launch: slot folds, stale sources, unique top-k, the next batch's carry
            float* cd0 = w.carry_sel ? w.carry2_d.p : w.carry_d.p;
            uint64_t* ci0 = w.carry_sel ? w.carry2_i.p : w.carry_i.p;
            float* cd1 = w.carry_sel ? w.carry_d.p : w.carry2_d.p;
            uint64_t* ci1 = w.carry_sel ? w.carry_i.p : w.carry2_i.p;
            vdbk::launch_merge_fused(regs_k, w.probes.p, d_count_global.p, w.nseg_qp.p, w.pbqp.p, w.part_d.p, w.part_i.p, B,
                                     P, k, stale, req_start, b0, cd0, ci0, w.slot_d.p, w.slot_i.p, cd1, ci1, out_d_, out_i_,
                                     s);
            if (stale) w.carry_sel ^= 1u;
            if (ev) HIPCHECK(hipEventRecord(ev->end, s));
            HIPCHECK(hipGetLastError());
            return true;
        }
        vdbk::launch_merge_partials(regs_k, (uint32_t)bd.max_l1, w.probes.p, d_count_global.p, w.nseg_qp.p, w.pbqp.p, w.l1base.p,
                                    w.l1_items.p, w.counters.p, w.part_d.p, w.part_i.p, k, w.l1_d.p, w.l1_i.p, s);
        vdbk::launch_slot_merge(regs_k, w.probes.p, d_count_global.p, w.nseg_qp.p, w.pbqp.p, w.l1base.p, w.part_d.p, w.part_i.p,
                                w.l1_d.p, w.l1_i.p, BP, k, w.slot_d.p, w.slot_i.p, s);
        vdbk::launch_query_merge(regs_k, w.probes.p, d_count_global.p, w.slot_d.p, w.slot_i.p, w.carry_d.p, w.carry_i.p, B, P, k,
                                 stale, req_start, b0, out_d_, out_i_, s);
        if (stale)
            vdbk::launch_carry(w.probes.p, d_count_global.p, B, P, k, w.slot_d.p, w.slot_i.p, req_start, b0, w.carry_d.p,
                               w.carry_i.p, s);
        if (ev) HIPCHECK(hipEventRecord(ev->end, s));
        HIPCHECK(hipGetLastError());
        return true;
    }

    // One batch, every list HBM-resident (or the tier with every stored list cached).
    bool run_batch(SearchSlot& w, const float* d_q, uint32_t B, uint32_t P, uint32_t k, float* out_d_,
                   uint64_t* out_i_, hipStream_t s, const uint32_t* req_start, uint32_t b0) {
        EventSet* ev = prof ? &next_events() : nullptr;
        if (ev) HIPCHECK(hipEventRecord(ev->begin, s));
        coarse_batch(w, d_q, B, P, s);
        if (ev) HIPCHECK(hipEventRecord(ev->coarse_end, s));
        if (!scan_batch(w, B, P, k, out_d_, out_i_, s, req_start, b0, ev)) {
            // the screened tier could not serve it (tier_cand_max): the exact list-cache path
            force_exact = true;
            try {
                search_tiered(w, d_q, B, P, k, out_d_, out_i_, s, req_start, b0);
            } catch (...) {
                force_exact = false;
                throw;
            }
            force_exact = false;
        }
        return true;
    }

    // ---- list-cache tier search (cache smaller than the index) ----
    // The probes of the whole call are computed first (coarse steps only), so loads and
    // evictions are planned against the call's known future:
    //  * the call is cut into sub-batches of at most `batch` queries whose probed lists
    //    fill at most half the cache (so the next sub-batch's lists load beside them; a
    //    query needing more gets a sub-batch of its own); results never depend on batch
    //    boundaries;
    //  * while sub-batch i scans, the lists of sub-batch i+1 are read from the home
    //    (file: io_uring into page-locked staging; host memory: DMA) and copied into free
    //    cache space on copy_stream; sub-batch i+1 waits for them by event;
    //  * a victim is the cached list whose next use in the call is furthest away (not
    //    used again: first), then the least recently used; sub-batch i's lists (and i+1's)
    //    are never evicted while i runs.
    // The cut, the victim order and the placement are list_cache.hpp's; here are the data
    // movement and its ordering.
    // (qbase: the call-global index of d_q's first query, for the stale-slot semantics)
    void search_tiered(SearchSlot& w, const float* d_q, uint32_t n, uint32_t P, uint32_t k, float* d_dist,
                       uint64_t* d_ids, hipStream_t s, const uint32_t* req_start, uint32_t qbase = 0) {
        if (tier_call_used) HIPCHECK(hipEventSynchronize(tier_call_ev));  // probe_stage is reused
        const uint32_t bmax = batch_cap(P, k);
        // 1. probes of the whole call
        probe_stage.host = true;
        uint32_t* hp = probe_stage.ensure((size_t)n * P);
        for (uint32_t b0 = 0; b0 < n; b0 += bmax) {
            const uint32_t B = std::min(bmax, n - b0);
            coarse_batch(w, d_q + (size_t)b0 * dim, B, P, s);
            HIPCHECK(hipMemcpyAsync(hp + (size_t)b0 * P, w.probes.p, (size_t)B * P * 4, hipMemcpyDeviceToHost, s));
        }
        HIPCHECK(hipStreamSynchronize(s));
        // 2. sub-batches whose lists fit the cache, and each list's uses for the next-use ranks
        const ListSizes sz = list_sizes();
        SubBatches sb;
        try {
            sb = cut_subbatches(hp, n, P, bmax, sz, lc);
        } catch (const QueryOverCapacity&) {
            throw VdbError(VDB_ERR_OUT_OF_MEMORY, "list_cache_bytes cannot hold the lists one query probes");
        }
        const size_t nsb = sb.size();
        const std::vector<std::vector<uint32_t>>& U = sb.lists;
        const std::vector<uint32_t>& sb_begin = sb.begin;
        bool miss = false;
        for (const auto& u : U)
            for (uint32_t l : u) miss |= !lc.resident(l);
        auto rank_after = [&](size_t cur) { return [&sb, cur](uint32_t l) { return next_use(sb, l, cur); }; };
        if (miss) quiesce();  // searches on other streams may still read lists evicted below
        if (!copy_stream) {
            HIPCHECK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
            for (auto& e : sb_done) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            HIPCHECK(hipEventCreateWithFlags(&load_ev, hipEventDisableTiming));
            HIPCHECK(hipEventCreateWithFlags(&tier_call_ev, hipEventDisableTiming));
        }
        // 3. sub-batches in order, each next one's lists loaded while the current one scans
        std::vector<uint8_t> protect(nlist, 0);
        std::vector<ListCache::Load> loads;
        bool prefetched = false;
        for (size_t b = 0; b < nsb; ++b) {
            const uint32_t b0 = sb_begin[b], B = sb_begin[b + 1] - b0;
            if (prefetched) {
                HIPCHECK(hipStreamWaitEvent(s, load_ev, 0));
            } else {  // load on s itself, after the previous sub-batch in stream order
                for (uint32_t l : U[b]) protect[l] = 1;
                const bool ok = lc.plan_loads(U[b], protect, sz, rank_after(b), true, loads);
                for (uint32_t l : U[b]) protect[l] = 0;
                require(ok, "list_cache_bytes cannot hold the lists one sub-batch probes", VDB_ERR_OUT_OF_MEMORY);
                if (!loads.empty()) {
                    load_lists(loads, s);
                    upload_scan_directory(s);
                    ++tier_sync_loads;
                }
            }
            lc.touch(U[b]);
            EventSet* ev = prof ? &next_events() : nullptr;
            if (ev) HIPCHECK(hipEventRecord(ev->begin, s));
            stage_queries(w, d_q + (size_t)b0 * dim, B, s);
            HIPCHECK(hipMemcpyAsync(w.probes.p, hp + (size_t)b0 * P, (size_t)B * P * 4, hipMemcpyHostToDevice, s));
            if (ev) HIPCHECK(hipEventRecord(ev->coarse_end, s));
            require(scan_batch(w, B, P, k, d_dist + (size_t)b0 * k, d_ids + (size_t)b0 * k, s, req_start, qbase + b0, ev),
                    "tier sub-batch not served", VDB_ERR_STATE);
            HIPCHECK(hipEventRecord(sb_done[b & 1], s));
            ++tier_subbatches;
            prefetched = false;
            if (b + 1 < nsb) {
                for (uint32_t l : U[b]) protect[l] = 1;
                for (uint32_t l : U[b + 1]) protect[l] = 1;
                const bool ok = lc.plan_loads(U[b + 1], protect, sz, rank_after(b + 1), false, loads);
                for (uint32_t l : U[b]) protect[l] = 0;
                for (uint32_t l : U[b + 1]) protect[l] = 0;
                if (ok) {
                    // victims may still be read by sub-batch b - 1 (not by b: protected)
                    if (b >= 1) HIPCHECK(hipStreamWaitEvent(copy_stream, sb_done[(b - 1) & 1], 0));
                    if (!loads.empty()) {
                        load_lists(loads, copy_stream);  // the host reads the file while b scans
                        upload_scan_directory(copy_stream);
                        ++tier_prefetches;
                    }
                    HIPCHECK(hipEventRecord(load_ev, copy_stream));
                    prefetched = true;
                }
            }
        }
        HIPCHECK(hipEventRecord(tier_call_ev, s));
        tier_call_used = true;
    }

    // ---- the scan's routing and sizing: scan_route.hpp decides, from these plain copies ----
    static constexpr ScanConsts kScanConsts{(uint32_t)vdbk::kMergeFan, (uint32_t)vdbk::kPlanMaxPairs,
                                            vdbk::kPersistentBlocks, VDB_SCAN_DIAG};
    ScanKnobs knobs() const {
        ScanKnobs kn;
        kn.wide_scan = wide_scan;
        kn.wide_group = wide_group;
        kn.fused_scan = fused_scan;
        kn.scan_mfma_min = scan_mfma_min;
        kn.scan_blocks = scan_blocks;
        kn.segs_item_opt = segs_item_opt;
        kn.narrow_blocks = narrow_blocks;
        kn.screen_group = screen_group;
        kn.screen_defer = screen_defer;
        kn.screen_i8 = screen_i8;
        kn.screen_recheck2 = screen_recheck2;
        kn.screen_thr_every = screen_thr_every;
        kn.screen_cand_cap = screen_cand_cap;
        kn.tier_cand_cap = tier_cand_cap;
        return kn;
    }
    ScanFacts facts() const {
        ScanFacts fa;
        fa.metric = metric;
        fa.seg_blocks = seg_blocks;
        fa.screen_segs_auto = screen_segs_auto;
        fa.screen_ready = screen_ready;
        fa.screen_fmt_i8 = screen_fmt_i8;
        fa.i8_vetoed = i8_vetoed;
        fa.arena_dropped = arena_dropped;
        fa.force_exact = force_exact;
        fa.calibrating = calibrating;
        fa.tiered = tiered();
        fa.file_home = file_home();
        return fa;
    }
    ScanFits fits(uint32_t k) const {
        return {vdbk::topk_regs(k),
                vdbk::scan_wide_fits(d4, k, 4),
                vdbk::scan_wide_fits(d4, k, 8),
                vdbk::scan_bounded_fits(d4, k),
                vdbk::scan_screen_fits(k, dp, 16, screen_defer),
                vdbk::scan_screen_fits(k, dp, 32, screen_defer)};
    }
    // The screen serves a search with this k and nprobe (the tier: the deferred scan with its
    // shadow resident; built lazily, so a stale screen is rebuilt first).
    bool screen_serves(uint32_t k, uint32_t P) {
        last_P = P;
        if (screen_stale) screen_update();
        return vdbe::screen_width(knobs(), facts(), fits(k), P) != 0;
    }
    uint32_t batch_cap(uint32_t P, uint32_t k) const { return vdbe::batch_cap(kScanConsts, batch, nseg_prefix, P, k); }

    // Grow a slot-owned buffer; a buffer still read by the slot's previous call is
    // only freed once that call is done.
    template <class T>
    T* slot_buf(SearchSlot& w, DevBuf<T>& b, size_t n) {
        if (b.cap < n && b.p && w.used) HIPCHECK(hipEventSynchronize(w.done));
        return b.ensure(n);
    }

    // One reference search() call on this handle's device: take the next workspace slot,
    // order stream s after the slot's previous call, start the call's probe slots
    // (allocated once per call, cpp:210-211). `xworld` > 0 sizes the multi-GPU records.
    SearchSlot& begin_call(uint32_t n, uint32_t P, uint32_t k, hipStream_t s, uint32_t xworld) {
        if (!stats.p) {
            stats.ensure(16);
            HIPCHECK(hipMemsetAsync(stats.p, 0, 128, s));
        }
        SearchSlot& w = slots[next_slot];
        next_slot = (next_slot + 1) % kSlots;
        const uint32_t B = std::min(batch_cap(P, k), n);
        ensure_workspace(w, B, P, k);
        if (xworld) {
            const uint64_t rb = vdb_rank_record_bytes(B, k);
            // (emulated exchange: W records are sent; the other ranks' places hold empty records)
            if (comm_world == 1 && xchg_emulate > 1 && w.xrec.cap < rb * xworld) {
                slot_buf(w, w.xrec, rb * xworld);
                w.xfill = 0;
            }
            slot_buf(w, w.xrec, rb);
            slot_buf(w, w.xgat, rb * xworld);
        }
        if (w.used) HIPCHECK(hipStreamWaitEvent(s, w.done, 0));
        HIPCHECK(hipMemsetAsync(w.carry_i.p, 0xFF, (size_t)P * k * 8, s));
        w.carry_sel = 0;
        return w;
    }

    void end_call(SearchSlot& w, hipStream_t s) {
        HIPCHECK(hipEventRecord(w.done, s));
        w.used = true;
    }

    // The slot's packed record for a batch of B queries (vdb_rank_record_bytes layout).
    static float* rec_dist(SearchSlot& w) { return (float*)w.xrec.p; }
    static uint64_t* rec_ids(SearchSlot& w, uint32_t B, uint32_t k) {
        return (uint64_t*)(w.xrec.p + ((uint64_t)B * k * 4 + 7) / 8 * 8);
    }
    // Final results of a batch from `nranks` gathered records: unique-id top-k of the
    // union (= merge_results over every rank's lists, cpp:474-518).
    static void merge_gathered(SearchSlot& w, uint32_t nranks, uint32_t B, uint32_t k, float* od, uint64_t* oi,
                               hipStream_t s) {
        const uint64_t rec = vdb_rank_record_bytes(B, k);
        const float* d = (const float*)w.xgat.p;
        const uint64_t* ids = (const uint64_t*)(w.xgat.p + ((uint64_t)B * k * 4 + 7) / 8 * 8);
        vdbk::launch_rank_merge(vdbk::topk_regs(k), d, ids, rec / 4, rec / 8, nranks, B, k, od, oi, s);
        HIPCHECK(hipGetLastError());
    }

    // Group handle (group.cpp): the same call over every member's shard.
    void group_search_device(const float* d_q, uint32_t n, uint32_t P, uint32_t k, float* d_dist, uint64_t* d_ids,
                             hipStream_t s, const uint32_t* req_start);
    bool group_tiered() const {
        for (auto& mb : members)
            if (mb->tiered()) return true;
        return false;
    }

    // req_start: null (one reference search() call) or, for a coalesced batch of calls,
    // per query the call-global index of its request's first query (device memory).
    // With a communicator attached, every batch's partials are all-gathered over RCCL
    // and merged, so d_dist / d_ids receive the final results on every rank.
    void search_device(const float* d_q, uint32_t n, uint32_t nprobe, uint32_t k, float* d_dist, uint64_t* d_ids,
                       hipStream_t s, const uint32_t* req_start = nullptr) {
        if (n == 0 || k == 0) return;
        require(k <= (uint32_t)vdbk::kMaxK, "k above 1024 is not supported", VDB_ERR_UNSUPPORTED);
        const uint32_t P = std::min(nprobe, nlist);  // cpp:218-222 reads out of bounds beyond nlist
        if (P == 0) {
            vdbk::launch_fill_empty((uint64_t)n * k, d_dist, d_ids, s);
            HIPCHECK(hipGetLastError());
            return;
        }
        require(P <= (uint32_t)vdbk::kMaxK, "nprobe above 1024 is not supported", VDB_ERR_UNSUPPORTED);
        if (is_group()) {
            // (the members, reached through run_batch / call_to_record, hand out -dot partials;
            // the mapping follows the group's merge)
            group_search_device(d_q, n, P, k, d_dist, d_ids, s, req_start);
            cos_finish(d_dist, d_ids, (uint64_t)n * k, s);
            return;
        }
        const bool xchg = comm != nullptr;
        if (xchg)
            require((comm_world == world && comm_rank == rank) || (comm_world == 1 && xchg_emulate == world),
                    "the attached communicator's (rank, world) differs from the handle's shard", VDB_ERR_STATE);
        SearchSlot& w = begin_call(n, P, k, s, xchg ? xchg_records() : 0);
        if (xchg && (tiered() || comm_world > 1)) {
            // The exchange is per CALL at world > 1: the whole call's partials in one record,
            // ONE all-gather, one merge. A rank's own state (its tier, switched on by its own
            // shard's size against max_gpu_memory, and what its cache holds) decides how it
            // cuts a call into batches, so per-batch exchanges could differ in number and
            // size between ranks; per call, every rank issues the same collective whatever
            // its state. With 64-query calls (the bench) a call is one batch.
            slot_buf(w, w.xgat, vdb_rank_record_bytes(n, k) * comm_world);
            call_to_record(w, d_q, n, P, k, s, req_start);
            exchange(w, n, k, d_dist, d_ids, s);
            end_call(w, s);
            return;
        }
        if (through_tier(k, P))
            search_tiered(w, d_q, n, P, k, d_dist, d_ids, s, req_start);
        else
            plain_batches(w, d_q, n, P, k, d_dist, d_ids, s, req_start, xchg);
        cos_finish(d_dist, d_ids, (uint64_t)n * k, s);
        end_call(w, s);
    }

    // unit_rows: the call's final [n][k] distances, after the last merge (the batches' stale
    // carries hold -dot and never read the output), mapped by 1.0f + d where an id is filled.
    void cos_finish(float* d_dist, const uint64_t* d_ids, uint64_t nk, hipStream_t s) {
        if (!unit_rows) return;
        vdbk::launch_cos_finish(d_dist, d_ids, nk, s);
        HIPCHECK(hipGetLastError());
    }

    // The tier serves a search through its list cache when some stored list is not cached
    // (every one cached: the plain path) and the screen does not serve it.
    bool through_tier(uint32_t k, uint32_t P) {
        return tiered() && lc.resident_lists() < storable_n && !screen_serves(k, P);
    }
    // A call's queries in batches of at most batch_cap, results at od / oi ([n][k]);
    // xchg_each: every batch goes through the slot's record and one exchange of its own.
    void plain_batches(SearchSlot& w, const float* d_q, uint32_t n, uint32_t P, uint32_t k, float* od, uint64_t* oi,
                       hipStream_t s, const uint32_t* req_start, bool xchg_each = false) {
        const uint32_t bmax = batch_cap(P, k);
        for (uint32_t b0 = 0, B = std::min(bmax, n); b0 < n; b0 += B, B = std::min(B, n - b0)) {
            float* bd = od + (size_t)b0 * k;
            uint64_t* bi = oi + (size_t)b0 * k;
            run_batch(w, d_q + (size_t)b0 * dim, B, P, k, xchg_each ? rec_dist(w) : bd, xchg_each ? rec_ids(w, B, k) : bi, s,
                      req_start, b0);
            if (xchg_each) exchange(w, B, k, bd, bi, s);
        }
    }

    // This shard's partial results of a whole call (n queries) into the slot's packed
    // record: through the tier when some stored list is not cached, else the plain batches.
    void call_to_record(SearchSlot& w, const float* d_q, uint32_t n, uint32_t P, uint32_t k, hipStream_t s,
                        const uint32_t* req_start) {
        slot_buf(w, w.xrec, vdb_rank_record_bytes(n, k));
        float* rd = rec_dist(w);
        uint64_t* ri = rec_ids(w, n, k);
        if (through_tier(k, P))
            search_tiered(w, d_q, n, P, k, rd, ri, s, req_start);
        else
            plain_batches(w, d_q, n, P, k, rd, ri, s, req_start);
    }

    // ONE all-gather of the slot's packed record (B queries) over the attached
    // communicator, on comm_stream fenced against s, then the on-device merge into the
    // final results. The enqueue is settled against the communicator's deadline and the
    // completion is handed to the watchdog (watch_exchange).
    void exchange(SearchSlot& w, uint32_t B, uint32_t k, float* od, uint64_t* oi, hipStream_t s) {
        if (comm_failed()) throw VdbError(VDB_ERR_DEVICE, comm_error_msg());
        EventSet* ev = prof && events_used ? &events[events_used - 1] : nullptr;  // (the call's last batch)
        const uint32_t nrec = xchg_records();
        if (comm_world == 1 && nrec > 1 && w.xfill != vdb_rank_record_bytes(B, k)) {
            // (emulation: the other ranks' places hold EMPTY records of this batch's layout —
            // (+inf or FLT_MAX, no id) entries the merge drops — so the emulated exchange moves
            // and merges W records and the results stay this rank's exact answer;
            // refilled whenever the record layout (B, k) changes)
            const uint64_t rb = vdb_rank_record_bytes(B, k);
            for (uint32_t r = 1; r < nrec; ++r)
                vdbk::launch_fill_empty((uint64_t)B * k, (float*)(w.xrec.p + rb * r),
                                        (uint64_t*)(w.xrec.p + rb * r + ((uint64_t)B * k * 4 + 7) / 8 * 8), s);
            HIPCHECK(hipGetLastError());
            w.xfill = rb;
        }
        const hipStream_t cs = comm_enter(w, s);
        nccl_settle(ncclAllGather(w.xrec.p, w.xgat.p, vdb_rank_record_bytes(B, k) * (comm_world == 1 ? nrec : 1), ncclUint8,
                                  comm, cs),
                    "ncclAllGather");
        if (ev) HIPCHECK(hipEventRecord(ev->x_end, cs));
        watch_exchange(cs);
        comm_leave(w, s);
        merge_gathered(w, nrec, B, k, od, oi, s);
        if (ev) {
            HIPCHECK(hipEventRecord(ev->m_end, s));
            ev->xchg = true;
        }
    }

    // ---- the communicator's deadline (option comm_timeout_ms) ----
    // Non-blocking RCCL (ncclCommInitRankConfig, blocking = 0): init and every collective
    // may return ncclInProgress and are polled to completion here, so a rank that never
    // joins or a connection that never forms ends in an error naming this rank instead of
    // a silent hang. Device-side completion of each exchange is watched by a host thread:
    // an all-gather still pending after the deadline (a peer stalled or died) marks the
    // communicator failed; later calls fail with that message, and vdb_ivf_comm_status
    // lets a caller that waits on its streams stop waiting. (The communicator is not
    // aborted from the watchdog: a collective still queued behind other work would then
    // run on released resources. The process is expected to exit.)
    uint32_t comm_timeout_ms = 120000;
    std::string rank_tag() const {
        return "rank " + std::to_string(comm_rank) + " of " + std::to_string(comm_world) + ": ";
    }
    void nccl_settle(ncclResult_t r, const char* what) {
        if (r == ncclSuccess) return;
        if (r != ncclInProgress) throw VdbError(VDB_ERR_DEVICE, rank_tag() + what + ": " + ncclGetErrorString(r));
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t spin = 0;; ++spin) {
            ncclResult_t st = ncclSuccess;
            const ncclResult_t q = ncclCommGetAsyncError(comm, &st);
            if (q != ncclSuccess) st = q;
            if (st == ncclSuccess) return;
            if (st != ncclInProgress)
                throw VdbError(VDB_ERR_DEVICE, rank_tag() + what + " failed: " + ncclGetErrorString(st));
            const double ms =
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (ms > comm_timeout_ms) {
                set_comm_error(rank_tag() + what + " still in progress after " + std::to_string((int)ms) +
                               " ms (comm_timeout_ms): a peer rank is missing or stalled");
                throw VdbError(VDB_ERR_DEVICE, comm_error_msg());
            }
            if (spin > 1000) std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
    }
    struct Watch {
        std::mutex m;
        std::condition_variable cv;
        std::deque<std::pair<hipEvent_t, std::chrono::steady_clock::time_point>> pending;  // issue order
        std::vector<hipEvent_t> spare;
        std::thread th;
        bool stop = false;
        uint64_t issued = 0, completed = 0;
        std::string error;  // the first deadline miss (sticky until detach / a new attach)
    };
    std::unique_ptr<Watch> watch;
    bool comm_failed() {
        if (!watch) return false;
        std::lock_guard<std::mutex> g(watch->m);
        return !watch->error.empty();
    }
    std::string comm_error_msg() {
        if (!watch) return std::string();
        std::lock_guard<std::mutex> g(watch->m);
        return watch->error;
    }
    void set_comm_error(const std::string& e) {
        start_watch();
        std::lock_guard<std::mutex> g(watch->m);
        if (watch->error.empty()) {
            watch->error = e;
            std::fprintf(stderr, "[vdb_ivf] %s\n", e.c_str());
        }
    }
    void start_watch() {
        if (watch) return;
        watch.reset(new Watch());
        watch->th = std::thread([this] { watch_loop(); });
    }
    void stop_watch() {
        if (!watch) return;
        {
            std::lock_guard<std::mutex> g(watch->m);
            watch->stop = true;
        }
        watch->cv.notify_all();
        if (watch->th.joinable()) watch->th.join();
        for (auto& p : watch->pending) (void)hipEventDestroy(p.first);
        for (hipEvent_t e : watch->spare) (void)hipEventDestroy(e);
        watch.reset();
    }
    void watch_exchange(hipStream_t cs) {
        start_watch();
        hipEvent_t e = nullptr;
        {
            std::lock_guard<std::mutex> g(watch->m);
            if (!watch->spare.empty()) {
                e = watch->spare.back();
                watch->spare.pop_back();
            }
        }
        if (!e) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(e, cs));
        {
            std::lock_guard<std::mutex> g(watch->m);
            watch->pending.push_back({e, std::chrono::steady_clock::now()});
            ++watch->issued;
        }
        watch->cv.notify_one();
    }
    void watch_loop() {
        (void)hipSetDevice(device);
        std::unique_lock<std::mutex> lk(watch->m);
        while (!watch->stop) {
            if (watch->pending.empty()) {
                watch->cv.wait_for(lk, std::chrono::milliseconds(200));
                continue;
            }
            const hipEvent_t e = watch->pending.front().first;
            const auto t = watch->pending.front().second;
            lk.unlock();
            const hipError_t q = hipEventQuery(e);
            lk.lock();
            if (q == hipSuccess) {
                watch->pending.pop_front();
                watch->spare.push_back(e);
                ++watch->completed;
                continue;
            }
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
            if (watch->error.empty() && (q != hipErrorNotReady || ms > comm_timeout_ms)) {
                watch->error = rank_tag() + "exchange " + std::to_string(watch->completed) + " (all-gather) " +
                               (q != hipErrorNotReady ? std::string("failed: ") + hipGetErrorString(q)
                                                      : "not complete after " + std::to_string((int)ms) +
                                                            " ms (comm_timeout_ms): a peer rank stalled or died");
                std::fprintf(stderr, "[vdb_ivf] %s\n", watch->error.c_str());
            }
            watch->cv.wait_for(lk, std::chrono::milliseconds(q == hipErrorNotReady ? 2 : 200));
        }
    }
};
