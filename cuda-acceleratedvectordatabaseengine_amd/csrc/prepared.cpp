// prepared.cpp — prepared id filters on one handle: vdb_ivf_filter_create(_device),
// vdb_filter_combine, vdb_ivf_search_prepared and vdb_ivf_range_search_prepared.
//
// A vdb_filter is what filter.cpp builds per call and throws away: per 64-slot arena block an
// allow mask, per list the allowed count, both on the device. Built once (the ids uploaded as
// given, sorted on the device by hipcub's radix sort, marked by ivf_filter_mark, counted by
// ivf_filter_count), it serves any number of searches, and of range searches through the
// masked range scan (range_kernels.hip). Two filters of one handle combine word by word
// (ivf_filter_combine), counted again.
//
// The masks are addressed by arena block and slot. The switch between the interleaved arena
// and the screen's row-major copy keeps every row in its block and slot, so a filter survives
// it; whatever can move a row (an add, a remove that removed, load, open_lists, the shard and
// residency calls, destroy) gives the handle a new epoch in its C ABI entry point
// (filter_epoch.hpp, engine.cpp), and the filter is stale from then on. A filter also keeps
// the block count and the row count it was made under and is live only while all of them match.
//
// Free functions over vdb_ivf's public members, as filter.cpp and range.cpp are and for the
// same reason. Nothing here changes the handle.
#include "prepared.hpp"

#include <cmath>
#include <vector>

#include "exact_call.hpp"
#include "filter.hpp"
#include "filter_epoch.hpp"
#include "filter_kernels.hpp"
#include "prepared_kernels.hpp"
#include "remove_plan.hpp"

namespace vdbe {

thread_local FilterCreateTiming g_filter_create_timing;

namespace {

struct Events {
    hipEvent_t e[4] = {};  // sort begin / end, mark begin / end
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

// A filter for h as it is now, its buffers sized and nothing in them yet.
std::unique_ptr<vdb_filter> blank_filter(vdb_ivf& h) {
    auto f = std::make_unique<vdb_filter>();
    f->h = &h;
    f->epoch = filter_epochs().get(&h);
    f->arena_blocks = h.arena_blocks;
    f->total = h.total;
    f->nlist = h.nlist;
    f->device = h.device;
    f->allow.ensure(h.arena_blocks);
    f->allowed.ensure(h.nlist);
    return f;
}

// The per-list counts of f's masks (ivf_filter_count, `after` recorded behind it), their sum to
// the host. Synchronises s.
void count_allowed(vdb_ivf& h, vdb_filter& f, hipStream_t s, hipEvent_t after = nullptr) {
    std::vector<uint32_t> per(h.nlist, 0);
    if (h.arena_blocks) {
        vdbk::launch_filter_count(f.allow.p, h.d_block_off.p, h.d_count_local.p, h.nlist, f.allowed.p, s);
        HIPCHECK(hipGetLastError());
        if (after) HIPCHECK(hipEventRecord(after, s));
        HIPCHECK(hipMemcpyAsync(per.data(), f.allowed.p, (size_t)h.nlist * 4, hipMemcpyDeviceToHost, s));
    } else {
        HIPCHECK(hipMemsetAsync(f.allowed.p, 0, (size_t)h.nlist * 4, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    f.n_allowed = 0;
    for (uint32_t c : per) f.n_allowed += c;
}

void require_filter(const vdb_ivf& h, const vdb_filter& f) {
    require(f.h == &h, "the filter belongs to another handle");
}

void require_live(const vdb_filter& f) {
    require(filter_live(f), "the filter is stale: the handle's rows changed after it was prepared (prepare it again)",
            VDB_ERR_STATE);
}

}  // namespace

bool filter_live(const vdb_filter& f) {
    if (!f.h || !filter_epochs().live(f.h, f.epoch)) return false;
    return f.h->arena_blocks == f.arena_blocks && f.h->total == f.total && f.h->nlist == f.nlist;
}

std::unique_ptr<vdb_filter> filter_create(vdb_ivf& h, const uint64_t* ids, uint64_t n, bool include,
                                          bool device_ids) {
    require(n < (1ull << 31), "more than 2^31 - 1 ids in one filter", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, "filter_create");
    g_filter_create_timing = FilterCreateTiming{};
    hipStream_t s = h.stream;
    const uint64_t nb = h.arena_blocks;
    require(nb == 0 || h.arena_ids.p != nullptr, "the handle holds no ids", VDB_ERR_STATE);

    DevBuf<uint64_t> d_in, d_sorted;
    DevBuf<uint32_t> d_valid;
    DevBuf<unsigned char> d_temp;
    Events ev;
    auto f = blank_filter(h);
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)
    if (nb == 0) {  // nothing stored: nothing to allow
        count_allowed(h, *f, s);
        return f;
    }
    const std::vector<uint32_t> valid = remove_block_valid(h.count, h.block_off, h.owned, nb);
    HIPCHECK(hipMemcpyAsync(d_valid.ensure(nb), valid.data(), nb * 4, hipMemcpyHostToDevice, s));
    // 1. the ids as given, sorted on the device (repeats stay)
    if (n) {
        const uint64_t* src = ids;
        if (!device_ids) {
            HIPCHECK(hipMemcpyAsync(d_in.ensure(n), ids, n * 8, hipMemcpyHostToDevice, s));
            src = d_in.p;
        }
        size_t tb = 0;
        HIPCHECK(vdbk::filter_sort_temp_bytes((uint32_t)n, tb));
        d_temp.ensure(tb);
        d_sorted.ensure(n);
        HIPCHECK(hipEventRecord(ev.e[0], s));
        HIPCHECK(vdbk::launch_filter_sort(d_temp.p, tb, src, d_sorted.p, (uint32_t)n, s));
        HIPCHECK(hipEventRecord(ev.e[1], s));
    }
    // 2. mark and count, as the one-shot call does
    HIPCHECK(hipEventRecord(ev.e[2], s));
    vdbk::launch_filter_mark(h.arena_ids.p, d_valid.p, nb, d_sorted.p, (uint32_t)n, include ? 1 : 0, f->allow.p, s);
    HIPCHECK(hipGetLastError());
    count_allowed(h, *f, s, ev.e[3]);
    if (n) g_filter_create_timing.sort_ms = ev.ms(0, 1);
    g_filter_create_timing.mark_ms = ev.ms(2, 3);
    return f;
}

std::unique_ptr<vdb_filter> filter_combine(const vdb_filter& a, const vdb_filter& b, int op) {
    require(a.h != nullptr && a.h == b.h, "the two filters belong to different handles");
    require(op == VDB_FILTER_AND || op == VDB_FILTER_OR || op == VDB_FILTER_ANDNOT, "invalid filter operation");
    require_live(a);
    require_live(b);
    vdb_ivf& h = *a.h;
    require_resident_single(h, "filter_combine");
    hipStream_t s = h.stream;
    auto f = blank_filter(h);
    StreamFence fence{s};
    vdbk::launch_filter_combine(a.allow.p, b.allow.p, h.arena_blocks, op, f->allow.p, s);
    HIPCHECK(hipGetLastError());
    count_allowed(h, *f, s);
    return f;
}

void search_prepared(vdb_ivf& h, const vdb_filter& f, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                     float* distances, uint64_t* ids) {
    require_filter(h, f);
    require(k <= vdbk::kFilterMaxK, "search_prepared serves k <= 64", VDB_ERR_UNSUPPORTED);
    require_resident_single(h, "search_prepared");
    require_live(f);
    search_masked(h, queries, n, nprobe, k, f.allow.p, f.allowed.p, distances, ids, "search_prepared");
}

std::unique_ptr<vdb_range_result> range_search_prepared(vdb_ivf& h, const vdb_filter& f, const float* queries,
                                                        uint32_t n, uint32_t nprobe, float radius, uint64_t reserve,
                                                        bool screen) {
    require_filter(h, f);
    require(!std::isnan(radius), "the radius is NaN");
    require_resident_single(h, "range_search_prepared");
    require_live(f);
    return range_search(h, queries, n, nprobe, radius, reserve, f.allow.p, f.allowed.p, screen);
}

}  // namespace vdbe
