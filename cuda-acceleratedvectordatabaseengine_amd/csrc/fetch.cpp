// fetch.cpp — vdb_ivf_fetch_ids(_device) and vdb_ivf_search_ids on one handle: given ids, the
// stored rows, and a search with stored rows as the queries.
//
// "The row of an id" is the stored row carrying it at the lowest list id and, within that
// list, the earliest position in add order, bit for bit as vdb_ivf_get_list returns it; an id no
// row carries gives dim zeros and found = 0. Pad slots are never matched.
//
// Nothing moves and nothing is rebuilt. Per call: the request uploaded as given and sorted on
// the device (launch_filter_sort, repeats stay), locate (ivf_fetch_locate: per sorted entry the
// smallest arena slot whose id equals it, from the ids alone), gather (ivf_fetch_gather: one
// wave per request entry, from the fp32 layout the handle holds at that moment: the interleaved
// arena, or the screen's row-major copy while the arena is dropped). search_ids gathers the
// found rows densely into a device buffer and hands that to the handle's own search_device, the
// entry vdb_ivf_search_device uses; the rows never leave the device.
//
// A free function over vdb_ivf's public members, as filter.cpp is and for the same reason: the
// handle's header is one of the sources the build id hashes. The fetch calls nothing that
// changes the handle; its buffers are the call's own.
#include "fetch.hpp"

#include <algorithm>
#include <cfloat>
#include <cstring>

#include "exact_call.hpp"
#include "fetch_kernels.hpp"
#include "prepared_kernels.hpp"
#include "remove_plan.hpp"

namespace vdbe {

thread_local FetchTiming g_fetch_timing;

namespace {

struct Events {
    hipEvent_t e[8] = {};  // begin / end of: sort, locate, gather, second gather
    bool used[4] = {};
    Events() {
        for (auto& x : e) HIPCHECK(hipEventCreate(&x));
    }
    ~Events() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
    void begin(int step, hipStream_t s) { HIPCHECK(hipEventRecord(e[2 * step], s)); }
    void end(int step, hipStream_t s) {
        HIPCHECK(hipEventRecord(e[2 * step + 1], s));
        used[step] = true;
    }
    double ms(int step) {  // (the stream is synchronised)
        if (!used[step]) return 0.0;
        float t = 0.f;
        HIPCHECK(hipEventElapsedTime(&t, e[2 * step], e[2 * step + 1]));
        return t;
    }
};

// The slot order is the (list, position) order only if the lists' blocks ascend with the list
// id: vdb_ivf::relayout and remove_plan both pack them so. Checked on the directory (O(nlist)).
bool blocks_ascend(const vdb_ivf& h) {
    uint64_t next = 0;
    for (uint32_t l = 0; l < h.nlist; ++l) {
        if (!h.owned[l] || h.count[l] == 0) continue;
        if (h.block_off[l] < next) return false;
        next = h.block_off[l] + cdiv(h.count[l], 64);
    }
    return next <= h.arena_blocks;
}

void refuse(const vdb_ivf& h, uint64_t n, const char* call) {
    require(n < (1ull << 31), std::string("more than 2^31 - 1 ids in one ") + call, VDB_ERR_UNSUPPORTED);
    require_resident_single(h, call);
}

// The call's device buffers up to the reverse map, and the layout the gather reads.
struct Located {
    DevBuf<uint64_t> d_in, d_sorted;
    DevBuf<unsigned char> d_temp;
    DevBuf<uint32_t> d_valid;
    std::vector<uint32_t> valid;  // (the upload's source: lives as long as the buffers)
    DevBuf<unsigned long long> d_loc;
    const uint64_t* req = nullptr;  // the request on the device, in request order
    const float4* lists = nullptr;
    int rows = 0;
};

// Steps 1 and 2 for n > 0 ids: upload (host ids), sort, locate. Enqueued on h.stream.
void locate(vdb_ivf& h, const uint64_t* ids, uint32_t n, bool device_ids, Located& L, Events& ev) {
    hipStream_t s = h.stream;
    const uint64_t nb = h.total ? h.arena_blocks : 0;
    if (nb) {
        L.lists = resident_lists(h);  // (refused before any device work)
        L.rows = h.arena_dropped ? 1 : 0;
        require(blocks_ascend(h), "the lists' blocks do not ascend with the list id", VDB_ERR_STATE);
    }
    L.req = ids;
    if (!device_ids) {
        HIPCHECK(hipMemcpyAsync(L.d_in.ensure(n), ids, (size_t)n * 8, hipMemcpyHostToDevice, s));
        L.req = L.d_in.p;
    }
    // 1. the ids as given, sorted on the device (repeats stay: an equal run shares its first entry)
    size_t tb = 0;
    HIPCHECK(vdbk::filter_sort_temp_bytes(n, tb));
    L.d_temp.ensure(tb);
    L.d_sorted.ensure(n);
    ev.begin(0, s);
    HIPCHECK(vdbk::launch_filter_sort(L.d_temp.p, tb, L.req, L.d_sorted.p, n, s));
    ev.end(0, s);
    // 2. per sorted entry the smallest slot that stores it
    if (nb) {
        L.valid = remove_block_valid(h.count, h.block_off, h.owned, nb);
        HIPCHECK(hipMemcpyAsync(L.d_valid.ensure(nb), L.valid.data(), nb * 4, hipMemcpyHostToDevice, s));
    }
    ev.begin(1, s);
    HIPCHECK(hipMemsetAsync(L.d_loc.ensure(n), 0xFF, (size_t)n * 8, s));
    vdbk::launch_fetch_locate(h.arena_ids.p, L.d_valid.p, nb, L.d_sorted.p, n, L.d_loc.p, s);
    HIPCHECK(hipGetLastError());
    ev.end(1, s);
}

void gather(vdb_ivf& h, const Located& L, uint32_t n, const uint32_t* d_dst, float* d_out, uint8_t* d_found,
            unsigned long long* d_count, Events& ev, int step) {
    ev.begin(step, h.stream);
    vdbk::launch_fetch_gather(L.lists, L.rows, h.d4, h.dim, L.req, n, L.d_sorted.p, L.d_loc.p, d_dst, d_out, d_found,
                              d_count, h.stream);
    HIPCHECK(hipGetLastError());
    ev.end(step, h.stream);
}

void take_timing(Events& ev, uint64_t rows_found) {
    g_fetch_timing.sort_ms = ev.ms(0);
    g_fetch_timing.locate_ms = ev.ms(1);
    g_fetch_timing.gather_ms = ev.ms(2) + ev.ms(3);
    g_fetch_timing.rows_found = rows_found;
}

}  // namespace

uint64_t fetch_ids(vdb_ivf& h, const uint64_t* ids, uint64_t n64, bool device_bufs, float* vectors, uint8_t* found) {
    refuse(h, n64, "fetch_ids");
    g_fetch_timing = FetchTiming{};
    if (n64 == 0) return 0;
    const uint32_t n = (uint32_t)n64;
    hipStream_t s = h.stream;
    Located L;
    DevBuf<float> d_out;
    DevBuf<uint8_t> d_found;
    DevBuf<unsigned long long> d_count;
    Events ev;
    unsigned long long count = 0;
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

    locate(h, ids, n, device_bufs, L, ev);
    // 3. the rows, the marks and the count
    float* out = vectors;
    uint8_t* fnd = found;
    if (!device_bufs) {
        if (vectors) out = d_out.ensure((size_t)n * h.dim);
        if (found) fnd = d_found.ensure(n);
    }
    HIPCHECK(hipMemsetAsync(d_count.ensure(1), 0, 8, s));
    gather(h, L, n, nullptr, out, fnd, d_count.p, ev, 2);
    if (!device_bufs) {
        if (vectors) HIPCHECK(hipMemcpyAsync(vectors, out, (size_t)n * h.dim * 4, hipMemcpyDeviceToHost, s));
        if (found) HIPCHECK(hipMemcpyAsync(found, fnd, n, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipMemcpyAsync(&count, d_count.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    take_timing(ev, count);
    return count;
}

void search_ids(vdb_ivf& h, const uint64_t* ids, uint32_t n, uint32_t nprobe, uint32_t k, float* distances,
                uint64_t* result_ids, uint8_t* found) {
    refuse(h, n, "search_ids");
    require(k <= (uint32_t)vdbk::kMaxK, "k above 1024 is not supported", VDB_ERR_UNSUPPORTED);
    (void)exact_probes(h, nprobe);  // (nprobe above 1024: refused as the search would)
    g_fetch_timing = FetchTiming{};
    if (n == 0) return;
    hipStream_t s = h.stream;
    const size_t nk = (size_t)n * k;
    Located L;
    DevBuf<float> d_rows, d_od;
    DevBuf<uint64_t> d_oi;
    DevBuf<uint8_t> d_found;
    DevBuf<uint32_t> d_dst;
    Events ev;
    std::vector<uint8_t> hit(n, 0);
    std::vector<uint32_t> dst(n, 0xFFFFFFFFu);
    StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

    // 1. to 3. which entries are found: their marks to the host, which numbers the found rows
    locate(h, ids, n, false, L, ev);
    gather(h, L, n, nullptr, nullptr, d_found.ensure(n), nullptr, ev, 2);
    HIPCHECK(hipMemcpyAsync(hit.data(), d_found.p, n, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    uint32_t nf = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (hit[i]) dst[i] = nf++;
    if (found) std::memcpy(found, hit.data(), n);
    std::fill(distances, distances + nk, FLT_MAX);
    std::fill(result_ids, result_ids + nk, ~0ull);
    if (nf && k) {
        // 4. the found rows, dense and in request order, into the search's query buffer
        HIPCHECK(hipMemcpyAsync(d_dst.ensure(n), dst.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        gather(h, L, n, d_dst.p, d_rows.ensure((size_t)nf * h.dim), nullptr, nullptr, ev, 3);
        // 5. one search call over them, as vdb_ivf_search_device runs it
        const size_t fk = (size_t)nf * k;
        h.search_device(d_rows.p, nf, nprobe, k, d_od.ensure(fk), d_oi.ensure(fk), s);
        std::vector<float> od(fk);
        std::vector<uint64_t> oi(fk);
        HIPCHECK(hipMemcpyAsync(od.data(), d_od.p, fk * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(oi.data(), d_oi.p, fk * 8, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < n; ++i) {
            if (!hit[i]) continue;
            std::memcpy(distances + (size_t)i * k, od.data() + (size_t)dst[i] * k, (size_t)k * 4);
            std::memcpy(result_ids + (size_t)i * k, oi.data() + (size_t)dst[i] * k, (size_t)k * 8);
        }
    }
    take_timing(ev, nf);
}

}  // namespace vdbe
