// scan_items.hip — the pair grouping in front of ivf_filter_scan and ivf_range_scan (gfx950):
// the batch's (query, probe) pairs by probed list (count, prefix, fill) and the lists' first
// scan items (scan_items.hpp). gate[l] != 0 admits list l: the filter passes its allowed rows,
// the range search the lists' counts. launch_scan_group_pairs gates per pair instead (gate[i]):
// vdb_ivf_search_prepared_multi passes the rows the pair's own filter allows in its list.
#include "scan_kernels.hpp"

namespace vdbk {
namespace {

__global__ void scan_pair_count(const uint32_t* __restrict__ probes, uint32_t BP, const uint32_t* __restrict__ gate,
                                uint32_t* __restrict__ cursor) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BP) return;
    const uint32_t l = probes[i];
    if (gate[l]) atomicAdd(&cursor[l], 1u);
}

// One workgroup: exclusive prefixes over the lists of their pairs and of their scan items;
// the per-list pair counts (cursor) are cleared for the fill pass.
__global__ __launch_bounds__(256) void scan_pair_prefix(uint32_t* __restrict__ cursor,
                                                        const uint32_t* __restrict__ count, uint32_t nlist,
                                                        uint32_t segs, uint32_t group,
                                                        uint32_t* __restrict__ pair_start,
                                                        uint32_t* __restrict__ item_start) {
    __shared__ uint32_t s_p[256], s_it[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (nlist + 255) / 256;
    const uint32_t lo = min(nlist, tid * chunk), hi = min(nlist, lo + chunk);
    auto items = [&](uint32_t l, uint32_t c) { return scan_items_of(c, group, (count[l] + 63) >> 6, segs); };
    uint32_t p = 0, it = 0;
    for (uint32_t l = lo; l < hi; ++l) {
        const uint32_t c = cursor[l];
        p += c;
        it += items(l, c);
    }
    s_p[tid] = p;
    s_it[tid] = it;
    __syncthreads();
    if (tid == 0) {
        uint32_t ap = 0, ai = 0;
        for (uint32_t t = 0; t < 256; ++t) {
            const uint32_t vp = s_p[t], vi = s_it[t];
            s_p[t] = ap;
            s_it[t] = ai;
            ap += vp;
            ai += vi;
        }
    }
    __syncthreads();
    p = s_p[tid];
    it = s_it[tid];
    for (uint32_t l = lo; l < hi; ++l) {
        const uint32_t c = cursor[l];
        pair_start[l] = p;
        item_start[l] = it;
        p += c;
        it += items(l, c);
        cursor[l] = 0;
    }
    if (tid == 255) {  // (its chunk ends at nlist: the totals)
        pair_start[nlist] = p;
        item_start[nlist] = it;
    }
}

__global__ void scan_pair_fill(const uint32_t* __restrict__ probes, uint32_t BP, const uint32_t* __restrict__ gate,
                               const uint32_t* __restrict__ pair_start, uint32_t* __restrict__ cursor,
                               uint32_t* __restrict__ inv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BP) return;
    const uint32_t l = probes[i];
    if (gate[l]) inv[pair_start[l] + atomicAdd(&cursor[l], 1u)] = i;
}

// The same two passes gated per pair (gate[i], i the pair): a list's pairs are the admitted
// ones among those that probe it.
__global__ void scan_pair_count_by_pair(const uint32_t* __restrict__ probes, uint32_t BP,
                                        const uint32_t* __restrict__ gate, uint32_t* __restrict__ cursor) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BP) return;
    if (gate[i]) atomicAdd(&cursor[probes[i]], 1u);
}

__global__ void scan_pair_fill_by_pair(const uint32_t* __restrict__ probes, uint32_t BP,
                                       const uint32_t* __restrict__ gate, const uint32_t* __restrict__ pair_start,
                                       uint32_t* __restrict__ cursor, uint32_t* __restrict__ inv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BP) return;
    const uint32_t l = probes[i];
    if (gate[i]) inv[pair_start[l] + atomicAdd(&cursor[l], 1u)] = i;
}

}  // namespace

void launch_scan_group_pairs(const uint32_t* probes, uint32_t BP, const uint32_t* gate, const uint32_t* count,
                             uint32_t nlist, uint32_t segs, uint32_t group, uint32_t* cursor, uint32_t* pair_start,
                             uint32_t* item_start, uint32_t* inv, hipStream_t s) {
    if (!BP || !nlist) return;
    (void)hipMemsetAsync(cursor, 0, (size_t)nlist * 4, s);
    scan_pair_count_by_pair<<<(BP + 255) / 256, 256, 0, s>>>(probes, BP, gate, cursor);
    scan_pair_prefix<<<1, 256, 0, s>>>(cursor, count, nlist, segs, group, pair_start, item_start);
    scan_pair_fill_by_pair<<<(BP + 255) / 256, 256, 0, s>>>(probes, BP, gate, pair_start, cursor, inv);
}

void launch_scan_group(const uint32_t* probes, uint32_t BP, const uint32_t* gate, const uint32_t* count,
                       uint32_t nlist, uint32_t segs, uint32_t group, uint32_t* cursor, uint32_t* pair_start,
                       uint32_t* item_start, uint32_t* inv, hipStream_t s) {
    if (!BP || !nlist) return;
    (void)hipMemsetAsync(cursor, 0, (size_t)nlist * 4, s);
    scan_pair_count<<<(BP + 255) / 256, 256, 0, s>>>(probes, BP, gate, cursor);
    scan_pair_prefix<<<1, 256, 0, s>>>(cursor, count, nlist, segs, group, pair_start, item_start);
    scan_pair_fill<<<(BP + 255) / 256, 256, 0, s>>>(probes, BP, gate, pair_start, cursor, inv);
}

}  // namespace vdbk
