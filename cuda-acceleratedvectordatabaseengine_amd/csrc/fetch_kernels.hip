// fetch_kernels.hip — device side of vdb_ivf_fetch_ids / vdb_ivf_search_ids (gfx950, wave64).
//
// The lists store (row, id) by slot; a fetch needs the reverse map for the few ids a request
// names. The request is sorted (launch_filter_sort), and then
//   ivf_fetch_locate  one wave per 64-slot arena block, lane = slot, as ivf_remove_mark: a lane
//                     whose slot holds a row takes the lower bound of its id in the sorted
//                     request and, on equality, a 64-bit atomicMin of its global slot on loc[j].
//                     Arena blocks ascend with the list id (vdb_ivf::relayout and remove_plan
//                     both pack the lists in list order) and slots with the add order, so the
//                     minimum is the row at the lowest (list, position). 8 bytes read per
//                     stored row, nothing else of the lists.
//   ivf_fetch_gather  one wave per request entry: the lower bound of its id among the sorted
//                     ids, loc[j], then lanes t = lane, lane + 64, .. copy float4 t of the row:
//                     from the interleaved arena d4-strided 16-byte reads (inherent to that
//                     layout), from the row-major copy one contiguous run.
#include "fetch_kernels.hpp"

#include <algorithm>

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup

// first j with sorted[j] >= id (n if none)
__device__ __forceinline__ uint32_t first_at_least(const uint64_t* __restrict__ sorted, uint32_t n, uint64_t id) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kWaves * 64) void ivf_fetch_locate(const uint64_t* __restrict__ ids,
                                                                 const uint32_t* __restrict__ valid, uint64_t nblocks,
                                                                 const uint64_t* __restrict__ sorted, uint32_t n,
                                                                 unsigned long long* __restrict__ loc) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t b = wave0; b < nblocks; b += nwaves) {  // (no wave-wide operation in the body)
        if (lane >= valid[b]) continue;
        const uint64_t slot = b * 64 + lane;
        const uint64_t id = ids[slot];
        const uint32_t j = first_at_least(sorted, n, id);
        if (j < n && sorted[j] == id) atomicMin(&loc[j], (unsigned long long)slot);
    }
}

// ROWS: the row-major copy; VEC: dim % 4 == 0 and out 16-byte aligned (float4 stores)
template <bool ROWS, bool VEC>
__global__ __launch_bounds__(kWaves * 64) void ivf_fetch_gather(const float4* __restrict__ lists, uint32_t d4,
                                                                 uint32_t dim, const uint64_t* __restrict__ req,
                                                                 uint32_t n, const uint64_t* __restrict__ sorted,
                                                                 const unsigned long long* __restrict__ loc,
                                                                 const uint32_t* __restrict__ dst,
                                                                 float* __restrict__ out, uint8_t* __restrict__ found,
                                                                 unsigned long long* __restrict__ n_found) {
    __shared__ uint32_t wave_hits[kWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    const uint32_t r4 = (dim + 3) / 4;  // float4 of a row that hold one of its dim floats
    uint32_t hits = 0;
    for (uint64_t i = wave0; i < n; i += nwaves) {  // (i is the same in every lane of a wave)
        const uint64_t id = req[i];
        const uint32_t j = first_at_least(sorted, n, id);  // (sorted holds every requested id: j < n)
        const unsigned long long slot = j < n ? loc[j] : kFetchNone;
        const bool hit = slot != kFetchNone;
        hits += hit ? 1u : 0u;
        if (found && lane == 0) found[i] = hit ? 1 : 0;
        const uint64_t o = dst ? dst[i] : i;
        if (!out || (dst && o == 0xFFFFFFFFull)) continue;
        const uint64_t sl = hit ? slot : 0;  // (no row: nothing is read)
        const float4* __restrict__ src = ROWS ? lists + sl * d4 : lists + (sl >> 6) * d4 * 64 + (sl & 63);
        for (uint32_t t = lane; t < r4; t += 64) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (hit) v = ROWS ? src[t] : src[(uint64_t)t * 64];
            if (VEC) {
                reinterpret_cast<float4*>(out)[o * r4 + t] = v;
            } else {
                float* __restrict__ p = out + o * dim;
                const uint32_t c = 4 * t;  // (c < dim)
                p[c] = v.x;
                if (c + 1 < dim) p[c + 1] = v.y;
                if (c + 2 < dim) p[c + 2] = v.z;
                if (c + 3 < dim) p[c + 3] = v.w;
            }
        }
    }
    // the found entries: one atomic per workgroup
    if (lane == 0) wave_hits[wave] = hits;
    __syncthreads();
    if (n_found && threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (uint32_t w = 0; w < kWaves; ++w) sum += wave_hits[w];
        if (sum) atomicAdd(n_found, sum);
    }
}

uint32_t wave_grid(uint64_t waves) {
    // persistent: 8 workgroups of 4 waves per CU on the whole chip at most
    return (uint32_t)std::min<uint64_t>((waves + kWaves - 1) / kWaves, 256 * 8);
}

}  // namespace

void launch_fetch_locate(const uint64_t* arena_ids, const uint32_t* valid, uint64_t nblocks, const uint64_t* sorted,
                         uint32_t n, unsigned long long* loc, hipStream_t s) {
    if (!nblocks || !n) return;
    ivf_fetch_locate<<<wave_grid(nblocks), kWaves * 64, 0, s>>>(arena_ids, valid, nblocks, sorted, n, loc);
}

void launch_fetch_gather(const float4* lists, int rows, uint32_t d4, uint32_t dim, const uint64_t* req, uint32_t n,
                         const uint64_t* sorted, const unsigned long long* loc, const uint32_t* dst, float* out,
                         uint8_t* found, unsigned long long* n_found, hipStream_t s) {
    if (!n) return;
    const bool vec = dim % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const uint32_t grid = wave_grid(n);
#define VDB_FETCH_GATHER(R, V)                                                                                        \
    ivf_fetch_gather<R, V><<<grid, kWaves * 64, 0, s>>>(lists, d4, dim, req, n, sorted, loc, dst, out, found, n_found)
    if (rows) {
        if (vec) VDB_FETCH_GATHER(true, true);
        else VDB_FETCH_GATHER(true, false);
    } else {
        if (vec) VDB_FETCH_GATHER(false, true);
        else VDB_FETCH_GATHER(false, false);
    }
#undef VDB_FETCH_GATHER
}

}  // namespace vdbk
