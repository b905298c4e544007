// remove_kernels.hip — device side of vdb_ivf_remove_ids (gfx950, wave64).
//
// The list arena is cut into blocks of 64 slots, [block][d4][64] float4 with the ids beside
// it: one block is one wavefront's worth of slots, so one wavefront handles one block in both
// kernels and lane i owns slot i.
//   ivf_remove_mark     lane i looks its slot's id up in the request's sorted ids; the wave's
//                       ballot is the block's 64-bit keep mask.
//   ivf_remove_compact  a kept lane's destination is the block's base plus the kept lanes
//                       below it (mbcnt over the mask); it moves its d4 float4 and its id.
//                       Reads are whole 1 KiB rows of a block; the kept lanes of a block are
//                       consecutive destination slots, so each row's writes land in at most
//                       two contiguous runs (the run may cross into the next block).
// Both take the arena by pointer only, so they serve the page-locked host arena of the
// list-cache tier as they serve HBM.
#include "remove_kernels.hpp"

#include <algorithm>

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts (blocks of 64 slots in flight) per workgroup

__device__ __forceinline__ bool listed(const uint64_t* __restrict__ sorted, uint32_t n, uint64_t id) {
    uint32_t lo = 0, hi = n;  // first element >= id
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == id;
}

__global__ __launch_bounds__(kWaves * 64) void ivf_remove_mark(const uint64_t* __restrict__ ids,
                                                                const uint32_t* __restrict__ valid, uint64_t nblocks,
                                                                const uint64_t* __restrict__ sorted, uint32_t n,
                                                                unsigned long long* __restrict__ keepmask) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t b = wave0; b < nblocks; b += nwaves) {  // (b is the same in every lane of a wave)
        bool keep = false;
        if (lane < valid[b]) keep = !listed(sorted, n, ids[b * 64 + lane]);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) keepmask[b] = m;
    }
}

__global__ __launch_bounds__(kWaves * 64) void ivf_remove_compact(const float4* __restrict__ old_arena,
                                                                   const uint64_t* __restrict__ old_ids,
                                                                   const unsigned long long* __restrict__ keepmask,
                                                                   const uint64_t* __restrict__ base, uint64_t nblocks,
                                                                   uint32_t d4, float4* __restrict__ new_arena,
                                                                   uint64_t* __restrict__ new_ids) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t b = wave0; b < nblocks; b += nwaves) {
        const unsigned long long m = keepmask[b];
        if (!((m >> lane) & 1ull)) continue;  // (no wave-wide operation follows in the body)
        // kept lanes below this one
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const uint64_t dest = base[b] + below;
        new_ids[dest] = old_ids[b * 64 + lane];
        const float4* __restrict__ src = old_arena + b * d4 * 64 + lane;
        float4* __restrict__ dst = new_arena + (dest >> 6) * d4 * 64 + (dest & 63);
#pragma unroll 8
        for (uint32_t t = 0; t < d4; ++t) dst[(uint64_t)t * 64] = src[(uint64_t)t * 64];
    }
}

uint32_t wave_grid(uint64_t nblocks) {
    // persistent: 8 workgroups of 4 waves per CU on the whole chip at most
    return (uint32_t)std::min<uint64_t>((nblocks + kWaves - 1) / kWaves, 256 * 8);
}

}  // namespace

void launch_remove_mark(const uint64_t* arena_ids, const uint32_t* valid, uint64_t nblocks, const uint64_t* sorted,
                        uint32_t n, unsigned long long* keepmask, hipStream_t s) {
    if (!nblocks) return;
    ivf_remove_mark<<<wave_grid(nblocks), kWaves * 64, 0, s>>>(arena_ids, valid, nblocks, sorted, n, keepmask);
}

void launch_remove_compact(const float4* old_arena, const uint64_t* old_ids, const unsigned long long* keepmask,
                           const uint64_t* base, uint64_t nblocks, uint32_t d4, float4* new_arena, uint64_t* new_ids,
                           hipStream_t s) {
    if (!nblocks) return;
    ivf_remove_compact<<<wave_grid(nblocks), kWaves * 64, 0, s>>>(old_arena, old_ids, keepmask, base, nblocks, d4,
                                                                new_arena, new_ids);
}

}  // namespace vdbk
