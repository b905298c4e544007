// upsert_kernels.hip — device side of vdb_ivf_upsert's request resolution (gfx950, wave64).
//
// A request may name an id more than once; the last entry carrying it wins. Three steps:
//   sort                 hipCUB's stable radix sort of (id, request position), all 64 key bits.
//                        The sorted ids, repeats left in, are also what ivf_remove_mark's binary
//                        search reads afterwards.
//   ivf_upsert_winners   one thread per sorted entry: the last entry of a run of equal ids has
//                        the largest position (the sort is stable), so it wins; win[position].
//   pack                 the winners dense, in request order. ivf_upsert_ballot: one wavefront
//                        per 64 request entries, lane i owns entry i, the wave's ballot is the
//                        group's mask and its popcount the group's count. The exclusive sum
//                        over the cdiv(n, 64) counts is taken on the HOST (upsert.cpp), as the
//                        remove plan's sums are: the host needs the total before it can size
//                        anything that follows, so the counts travel there anyway.
//                        ivf_upsert_pack: one wavefront per request entry; a losing entry is
//                        dropped on one uniform test of its mask bit, a winner's slot is the
//                        group's base plus the mask bits below its own (what mbcnt gives the
//                        lane that owns the entry, taken uniformly here), and the wave copies
//                        its dim floats with coalesced reads: float4 where dim % 4 == 0 and
//                        both buffers are 16-byte aligned, float by float otherwise.
// The rows are packed raw: padding and (CosineDistance) the one normalisation are
// vdb_ivf::padded_rows' afterwards, as for an add.
#include "upsert_kernels.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup

__global__ __launch_bounds__(256) void ivf_upsert_winners(const uint64_t* __restrict__ sorted,
                                                          const uint32_t* __restrict__ pos, uint32_t n,
                                                          uint8_t* __restrict__ win) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
        win[pos[j]] = (j + 1 == n || sorted[j + 1] != sorted[j]) ? 1 : 0;
}

__global__ __launch_bounds__(kWaves * 64) void ivf_upsert_ballot(const uint8_t* __restrict__ win, uint32_t n,
                                                                  uint64_t ngroups,
                                                                  unsigned long long* __restrict__ mask,
                                                                  uint32_t* __restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t g = wave0; g < ngroups; g += nwaves) {  // (g is the same in every lane of a wave)
        const uint64_t i = g * 64 + lane;
        const unsigned long long m = __ballot(i < n && win[i] != 0);
        if (lane == 0) {
            mask[g] = m;
            cnt[g] = (uint32_t)__popcll(m);
        }
    }
}

template <bool VEC4>
__global__ __launch_bounds__(kWaves * 64) void ivf_upsert_pack(const float* __restrict__ rows,
                                                                const uint64_t* __restrict__ ids, uint32_t n,
                                                                uint32_t dim,
                                                                const unsigned long long* __restrict__ mask,
                                                                const uint32_t* __restrict__ base,
                                                                float* __restrict__ out_rows,
                                                                uint64_t* __restrict__ out_ids) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t i = wave0; i < n; i += nwaves) {  // (i is the same in every lane of a wave)
        const unsigned long long m = mask[i >> 6];
        const uint32_t bit = (uint32_t)(i & 63);
        if (!((m >> bit) & 1ull)) continue;
        const uint64_t slot = (uint64_t)base[i >> 6] + (uint32_t)__popcll(m & ((1ull << bit) - 1ull));
        if (lane == 0) out_ids[slot] = ids[i];
        if (VEC4) {
            const float4* __restrict__ src = (const float4*)(rows + i * dim);
            float4* __restrict__ dst = (float4*)(out_rows + slot * dim);
            for (uint32_t t = lane; t < dim / 4; t += 64) dst[t] = src[t];
        } else {
            const float* __restrict__ src = rows + i * dim;
            float* __restrict__ dst = out_rows + slot * dim;
            for (uint32_t t = lane; t < dim; t += 64) dst[t] = src[t];
        }
    }
}

uint32_t wave_grid(uint64_t nwaves) {
    // persistent: 8 workgroups of 4 waves per CU on the whole chip at most
    return (uint32_t)std::min<uint64_t>((nwaves + kWaves - 1) / kWaves, 256 * 8);
}

}  // namespace

hipError_t upsert_sort_pairs(void* temp, size_t& temp_bytes, const uint64_t* ids_in, uint64_t* ids_out,
                             const uint32_t* pos_in, uint32_t* pos_out, uint32_t n, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, ids_in, ids_out, pos_in, pos_out, (int)n, 0, 64, s);
}

void launch_upsert_winners(const uint64_t* sorted_ids, const uint32_t* pos, uint32_t n, uint8_t* win, hipStream_t s) {
    if (!n) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + 255) / 256, 256 * 8);
    ivf_upsert_winners<<<grid, 256, 0, s>>>(sorted_ids, pos, n, win);
}

void launch_upsert_ballot(const uint8_t* win, uint32_t n, unsigned long long* mask, uint32_t* cnt, hipStream_t s) {
    if (!n) return;
    const uint64_t ngroups = ((uint64_t)n + 63) / 64;
    ivf_upsert_ballot<<<wave_grid(ngroups), kWaves * 64, 0, s>>>(win, n, ngroups, mask, cnt);
}

void launch_upsert_pack(const float* rows, const uint64_t* ids, uint32_t n, uint32_t dim,
                        const unsigned long long* mask, const uint32_t* base, float* out_rows, uint64_t* out_ids,
                        hipStream_t s) {
    if (!n) return;
    const bool vec4 = dim % 4 == 0 && ((uintptr_t)rows | (uintptr_t)out_rows) % 16 == 0;
    if (vec4) ivf_upsert_pack<true><<<wave_grid(n), kWaves * 64, 0, s>>>(rows, ids, n, dim, mask, base, out_rows, out_ids);
    else ivf_upsert_pack<false><<<wave_grid(n), kWaves * 64, 0, s>>>(rows, ids, n, dim, mask, base, out_rows, out_ids);
}

}  // namespace vdbk
