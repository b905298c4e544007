// range_kernels.hip — device side of vdb_ivf_range_search (gfx950, wave64).
//
// The list arena is cut into blocks of 64 slots with the ids beside it, so one wavefront
// handles one block and lane i owns slot i, as in filter_kernels.hip.
//   ivf_range_scan    persistent workgroups of 4 waves over the items of the pair grouping
//                     (scan_items.hip with a group of 8, decoded by scan_items.hpp):
//                     one segment of one list against up to 8 of the queries that probe it (one
//                     read of a block feeds 8 distance chains, 4 for a group of at most 4). A
//                     workgroup takes its next item from one device counter. The waves take the
//                     segment's blocks in turn; a lane computes its slot's exact distance (the
//                     reference's sequential fp32 sum) per query, the queries read through the
//                     scalar cache. The threshold is the call's radius, known before the scan
//                     and never moved: no top-k, no shared state between blocks.
//                     Interleaved layout: the wave reads whole 1 KiB rows of the block.
//                     Row-major layout: the block is 64 consecutive rows of dp floats; the wave
//                     stages kRangeChunk4 float4 of every row through its own LDS tile (eight
//                     lanes read one row's 128-byte run), then lane i reads row i back, so each
//                     row's sum stays in sequence order. The next chunk of the same block is in
//                     flight while the current one is summed.
//                     A hit (slot below the block's valid count, d <= radius) is appended
//                     wave-aggregated: ballot, one atomic add of the popcount by one lane, the
//                     base broadcast, each hit lane at base + mbcnt. Past the buffer's capacity
//                     nothing is written and the cursor keeps counting.
//   ivf_range_scan_masked  the same body over the rows a prepared filter allows (MASKED): the
//                     block's 64-bit allow mask read wave-uniform through the scalar cache, a
//                     zero mask skipping the block unread, row-major staging lanes loading
//                     allowed rows only, a hit needing its lane's bit; the one thing asked for
//                     ahead is the mask word of the wave's next block of the same item. A sibling kernel with its
//                     own argument block: ivf_range_scan is instruction for instruction unchanged.
//   range_dedup       after the sorts by (query, distance) and by id: the first entry of each
//                     (id, query) run keeps its key (-0.0f folded onto +0.0f), the others get the
//                     key of no query.
//   range_finish      after the sort by that key: ids and distance bits in their final order
//                     and the batch's per-query starts.
// No kernel reads a block or an id it was not given: nothing is prefetched beyond a block, the
// arena's slack block is never touched, and ids are read for hit lanes only.
#pragma clang fp contract(off)
#include "range_kernels.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "scan_common.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup

// The wave's LDS stores land before its lanes read each other's, and the reads before the
// tile is written again (LDS operations of one wave complete in order; this keeps the
// compiler from moving them across).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef const float4 __attribute__((address_space(4))) ConstF4;
#else
typedef const float4 ConstF4;  // (the host pass only parses the kernels)
#endif
#if defined(__HIP_DEVICE_COMPILE__)
typedef const unsigned long long __attribute__((address_space(4))) ConstU64;
#else
typedef const unsigned long long ConstU64;
#endif

// The argument block of a scan: the masked kernels carry the filter's two arrays behind it.
template <bool MASKED>
struct RangeArgsOf {
    typedef RangeScanArgs type;
};
template <>
struct RangeArgsOf<true> {
    typedef RangeMaskedScanArgs type;
};

constexpr int kC4 = (int)kRangeChunk4;
// one tile per wave: 64 rows x kC4 float4, a row padded by one float4 (36 words: the 16 lanes
// a ds_read_b128 serves together fall on 16 different bank quads)
typedef float4 RangeTile[64][kC4 + 1];

// Blocks b_lo + wave, + kWaves, ... < b_hi of the list at arena block `base` (cnt rows) against
// the np <= NG queries of pairs inv[p0 ..): NG distance chains per lane, chains g >= np repeat
// the last query and are dropped.
// MASKED: the block's allow mask is one wave-uniform 64-bit word, read like the queries through
// the constant address space into SGPRs (the masks were written before the launch). A zero
// mask skips the block before any row byte is loaded. Row-major layout: a staging lane loads
// its float4 of a row only if that row's bit is set, so a sparse filter reads the allowed rows'
// bytes alone; the tile rows of the other slots hold zeros and belong to lanes that never hit.
template <int M, bool ROWS, int NG, bool MASKED>
__device__ __forceinline__ void range_scan_blocks(const typename RangeArgsOf<MASKED>::type& a,
                                                  float4 (*tile)[kC4 + 1], uint32_t p0, int np, uint32_t b_lo,
                                                  uint32_t b_hi, uint64_t base, uint32_t cnt) {
    constexpr int C4 = kC4;
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const uint32_t d4 = a.d4;
    // The queries are read through the constant address space at wave-uniform addresses, so
    // they come through the scalar cache into SGPRs (they were written before the launch);
    // as plain global reads behind the kernel's own stores they would be vector loads, NG of
    // them beside every load of list data.
    ConstF4* q4[NG];
    uint32_t qi[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        qi[g] = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.inv[p0 + (g < np ? g : np - 1)]) / a.P;
        q4[g] = (ConstF4*)(a.q + (size_t)qi[g] * d4 * 4);
    }

    // MASKED: the masks of this wave's blocks, the next one asked for while the current block is
    // summed (8 bytes of the item's own blocks, never beyond b_hi), so no block waits for its mask
    ConstU64* masks = nullptr;
    unsigned long long allow_next = 0;
    if constexpr (MASKED) {
        const uint64_t base_u = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        masks = (ConstU64*)a.allow + base_u;
        if (b_lo + wave < b_hi) allow_next = masks[b_lo + wave];
    }

    for (uint32_t b = b_lo + wave; b < b_hi; b += kWaves) {
        const uint64_t gb = base + b;
        const uint32_t valid = min(64u, cnt - b * 64);
        unsigned long long allow = ~0ull;
        if constexpr (MASKED) {
            allow = allow_next;
            if (b + kWaves < b_hi) allow_next = masks[b + kWaves];
            if (allow == 0) continue;  // (wave-uniform) no row byte of this block is read
        }
        float acc[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = 0.0f;
        if constexpr (M != kCos) {
            if constexpr (ROWS) {
                // lane l fetches float4 (l & 7) of rows (l >> 3) + 8 i of the chunk
                const float4* __restrict__ src = a.lists + (gb * 64 + (uint64_t)(lane >> 3)) * d4 + (lane & 7);
                float4 nx[8];
                // MASKED: bit 8 i of `rows_on` = row (lane >> 3) + 8 i of the block is allowed
                const unsigned long long rows_on = allow >> (lane >> 3);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if constexpr (MASKED) {
                        nx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if ((rows_on >> (8 * i)) & 1ull) nx[i] = load_nt(src + (size_t)i * 8 * d4);
                    } else {
                        nx[i] = load_nt(src + (size_t)i * 8 * d4);
                    }
                }
                for (uint32_t c = 0; c < d4; c += C4) {
                    wave_sync();  // (the previous chunk's reads are done)
#pragma unroll
                    for (int i = 0; i < 8; ++i) tile[i * 8 + (lane >> 3)][lane & 7] = nx[i];
                    if (c + C4 < d4) {  // the block's next chunk, never beyond the block
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            if constexpr (MASKED) {
                                if ((rows_on >> (8 * i)) & 1ull) nx[i] = load_nt(src + (size_t)i * 8 * d4 + c + C4);
                            } else {
                                nx[i] = load_nt(src + (size_t)i * 8 * d4 + c + C4);
                            }
                        }
                    }
                    wave_sync();
#pragma unroll
                    for (int t = 0; t < C4; ++t) {
                        const float4 x = tile[lane][t];
#pragma unroll
                        for (int g = 0; g < NG; ++g) acc[g] = acc4<M>(acc[g], q4[g][c + t], x);
                    }
                }
            } else {
                const float4* __restrict__ p = a.lists + gb * d4 * 64 + lane;
#pragma unroll 8
                for (uint32_t t = 0; t < d4; ++t) {
                    const float4 x = load_nt(p + (size_t)t * 64);
#pragma unroll
                    for (int g = 0; g < NG; ++g) acc[g] = acc4<M>(acc[g], q4[g][t], x);
                }
            }
        }
        uint64_t id = 0;
        bool have_id = false;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g < np) {  // (wave-uniform)
                const float dv = dist_finish<M>(acc[g]);
                bool hit = (uint32_t)lane < valid && dv <= a.radius;  // (false for a NaN distance)
                if constexpr (MASKED) hit = hit && ((allow >> lane) & 1ull);
                const unsigned long long m = __ballot(hit);
                if (m) {  // (wave-uniform)
                    if (hit && !have_id) {
                        id = a.ids[gb * 64 + lane];
                        have_id = true;
                    }
                    unsigned long long at = 0;
                    if (lane == 0) at = atomicAdd(a.ctrl + kRangeCursor, (unsigned long long)__popcll(m));
                    at = rd_lane((uint64_t)at, 0);
                    at += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (hit && at < a.cap) {
                        a.hit_key[at] = ((uint64_t)qi[g] << 32) | ord_enc(dv);
                        a.hit_id[at] = id;
                    }
                }
            }
        }
    }
}

template <int M, bool ROWS, bool MASKED>
__device__ __forceinline__ void range_scan_body(const typename RangeArgsOf<MASKED>::type& a) {
    constexpr int G = (int)kRangeGroup;
    constexpr int C4 = kC4;
    __shared__ RangeTile s_x[ROWS ? kWaves : 1];
    const uint32_t wave = wave_index();
    const uint32_t d4 = a.d4;
    if (d4 == 0 || d4 % C4 != 0) {  // (the host guard refuses this first: range_scan_serves)
        if (threadIdx.x == 0) atomicOr(a.ctrl + kRangeStatus, kRangeUnserved);
        return;
    }
    const uint32_t total = a.item_start[a.nlist];
    __shared__ uint32_t s_item;
    for (;;) {
        // the workgroup's next item, from one counter: items differ in length (a short list's
        // segment, a short group), so the workgroups take them as they come
        if (threadIdx.x == 0) s_item = (uint32_t)atomicAdd(a.ctrl + kRangeNext, 1ull);
        __syncthreads();
        const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_item);  // (the same in every wave)
        __syncthreads();               // (read by all before thread 0 writes the next)
        if (item >= total) break;
        const ExactScanItem it = decode_scan_item<kRangeGroup>(item, a.item_start, a.pair_start, a.count, a.nlist, a.segs);
        const int np = (int)it.np;  // >= 1; slots g >= np repeat the last query
        const uint32_t cnt = a.count[it.list];
        const uint64_t base = a.block_off[it.list];
        if constexpr (MASKED) {
            if (it.seg == 0 && threadIdx.x == 0)
                atomicAdd(a.ctrl + kRangePairs, (unsigned long long)np * a.allowed[it.list]);
        } else {
            if (it.seg == 0 && threadIdx.x == 0) atomicAdd(a.ctrl + kRangePairs, (unsigned long long)np * cnt);
        }
        // (half the chains for a short group: a list few of the batch's queries probe)
        if (np <= G / 2)
            range_scan_blocks<M, ROWS, G / 2, MASKED>(a, s_x[ROWS ? wave : 0], it.p0, np, it.b_lo, it.b_hi, base, cnt);
        else range_scan_blocks<M, ROWS, G, MASKED>(a, s_x[ROWS ? wave : 0], it.p0, np, it.b_lo, it.b_hi, base, cnt);
    }
}

template <int M, bool ROWS>
__global__ __launch_bounds__(kWaves * 64) void ivf_range_scan(const RangeScanArgs a) {
    range_scan_body<M, ROWS, false>(a);
}

// The scan of vdb_ivf_range_search_prepared: a sibling kernel, so ivf_range_scan stays as it is.
template <int M, bool ROWS>
__global__ __launch_bounds__(kWaves * 64) void ivf_range_scan_masked(const RangeMaskedScanArgs a) {
    range_scan_body<M, ROWS, true>(a);
}

// -0.0f and +0.0f are one key (key_less compares them equal; the id breaks the tie).
__device__ __forceinline__ uint32_t fold_zero(uint32_t enc) { return enc == 0x7FFFFFFFu ? 0x80000000u : enc; }

// key / id: sorted by id, within an id by (query, distance). out_key[i] is the entry's key
// for the final sort, (B, 0) for a repeat of its (id, query); perm[i] = i.
__global__ void range_dedup(const uint64_t* __restrict__ key, const uint64_t* __restrict__ id, uint32_t m, uint32_t B,
                            uint64_t* __restrict__ out_key, uint32_t* __restrict__ perm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = key[i];
    const bool repeat = i > 0 && id[i] == id[i - 1] && (k >> 32) == (key[i - 1] >> 32);
    out_key[i] = repeat ? ((uint64_t)B << 32) : ((k & 0xFFFFFFFF00000000ull) | fold_zero((uint32_t)k));
    perm[i] = i;
}

// skey / perm: the final order (repeats last). Entry i of a query takes the id and the computed
// distance bits of its source; start[q] is the first entry of batch query q, start[B] the
// number of entries.
__global__ void range_finish(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm,
                             const uint64_t* __restrict__ key, const uint64_t* __restrict__ id, uint32_t m, uint32_t B,
                             uint64_t* __restrict__ out_i, float* __restrict__ out_d, uint32_t* __restrict__ start) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t q = min((uint32_t)(skey[i] >> 32), B);
    const int64_t prev = i ? (int64_t)min((uint32_t)(skey[i - 1] >> 32), B) : -1;
    for (int64_t x = prev + 1; x <= (int64_t)q; ++x) start[x] = i;
    if (i == m - 1)
        for (uint32_t x = q + 1; x <= B; ++x) start[x] = m;
    if (q < B) {
        const uint32_t j = perm[i];
        out_i[i] = id[j];
        out_d[i] = ord_dec((uint32_t)key[j]);
    }
}

template <int M>
void scan_metric(const RangeScanArgs& a, hipStream_t s) {
    // persistent over the items (their number is known on the device only): the workgroups the
    // whole chip holds at once, 4 per CU in the row-major layout (its LDS tiles), 8 otherwise
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)a.B * a.P * a.segs, 256 * (a.rows ? 4 : 8));
    if (a.rows) ivf_range_scan<M, true><<<grid, kWaves * 64, 0, s>>>(a);
    else ivf_range_scan<M, false><<<grid, kWaves * 64, 0, s>>>(a);
}

template <int M>
void scan_metric_masked(const RangeMaskedScanArgs& a, hipStream_t s) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)a.B * a.P * a.segs, 256 * (a.rows ? 4 : 8));
    if (a.rows) ivf_range_scan_masked<M, true><<<grid, kWaves * 64, 0, s>>>(a);
    else ivf_range_scan_masked<M, false><<<grid, kWaves * 64, 0, s>>>(a);
}

// Key bits of a batch of B queries: the distance's 32 and enough for the query values 0 .. B.
int key_bits(uint32_t B) {
    int qb = 1;
    while (qb < 32 && (B >> qb)) ++qb;
    return 32 + qb;
}

}  // namespace

void launch_range_scan(int metric, const RangeScanArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) scan_metric<kL2>(a, s);
    else if (metric == kIP) scan_metric<kIP>(a, s);
    else scan_metric<kCos>(a, s);
}

void launch_range_scan_masked(int metric, const RangeMaskedScanArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) scan_metric_masked<kL2>(a, s);
    else if (metric == kIP) scan_metric_masked<kIP>(a, s);
    else scan_metric_masked<kCos>(a, s);
}

hipError_t range_order_temp_bytes(uint64_t m, uint32_t B, size_t& bytes) {
    size_t t1 = 0, t2 = 0, t3 = 0;
    const uint64_t* k64 = nullptr;
    uint64_t* o64 = nullptr;
    const uint32_t* k32 = nullptr;
    uint32_t* o32 = nullptr;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, t1, k64, o64, k64, o64, (int)m, 0, key_bits(B), nullptr);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairs(nullptr, t2, k64, o64, k64, o64, (int)m, 0, 64, nullptr);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairs(nullptr, t3, k64, o64, k32, o32, (int)m, 0, key_bits(B), nullptr);
    bytes = std::max(t1, std::max(t2, t3));
    return e;
}

hipError_t launch_range_order(const RangeOrderBufs& b, uint64_t m, uint32_t B, hipStream_t s) {
    if (!m || !B) return hipSuccess;
    const int bits = key_bits(B);
    const uint32_t grid = (uint32_t)((m + 255) / 256);
    size_t tb = b.temp_bytes;
    // by (query, distance) ...
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(b.temp, tb, (const uint64_t*)b.key_a, b.key_b,
                                                      (const uint64_t*)b.id_a, b.id_b, (int)m, 0, bits, s);
    if (e != hipSuccess) return e;
    // ... then by id (stable: an id's entries stay in (query, distance) order)
    tb = b.temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(b.temp, tb, (const uint64_t*)b.id_b, b.id_a, (const uint64_t*)b.key_b,
                                           b.key_a, (int)m, 0, 64, s);
    if (e != hipSuccess) return e;
    range_dedup<<<grid, 256, 0, s>>>(b.key_a, b.id_a, (uint32_t)m, B, b.key_b, b.perm_a);
    // by (query, distance) again, repeats last (stable: equal keys stay in id order)
    tb = b.temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(b.temp, tb, (const uint64_t*)b.key_b, b.id_b, (const uint32_t*)b.perm_a,
                                           b.perm_b, (int)m, 0, bits, s);
    if (e != hipSuccess) return e;
    range_finish<<<grid, 256, 0, s>>>(b.id_b, b.perm_b, b.key_a, b.id_a, (uint32_t)m, B, b.key_b, (float*)b.perm_a,
                                      b.start);
    return hipGetLastError();
}

}  // namespace vdbk
