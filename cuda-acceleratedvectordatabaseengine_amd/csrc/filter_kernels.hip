// filter_kernels.hip — device side of vdb_ivf_search_filtered (gfx950, wave64).
//
// The list arena is cut into blocks of 64 slots with the ids beside it, so one wavefront
// handles one block and lane i owns slot i, as in remove_kernels.hip.
//   ivf_filter_mark   lane i looks its slot's id up in the call's sorted filter ids; the wave's
//                     ballot is the block's 64-bit allow mask (pad slots never set).
//   ivf_filter_count  per list the popcount of its blocks' masks.
//   ivf_filter_scan   one workgroup of 4 waves per item of the pair grouping (scan_items.hip,
//                     decoded by scan_items.hpp): one segment of one list against up to
//                     4 of the queries that probe it (one read of a block feeds 4 distance
//                     chains). The waves take the segment's blocks in turn, skip a block whose
//                     mask is zero without touching its rows, and compute the exact distance
//                     (the reference's sequential fp32 sum) of the allowed lanes only.
//                     Interleaved layout: the wave reads whole 1 KiB rows of the block.
//                     Row-major layout: a lane's row is dp consecutive floats, so only the
//                     allowed lanes load, each its own row in 128-byte runs. Each wave keeps a WaveTopK<1> per query; wave
//                     g folds the four waves' lists of query g through LDS into the segment's
//                     top-k.
//   ivf_filter_fold   (lists cut into segments) per pair the top-k of its segments.
//   ivf_filter_merge  per query the unique-id top-k of its P slot lists, with the reference's
//                     stale-slot reuse where "empty list" reads "no allowed row";
//   ivf_filter_carry  the slot content that survives into the call's next batch.
// No kernel reads a block, an id or a slot list it was not given: nothing is prefetched
// beyond a segment, and the arena's slack block is never touched.
#pragma clang fp contract(off)
#include "filter_kernels.hpp"

#include <algorithm>
#include <cfloat>

#include "filter_offer.hpp"
#include "scan_common.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup

__device__ __forceinline__ bool listed(const uint64_t* __restrict__ sorted, uint32_t n, uint64_t id) {
    uint32_t lo = 0, hi = n;  // first element >= id
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == id;
}

__global__ __launch_bounds__(kWaves * 64) void ivf_filter_mark(const uint64_t* __restrict__ ids,
                                                                const uint32_t* __restrict__ valid, uint64_t nblocks,
                                                                const uint64_t* __restrict__ sorted, uint32_t n,
                                                                int include, unsigned long long* __restrict__ allow) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t b = wave0; b < nblocks; b += nwaves) {  // (b is the same in every lane of a wave)
        bool ok = false;
        if (lane < valid[b]) ok = listed(sorted, n, ids[b * 64 + lane]) == (include != 0);
        const unsigned long long m = __ballot(ok);
        if (lane == 0) allow[b] = m;
    }
}

__global__ __launch_bounds__(kWaves * 64) void ivf_filter_count(const unsigned long long* __restrict__ allow,
                                                                 const uint64_t* __restrict__ block_off,
                                                                 const uint32_t* __restrict__ count, uint32_t nlist,
                                                                 uint32_t* __restrict__ allowed) {
    const uint32_t l = blockIdx.x * kWaves + wave_index();
    if (l >= nlist) return;
    const uint32_t nb = (count[l] + 63) >> 6;
    const unsigned long long* m = allow + block_off[l];
    uint32_t sum = 0;
    for (uint32_t b = lane_id(); b < nb; b += 64) sum += (uint32_t)__popcll(m[b]);
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) sum += (uint32_t)__shfl_xor((int)sum, x);
    if (lane_id() == 0) allowed[l] = sum;
}

template <int M, bool ROWS>
__global__ __launch_bounds__(kWaves * 64) void ivf_filter_scan(const FilterScanArgs a) {
    constexpr int G = (int)kFilterGroup;
    static_assert(kFilterGroup <= kWaves, "one wave folds one query of the group");
    __shared__ float s_d[kWaves][G][64];
    __shared__ uint64_t s_i[kWaves][G][64];
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const uint32_t d4 = a.d4;
    const int k = (int)a.k;
    const uint32_t total = a.item_start[a.nlist];
    for (uint32_t item = blockIdx.x; item < total; item += gridDim.x) {  // (the same in every wave)
        const ExactScanItem it = decode_scan_item<kFilterGroup>(item, a.item_start, a.pair_start, a.count, a.nlist, a.segs);
        const uint32_t seg = it.seg, p0 = it.p0, b_lo = it.b_lo, b_hi = it.b_hi;
        const int np = (int)it.np;  // >= 1; slots g >= np repeat the last query
        const uint64_t base = a.block_off[it.list];
        const float4* __restrict__ q4[G];  // (wave-uniform reads)
#pragma unroll
        for (int g = 0; g < G; ++g)
            q4[g] = (const float4*)(a.q + (size_t)(a.inv[p0 + (g < np ? g : np - 1)] / a.P) * d4 * 4);

        WaveTopK<1> tk[G];
        float kd[G];
        uint64_t ki[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            tk[g].init();
            kd[g] = __builtin_inff();
            ki[g] = kNoId;
        }
        for (uint32_t b = b_lo + wave; b < b_hi; b += kWaves) {
            const uint64_t gb = base + b;
            const unsigned long long m = a.allow[gb];
            if (m == 0) continue;  // no row byte of this block is read
            const bool mine = (m >> lane) & 1ull;
            float acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.0f;
            if constexpr (M != kCos) {
                if constexpr (ROWS) {
                    if (mine) {
                        const float4* __restrict__ p = a.lists + (gb * 64 + (uint64_t)lane) * d4;
#pragma unroll 8
                        for (uint32_t t = 0; t < d4; ++t) {
                            const float4 x = p[t];
#pragma unroll
                            for (int g = 0; g < G; ++g) acc[g] = acc4<M>(acc[g], q4[g][t], x);
                        }
                    }
                } else {
                    const float4* __restrict__ p = a.lists + gb * d4 * 64 + lane;
#pragma unroll 8
                    for (uint32_t t = 0; t < d4; ++t) {
                        const float4 x = load_nt(p + (size_t)t * 64);
#pragma unroll
                        for (int g = 0; g < G; ++g) acc[g] = acc4<M>(acc[g], q4[g][t], x);
                    }
                }
            }
            const uint64_t id = mine ? a.ids[gb * 64 + lane] : kNoId;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g < np) {
                    const float dv = dist_finish<M>(acc[g]);
                    offer_lanes<1>(tk[g], mine && dv <= kd[g], dv, id, k, kd[g], ki[g]);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            s_d[wave][g][lane] = tk[g].d[0];
            s_i[wave][g][lane] = tk[g].id[0];
        }
        __syncthreads();
        if ((int)wave < np) {  // wave g folds the four waves' lists of the group's query g
            WaveTopK<1> f;
            f.d[0] = s_d[0][wave][lane];
            f.id[0] = s_i[0][wave][lane];
            float fkd;
            uint64_t fki;
            f.at(k - 1, fkd, fki);
            for (uint32_t w = 1; w < kWaves; ++w) {
                const float dv = s_d[w][wave][lane];
                const uint64_t iv = s_i[w][wave][lane];
                offer_lanes<1>(f, dv <= fkd, dv, iv, k, fkd, fki);
            }
            if (lane < k) {
                const size_t o = ((size_t)a.inv[p0 + wave] * a.segs + seg) * k + lane;
                a.part_d[o] = f.d[0];
                a.part_i[o] = f.id[0];
            }
        }
        __syncthreads();  // (the lists in LDS are read before the next item's are written)
    }
}

__global__ __launch_bounds__(kWaves * 64) void ivf_filter_fold(const float* __restrict__ part_d,
                                                                const uint64_t* __restrict__ part_i,
                                                                const uint32_t* __restrict__ probes,
                                                                const uint32_t* __restrict__ allowed,
                                                                const uint32_t* __restrict__ count, uint32_t BP,
                                                                uint32_t segs, uint32_t k, float* __restrict__ slot_d,
                                                                uint64_t* __restrict__ slot_i) {
    const uint32_t i = blockIdx.x * kWaves + wave_index();
    if (i >= BP) return;
    const uint32_t list = probes[i];
    if (allowed[list] == 0) return;  // (the scan wrote no partial)
    const int lane = lane_id();
    WaveTopK<1> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    const uint32_t n = scan_segs((count[list] + 63) >> 6, segs) * k;  // the list's segments are the pair's first
    const size_t base = (size_t)i * segs * k;
    for (uint32_t e0 = 0; e0 < n; e0 += 64) {
        const uint32_t e = e0 + lane;
        const bool v = e < n;
        const float dv = v ? part_d[base + e] : __builtin_inff();
        const uint64_t iv = v ? part_i[base + e] : kNoId;
        offer_lanes<1>(tk, v && dv <= kd, dv, iv, (int)k, kd, ki);
    }
    if ((uint32_t)lane < k) {
        slot_d[(size_t)i * k + lane] = tk.d[0];
        slot_i[(size_t)i * k + lane] = tk.id[0];
    }
}

// (offer_slot_unique: filter_offer.hpp, shared with multi_filter_kernels.hip)
__global__ __launch_bounds__(kWaves * 64) void ivf_filter_merge(const uint32_t* __restrict__ probes,
                                                                 const uint32_t* __restrict__ allowed,
                                                                 const float* __restrict__ slot_d,
                                                                 const uint64_t* __restrict__ slot_i,
                                                                 const float* __restrict__ carry_d,
                                                                 const uint64_t* __restrict__ carry_i, uint32_t B,
                                                                 uint32_t P, uint32_t k, int stale,
                                                                 float* __restrict__ out_d, uint64_t* __restrict__ out_i,
                                                                 unsigned long long* __restrict__ pairs) {
    const uint32_t q = blockIdx.x * kWaves + wave_index();
    if (q >= B) return;
    const int lane = lane_id();
    WaveTopK<1> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    unsigned long long rows = 0;  // this lane's share of the query's allowed rows
    for (uint32_t p = lane; p < P; p += 64) rows += allowed[probes[(size_t)q * P + p]];
    for (uint32_t p = 0; p < P; ++p) {
        const float* sd = nullptr;
        const uint64_t* si = nullptr;
        if (allowed[probes[(size_t)q * P + p]] > 0) {
            sd = slot_d + ((size_t)q * P + p) * k;
            si = slot_i + ((size_t)q * P + p) * k;
        } else if (stale) {
            uint32_t q2 = q;
            bool found = false;
            while (q2 > 0) {
                --q2;
                if (allowed[probes[(size_t)q2 * P + p]] > 0) {
                    found = true;
                    break;
                }
            }
            if (found) {
                sd = slot_d + ((size_t)q2 * P + p) * k;
                si = slot_i + ((size_t)q2 * P + p) * k;
            } else {  // an earlier batch of the call (ids UINT64_MAX where there is none)
                sd = carry_d + (size_t)p * k;
                si = carry_i + (size_t)p * k;
            }
        }
        if (sd) offer_slot_unique(tk, sd, si, k, kd, ki);
    }
    if ((uint32_t)lane < k) {
        const bool real = tk.id[0] != kNoId;
        out_d[(size_t)q * k + lane] = real ? tk.d[0] : FLT_MAX;
        out_i[(size_t)q * k + lane] = tk.id[0];
    }
    if (rows) atomicAdd(pairs, rows);
}

__global__ void ivf_filter_carry(const uint32_t* __restrict__ probes, const uint32_t* __restrict__ allowed, uint32_t B,
                                 uint32_t P, uint32_t k, const float* __restrict__ slot_d,
                                 const uint64_t* __restrict__ slot_i, float* __restrict__ carry_d,
                                 uint64_t* __restrict__ carry_i) {
    __shared__ int s_q;
    const uint32_t p = blockIdx.x;
    if (threadIdx.x == 0) {
        int found = -1;
        for (int q = (int)B - 1; q >= 0; --q)
            if (allowed[probes[(size_t)q * P + p]] > 0) {
                found = q;
                break;
            }
        s_q = found;
    }
    __syncthreads();
    if (s_q < 0) return;  // the carry keeps what it has
    const size_t src = ((size_t)s_q * P + p) * k;
    for (uint32_t e = threadIdx.x; e < k; e += blockDim.x) {
        carry_d[(size_t)p * k + e] = slot_d[src + e];
        carry_i[(size_t)p * k + e] = slot_i[src + e];
    }
}

uint32_t wave_grid(uint64_t nblocks) {
    // persistent: 8 workgroups of 4 waves per CU on the whole chip at most
    return (uint32_t)std::min<uint64_t>((nblocks + kWaves - 1) / kWaves, 256 * 8);
}

template <int M>
void scan_metric(const FilterScanArgs& a, hipStream_t s) {
    // persistent over the items (their number is known on the device only): 8 workgroups per CU at most
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)a.B * a.P * a.segs, 256 * 8);
    if (a.rows) ivf_filter_scan<M, true><<<grid, kWaves * 64, 0, s>>>(a);
    else ivf_filter_scan<M, false><<<grid, kWaves * 64, 0, s>>>(a);
}

}  // namespace

void launch_filter_mark(const uint64_t* arena_ids, const uint32_t* valid, uint64_t nblocks, const uint64_t* sorted,
                        uint32_t n, int include, unsigned long long* allow, hipStream_t s) {
    if (!nblocks) return;
    ivf_filter_mark<<<wave_grid(nblocks), kWaves * 64, 0, s>>>(arena_ids, valid, nblocks, sorted, n, include, allow);
}

void launch_filter_count(const unsigned long long* allow, const uint64_t* block_off, const uint32_t* count,
                         uint32_t nlist, uint32_t* allowed, hipStream_t s) {
    if (!nlist) return;
    ivf_filter_count<<<(nlist + kWaves - 1) / kWaves, kWaves * 64, 0, s>>>(allow, block_off, count, nlist, allowed);
}

void launch_filter_scan(int metric, const FilterScanArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) scan_metric<kL2>(a, s);
    else if (metric == kIP) scan_metric<kIP>(a, s);
    else scan_metric<kCos>(a, s);
}

void launch_filter_fold(const float* part_d, const uint64_t* part_i, const uint32_t* probes, const uint32_t* allowed,
                        const uint32_t* count, uint32_t BP, uint32_t segs, uint32_t k, float* slot_d, uint64_t* slot_i,
                        hipStream_t s) {
    if (!BP) return;
    ivf_filter_fold<<<(BP + kWaves - 1) / kWaves, kWaves * 64, 0, s>>>(part_d, part_i, probes, allowed, count, BP, segs,
                                                                    k, slot_d, slot_i);
}

void launch_filter_merge(const uint32_t* probes, const uint32_t* allowed, const float* slot_d, const uint64_t* slot_i,
                         float* carry_d, uint64_t* carry_i, uint32_t B, uint32_t P, uint32_t k, int stale,
                         float* out_d, uint64_t* out_i, unsigned long long* pairs, hipStream_t s) {
    if (!B) return;
    ivf_filter_merge<<<(B + kWaves - 1) / kWaves, kWaves * 64, 0, s>>>(probes, allowed, slot_d, slot_i, carry_d, carry_i,
                                                                    B, P, k, stale, out_d, out_i, pairs);
    if (stale) ivf_filter_carry<<<P, 64, 0, s>>>(probes, allowed, B, P, k, slot_d, slot_i, carry_d, carry_i);
}

}  // namespace vdbk
