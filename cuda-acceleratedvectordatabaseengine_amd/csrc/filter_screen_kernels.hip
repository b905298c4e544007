// filter_screen_kernels.hip — device side of vdb_ivf_search_prepared_screened (gfx950, wave64).
//
// A filtered top-k through the screen in two passes over the shadow and one over the few rows
// that survive. The threshold of the pruning pass is computed before it, not during it, so the
// kernels share no moving state and the candidate set is a function of the inputs alone.
//
//   ivf_filter_screen_thresh  persistent workgroups of 4 waves over the items of the pair
//                      grouping (scan_items.hip with a group of 16, gated by the filter's allowed
//                      counts): one segment of one list against up to 16 of the pairs that probe
//                      it, the 16 rows of one MFMA A operand. The waves take the segment's blocks
//                      in turn and skip a block whose allow mask is zero unread. Per block a wave
//                      streams the shadow through the matrix cores (screen_bound.hpp) and forms
//                      the upper bound ub = approx + del of its 64 x 16 (slot, pair)s. The MFMA D
//                      layout spreads a pair's 64 slots over 16 lanes x 4 registers; the wave
//                      turns it through its LDS tile [pair][slot] so that lane i holds slot i,
//                      and keeps per pair the k smallest ub seen so far as one sorted float per
//                      lane, in LDS beside the tile (sixteen lists in registers would cost the
//                      second workgroup per CU). A pair's row is touched only when a lane beats
//                      the pair's current k-th (one ballot); then few lanes insert one by one and
//                      many go through a bitonic sort and merge, as offer_lanes does. The four
//                      waves' lists of a pair are merged by one wave (bitonic merges of sorted
//                      lists); with one segment per list that is tau, else the segment's k values
//                      go to `part` and ivf_filter_screen_tau folds the segments.
//                      A slot at or above the list's count, a slot the mask leaves out and a NaN
//                      ub read +inf and never beat a k-th, so they never count.
//   ivf_filter_screen_bound   the same items and the same stream; a (pair, slot) below the count
//                      with its allow bit set is a candidate unless lb = approx - del > tau[pair].
//                      The block's candidates are appended wave-aggregated (sixteen ballots, one
//                      atomic add by one lane) as (pair << 32) | arena slot. Past the capacity
//                      nothing is written and the cursor keeps counting.
//   ivf_filter_screen_select  one wave per pair over its run of the sorted candidates (found by
//                      two binary searches), 64 at a time: the rows are staged through the wave's
//                      LDS tile as ivf_range_recheck stages them (eight lanes per 128-byte run,
//                      the next chunk in flight), lane i reads row i back and sums in sequence
//                      order; (d, id) goes to a WaveTopK<1> exactly as ivf_filter_scan offers it.
// No kernel reads a shadow byte, a row or an id beyond the item's own blocks or the candidates'
// own slots.
#pragma clang fp contract(off)
#include "filter_screen_kernels.hpp"

#include <algorithm>

#include "scan_common.hpp"
#include "screen_bound.hpp"
#include "screen_klist.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup
constexpr int G = (int)kFilterScreenGroup;

__device__ __forceinline__ sbound::BoundSrc bound_src(const FilterScreenArgs& a) {
    return sbound::BoundSrc{a.shadow, a.meta, a.sscale, a.pst, a.qscale, a.dp};
}

__device__ __forceinline__ bool bad_shape(const FilterScreenArgs& a, bool i8) {
    return a.dp == 0 || a.dp % (i8 ? 64u : 32u) != 0 || a.k < 1 || a.k > kFilterScreenMaxK;
}

template <int M, bool I8>
__global__ __launch_bounds__(kWaves * 64, 2) void ivf_filter_screen_thresh(const FilterScreenArgs a) {
    __shared__ float s_tile[kWaves][G][64];  // a block's ub, [pair][slot]
    __shared__ float s_list[kWaves][G][64];  // per pair the wave's k smallest so far
    __shared__ uint32_t s_item;
    if (bad_shape(a, I8)) {  // (the host guard refuses this first: filter_screen_serves_shape)
        if (threadIdx.x == 0) atomicOr(a.ctrl + kFsStatus, kRangeUnserved);
        return;
    }
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const int k = (int)a.k;
    const float inf = __builtin_inff();
    const sbound::BoundSrc src = bound_src(a);
    const uint32_t total = a.item_start[a.nlist];
    for (;;) {
        const uint32_t item = next_item(a.ctrl, kFsNextT, &s_item);
        if (item >= total) break;
        const ExactScanItem it =
            decode_scan_item<kFilterScreenGroup>(item, a.item_start, a.pair_start, a.count, a.nlist, a.segs);
        const int np = (int)it.np;
        if (np < 1 || np > G) {  // (never decoded: an item is one A operand at most)
            if (threadIdx.x == 0) atomicOr(a.ctrl + kFsStatus, kRangeUnserved);
            continue;
        }
        const uint32_t cnt = a.count[it.list];
        const uint64_t base = a.block_off[it.list];
        const uint4* qa_row = sbound::a_row<I8>(a.qres, a.inv, it.p0, np, a.dp, lane);
        uint32_t pr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pr[r] = a.inv[it.p0 + (uint32_t)min(4 * (lane >> 4) + r, np - 1)];
#pragma unroll
        for (int p = 0; p < G; ++p) s_list[wave][p][lane] = inf;
        float kdv = inf;  // lane p: the current k-th of pair p
        for (uint32_t b = it.b_lo + wave; b < it.b_hi; b += kWaves) {
            const uint64_t gb = base + b;
            const unsigned long long allow = rd_lane((uint64_t)a.allow[gb], 0);
            if (allow == 0) continue;  // (wave-uniform) no shadow byte of this block is read
            wave_sync();               // (the previous block's tile is read)
            sbound::block_bounds<M, I8>(src, qa_row, pr, gb, lane, [&](int vt, int r, float approx, float del) {
                const uint32_t v = 16 * vt + (lane & 15);
                const float ub = approx + del;
                const bool counts = b * 64 + v < cnt && ((allow >> v) & 1ull) && ub == ub;
                s_tile[wave][4 * (lane >> 4) + r][v] = counts ? ub : inf;
            });
            wave_sync();
            for (int p = 0; p < np; ++p) {  // (rows at or above np repeat the last pair: dropped)
                const float v = s_tile[wave][p][lane];
                float kd = rd_lane(kdv, p);
                const bool want = v < kd;
                unsigned long long m = __ballot(want);
                if (!m) continue;  // (wave-uniform)
                float d = s_list[wave][p][lane];
                if (__popcll(m) > 6) {
                    float bd = want ? v : inf;
                    sort64_f(bd);
                    merge64_f(d, bd);
                } else {
                    while (m) {
                        const int l = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float c = rd_lane(v, l);
                        if (c < kd) {
                            insert_f(d, c);
                            kd = rd_lane(d, k - 1);
                        }
                    }
                }
                s_list[wave][p][lane] = d;
                kd = rd_lane(d, k - 1);
                if (lane == p) kdv = kd;
            }
        }
        __syncthreads();
        for (int p = (int)wave; p < np; p += (int)kWaves) {  // one wave merges the four waves' lists of a pair
            float d = s_list[0][p][lane];
            for (uint32_t w = 1; w < kWaves; ++w) merge64_f(d, s_list[w][p][lane]);
            const uint32_t pair = a.inv[it.p0 + (uint32_t)p];
            if (a.segs > 1) {
                if (lane < k) a.part[((size_t)pair * a.segs + it.seg) * k + lane] = d;
            } else if (lane == k - 1) {
                a.tau[pair] = d;
            }
        }
        __syncthreads();  // (the lists are read before the next item's are written)
    }
}

// segs > 1: per pair the k-th smallest of its segments' partials.
__global__ __launch_bounds__(kWaves * 64) void ivf_filter_screen_tau(const float* __restrict__ part,
                                                                      const uint32_t* __restrict__ probes,
                                                                      const uint32_t* __restrict__ allowed,
                                                                      const uint32_t* __restrict__ count, uint32_t BP,
                                                                      uint32_t segs, uint32_t k, float* __restrict__ tau) {
    const uint32_t i = blockIdx.x * kWaves + wave_index();
    if (i >= BP) return;
    const uint32_t list = probes[i];
    if (allowed[list] == 0) return;  // (no item, no partial)
    const int lane = lane_id();
    const uint32_t n = scan_segs((count[list] + 63) >> 6, segs) * k;  // the list's segments are the pair's first
    const size_t base = (size_t)i * segs * k;
    float d = __builtin_inff();
    for (uint32_t e0 = 0; e0 < n; e0 += 64) {
        const uint32_t e = e0 + lane;
        float v = e < n ? part[base + e] : __builtin_inff();
        sort64_f(v);
        merge64_f(d, v);
    }
    if ((uint32_t)lane == k - 1) tau[i] = d;
}

template <int M, bool I8>
__global__ __launch_bounds__(kWaves * 64, 2) void ivf_filter_screen_bound(const FilterScreenArgs a) {
    __shared__ uint32_t s_item;
    if (bad_shape(a, I8)) {
        if (threadIdx.x == 0) atomicOr(a.ctrl + kFsStatus, kRangeUnserved);
        return;
    }
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const sbound::BoundSrc src = bound_src(a);
    const uint32_t total = a.item_start[a.nlist];
    for (;;) {
        const uint32_t item = next_item(a.ctrl, kFsNextB, &s_item);
        if (item >= total) break;
        const ExactScanItem it =
            decode_scan_item<kFilterScreenGroup>(item, a.item_start, a.pair_start, a.count, a.nlist, a.segs);
        const int np = (int)it.np;
        if (np < 1 || np > G) {
            if (threadIdx.x == 0) atomicOr(a.ctrl + kFsStatus, kRangeUnserved);
            continue;
        }
        const uint32_t cnt = a.count[it.list];
        const uint64_t base = a.block_off[it.list];
        if (it.seg == 0 && threadIdx.x == 0)
            atomicAdd(a.ctrl + kFsPairs, (unsigned long long)np * a.allowed[it.list]);
        const uint4* qa_row = sbound::a_row<I8>(a.qres, a.inv, it.p0, np, a.dp, lane);
        uint32_t pr[4];
        float tau[4];  // the pairs' thresholds, fixed before this launch
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pr[r] = a.inv[it.p0 + (uint32_t)min(4 * (lane >> 4) + r, np - 1)];
            tau[r] = a.tau[pr[r]];
        }
        for (uint32_t b = it.b_lo + wave; b < it.b_hi; b += kWaves) {
            const uint64_t gb = base + b;
            const unsigned long long allow = rd_lane((uint64_t)a.allow[gb], 0);
            if (allow == 0) continue;  // (wave-uniform) no shadow byte of this block is read
            // bit 4 vt + r: (slot 16 vt + (lane & 15), pair row 4 (lane >> 4) + r) is a candidate
            uint32_t keep = 0;
            sbound::block_bounds<M, I8>(src, qa_row, pr, gb, lane, [&](int vt, int r, float approx, float del) {
                const uint32_t v = 16 * vt + (lane & 15);
                const float lb = approx - del;
                const bool c = b * 64 + v < cnt && 4 * (lane >> 4) + r < np && ((allow >> v) & 1ull) && !(lb > tau[r]);
                keep |= (uint32_t)c << (4 * vt + r);
            });
            uint32_t tot = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) tot += (uint32_t)__popcll(__ballot((keep >> e) & 1u));
            if (tot) {  // (wave-uniform)
                unsigned long long at = 0;
                if (lane == 0) at = atomicAdd(a.ctrl + kFsCursor, (unsigned long long)tot);
                at = rd_lane((uint64_t)at, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const bool c = (keep >> e) & 1u;
                    const unsigned long long mm = __ballot(c);
                    const unsigned long long idx =
                        at + __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
                    if (c && idx < a.cand_cap)
                        a.cand[idx] = ((uint64_t)pr[e & 3] << 32) | (uint32_t)(gb * 64 + 16 * (e >> 2) + (lane & 15));
                    at += (unsigned long long)__popcll(mm);
                }
            }
        }
    }
}

constexpr int kC4 = (int)kRangeChunk4;
// one tile per wave: 64 rows x kC4 float4, a row padded by one float4 (as ivf_range_recheck's)
typedef float4 SelectTile[64][kC4 + 1];

// The first candidate at or above `key`.
__device__ __forceinline__ uint64_t cand_lower(const uint64_t* __restrict__ c, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (c[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int M>
__global__ __launch_bounds__(kWaves * 64) void ivf_filter_screen_select(const FilterSelectArgs a) {
    constexpr int C4 = kC4;
    __shared__ SelectTile s_x[kWaves];
    const uint32_t d4 = a.d4;
    if (d4 == 0 || d4 % C4 != 0 || a.k < 1 || a.k > kFilterScreenMaxK) {  // (the host guard refuses this first)
        if (threadIdx.x == 0) atomicOr(a.ctrl + kFsStatus, kRangeUnserved);
        return;
    }
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const uint32_t pair = blockIdx.x * kWaves + wave;  // (wave-uniform)
    if (pair >= a.BP) return;
    // nothing is written for a pair without an allowed row, as the scan writes nothing
    if ((a.gate ? a.gate[pair] : a.allowed[a.probes[pair]]) == 0) return;
    float4(*tile)[C4 + 1] = s_x[wave];
    const int k = (int)a.k;
    const uint64_t lo = cand_lower(a.cand, a.n, (uint64_t)pair << 32);
    const uint64_t hi = cand_lower(a.cand, a.n, ((uint64_t)pair + 1) << 32);
    const float4* __restrict__ q4 = (const float4*)(a.q + (size_t)(pair / a.P) * d4 * 4);  // (wave-uniform reads)
    WaveTopK<1> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    for (uint64_t c0 = lo; c0 < hi; c0 += 64) {
        const uint32_t live = (uint32_t)min((uint64_t)64, hi - c0);  // >= 1
        const bool act = (uint32_t)lane < live;
        const uint32_t slot = (uint32_t)a.cand[c0 + (act ? (uint32_t)lane : live - 1)];  // (a lane past the end repeats the last)
        // lane l fetches float4 (l & 7) of the rows of candidates (l >> 3) + 8 i
        const float4* src[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t sl = (uint32_t)__shfl((int)slot, (lane >> 3) + 8 * i);
            src[i] = a.rows + (uint64_t)sl * d4 + (lane & 7);
        }
        float4 nx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) nx[i] = load_nt(src[i]);
        float acc = 0.0f;
        for (uint32_t c = 0; c < d4; c += C4) {
            wave_sync();  // (the previous chunk's reads are done)
#pragma unroll
            for (int i = 0; i < 8; ++i) tile[i * 8 + (lane >> 3)][lane & 7] = nx[i];
            if (c + C4 < d4) {  // the rows' next chunk, never beyond a row
#pragma unroll
                for (int i = 0; i < 8; ++i) nx[i] = load_nt(src[i] + c + C4);
            }
            wave_sync();
#pragma unroll
            for (int t = 0; t < C4; ++t) acc = acc4<M>(acc, q4[c + t], tile[lane][t]);
        }
        const float dv = dist_finish<M>(acc);
        const uint64_t id = act ? a.ids[slot] : kNoId;
        offer_lanes<1>(tk, act && dv <= kd, dv, id, k, kd, ki);
    }
    if (lane < k) {
        a.slot_d[(size_t)pair * k + lane] = tk.d[0];
        a.slot_i[(size_t)pair * k + lane] = tk.id[0];
    }
}

// persistent over the items (their number is known on the device only): the workgroups the
// whole chip holds at once
uint32_t item_grid(const FilterScreenArgs& a) {
    return (uint32_t)std::min<uint64_t>((uint64_t)a.B * a.P * a.segs, 256 * 2);
}

template <int M>
void thresh_metric(const FilterScreenArgs& a, hipStream_t s) {
    if (a.sscale) ivf_filter_screen_thresh<M, true><<<item_grid(a), kWaves * 64, 0, s>>>(a);
    else ivf_filter_screen_thresh<M, false><<<item_grid(a), kWaves * 64, 0, s>>>(a);
    if (a.segs > 1) {
        const uint32_t BP = a.B * a.P;
        ivf_filter_screen_tau<<<(BP + kWaves - 1) / kWaves, kWaves * 64, 0, s>>>(a.part, a.probes, a.allowed,
                                                                               a.count, BP, a.segs, a.k, a.tau);
    }
}

template <int M>
void bound_metric(const FilterScreenArgs& a, hipStream_t s) {
    if (a.sscale) ivf_filter_screen_bound<M, true><<<item_grid(a), kWaves * 64, 0, s>>>(a);
    else ivf_filter_screen_bound<M, false><<<item_grid(a), kWaves * 64, 0, s>>>(a);
}

}  // namespace

void launch_filter_screen_thresh(int metric, const FilterScreenArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) thresh_metric<kL2>(a, s);
    else thresh_metric<kIP>(a, s);
}

void launch_filter_screen_bound(int metric, const FilterScreenArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) bound_metric<kL2>(a, s);
    else bound_metric<kIP>(a, s);
}

void launch_filter_screen_select(int metric, const FilterSelectArgs& a, hipStream_t s) {
    if (!a.BP) return;
    const uint32_t grid = (a.BP + kWaves - 1) / kWaves;
    if (metric == kL2) ivf_filter_screen_select<kL2><<<grid, kWaves * 64, 0, s>>>(a);
    else ivf_filter_screen_select<kIP><<<grid, kWaves * 64, 0, s>>>(a);
}

}  // namespace vdbk
