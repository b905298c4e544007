// multi_filter_screen_kernels.hip — device side of vdb_ivf_search_prepared_multi_screened
// (gfx950, wave64): the two shadow passes of filter_screen_kernels.hip for a batch whose queries
// each name their own prepared filter.
//
// The items are those of the pair grouping gated per pair (launch_scan_group_pairs, a group of
// 16): one segment of one list against up to 16 pairs, the 16 rows of one MFMA A operand, and
// now up to 16 different mask rows. The stream through the matrix cores, the LDS transpose tile,
// the per-pair sorted k-lists, the cross-wave merge, `part` and the candidate append are
// ivf_filter_screen_thresh's and ivf_filter_screen_bound's. What is new is how the mask moves:
//   per item   lane p < 16 resolves the mask row of pair min(p, np - 1) once:
//              allow_tab[qf[inv[p0 + p] / P]] + block_off[list];
//   per block  lanes 0..15 load their pair's 8-byte word of block b, one iteration ahead of its
//              use, so the (up to 16) scattered loads wait under the current block's MFMA
//              stream; no word is loaded outside the item's [b_lo, b_hi);
//   the union  of the sixteen words (four DPP steps inside the row, on two dwords) is
//              wave-uniform and decides what is read: a block whose union is zero costs no
//              shadow byte;
//   the own    word decides what counts: the lane that emits rows 4 (lane >> 4) + r fetches those
//              four pairs' words from the holding lanes (four 64-bit shuffles), and slot v counts
//              for row r only if bit v of that row's own word is set. A row that a neighbour's
//              filter allows and the pair's own does not never reaches a k-list or the
//              candidate buffer.
//   ivf_filter_screen_tau_gated   ivf_filter_screen_tau with gate[pair] for allowed[list].
// No kernel reads a shadow byte, a mask word or a meta entry beyond the item's own blocks.
#pragma clang fp contract(off)
#include "multi_filter_screen_kernels.hpp"

#include <algorithm>

#include "scan_common.hpp"
#include "screen_bound.hpp"
#include "screen_klist.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup
constexpr int G = (int)kFilterScreenGroup;

__device__ __forceinline__ sbound::BoundSrc bound_src(const MultiFilterScreenArgs& a) {
    return sbound::BoundSrc{a.shadow, a.meta, a.sscale, a.pst, a.qscale, a.dp};
}

__device__ __forceinline__ bool bad_shape(const MultiFilterScreenArgs& a, bool i8) {
    return a.dp == 0 || a.dp % (i8 ? 64u : 32u) != 0 || a.k < 1 || a.k > kFilterScreenMaxK;
}

// The mask words of an item's pairs for the blocks one wave takes, b_lo + wave, + kWaves, ...
struct MaskStream {
    const unsigned long long* row;  // lane l: the masks of pair min(l & 15, np - 1) over this list's blocks
    unsigned long long ahead;       // lanes 0..15: the word of the wave's next block; 0 in the other lanes
    uint32_t b_hi;

    __device__ __forceinline__ unsigned long long load(uint32_t b, int lane) const {
        return b < b_hi && lane < G ? row[b] : 0ull;  // (never outside the item's blocks)
    }
    __device__ __forceinline__ void open(const MultiFilterScreenArgs& a, const ExactScanItem& it, uint32_t b, int lane) {
        const uint32_t pair = a.inv[it.p0 + (uint32_t)min(lane & 15, (int)it.np - 1)];
        row = a.allow_tab[a.qf[pair / a.P]] + a.block_off[it.list];
        b_hi = it.b_hi;
        ahead = load(b, lane);
    }
    // Block b's words (lanes 0..15; requested an iteration ago) and their union, wave-uniform;
    // the words of block b + kWaves are requested.
    __device__ __forceinline__ unsigned long long take(uint32_t b, int lane, unsigned long long& word) {
        word = ahead;
        ahead = load(b + kWaves, lane);
        unsigned long long u = word;
        u |= xor_u64<8>(u);
        u |= xor_u64<4>(u);
        u |= xor_u64<2>(u);
        u |= xor_u64<1>(u);
        return rd_lane((uint64_t)u, 0);
    }
    // The words of this lane's four rows 4 (lane >> 4) + r, from the lanes that hold them.
    __device__ __forceinline__ static void own(unsigned long long word, int lane, unsigned long long (&w)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = shfl_u64(word, 4 * (lane >> 4) + r);
    }
};

template <int M, bool I8>
__global__ __launch_bounds__(kWaves * 64, 2) void ivf_filter_screen_thresh_multi(const MultiFilterScreenArgs a) {
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
        MaskStream ms;
        ms.open(a, it, it.b_lo + wave, lane);
        for (uint32_t b = it.b_lo + wave; b < it.b_hi; b += kWaves) {
            unsigned long long word;
            if (ms.take(b, lane, word) == 0) continue;  // (wave-uniform) no shadow byte of this block is read
            unsigned long long mw[4];
            MaskStream::own(word, lane, mw);
            const uint64_t gb = base + b;
            wave_sync();  // (the previous block's tile is read)
            sbound::block_bounds<M, I8>(src, qa_row, pr, gb, lane, [&](int vt, int r, float approx, float del) {
                const uint32_t v = 16 * vt + (lane & 15);
                const float ub = approx + del;
                const bool counts = b * 64 + v < cnt && ((mw[r] >> v) & 1ull) && ub == ub;
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

// segs > 1: per gated pair the k-th smallest of its segments' partials.
__global__ __launch_bounds__(kWaves * 64) void ivf_filter_screen_tau_gated(const float* __restrict__ part,
                                                                            const uint32_t* __restrict__ probes,
                                                                            const uint32_t* __restrict__ gate,
                                                                            const uint32_t* __restrict__ count,
                                                                            uint32_t BP, uint32_t segs, uint32_t k,
                                                                            float* __restrict__ tau) {
    const uint32_t i = blockIdx.x * kWaves + wave_index();
    if (i >= BP) return;
    if (gate[i] == 0) return;  // (no item, no partial)
    const int lane = lane_id();
    const uint32_t n = scan_segs((count[probes[i]] + 63) >> 6, segs) * k;  // the list's segments are the pair's first
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
__global__ __launch_bounds__(kWaves * 64, 2) void ivf_filter_screen_bound_multi(const MultiFilterScreenArgs a) {
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
        // the rows the pairs' own filters allow in the list, once per pair
        if (it.seg == 0 && wave == 0 && lane < np)
            atomicAdd(a.ctrl + kFsPairs, (unsigned long long)a.gate[a.inv[it.p0 + (uint32_t)lane]]);
        const uint4* qa_row = sbound::a_row<I8>(a.qres, a.inv, it.p0, np, a.dp, lane);
        uint32_t pr[4];
        float tau[4];  // the pairs' thresholds, fixed before this launch
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pr[r] = a.inv[it.p0 + (uint32_t)min(4 * (lane >> 4) + r, np - 1)];
            tau[r] = a.tau[pr[r]];
        }
        MaskStream ms;
        ms.open(a, it, it.b_lo + wave, lane);
        for (uint32_t b = it.b_lo + wave; b < it.b_hi; b += kWaves) {
            unsigned long long word;
            if (ms.take(b, lane, word) == 0) continue;  // (wave-uniform) no shadow byte of this block is read
            unsigned long long mw[4];
            MaskStream::own(word, lane, mw);
            const uint64_t gb = base + b;
            // bit 4 vt + r: (slot 16 vt + (lane & 15), pair row 4 (lane >> 4) + r) is a candidate
            uint32_t keep = 0;
            sbound::block_bounds<M, I8>(src, qa_row, pr, gb, lane, [&](int vt, int r, float approx, float del) {
                const uint32_t v = 16 * vt + (lane & 15);
                const float lb = approx - del;
                const bool c = b * 64 + v < cnt && 4 * (lane >> 4) + r < np && ((mw[r] >> v) & 1ull) && !(lb > tau[r]);
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

// persistent over the items (their number is known on the device only): the workgroups the
// whole chip holds at once
uint32_t item_grid(const MultiFilterScreenArgs& a) {
    return (uint32_t)std::min<uint64_t>((uint64_t)a.B * a.P * a.segs, 256 * 2);
}

template <int M>
void thresh_metric(const MultiFilterScreenArgs& a, hipStream_t s) {
    if (a.sscale) ivf_filter_screen_thresh_multi<M, true><<<item_grid(a), kWaves * 64, 0, s>>>(a);
    else ivf_filter_screen_thresh_multi<M, false><<<item_grid(a), kWaves * 64, 0, s>>>(a);
    if (a.segs > 1) {
        const uint32_t BP = a.B * a.P;
        ivf_filter_screen_tau_gated<<<(BP + kWaves - 1) / kWaves, kWaves * 64, 0, s>>>(a.part, a.probes, a.gate, a.count,
                                                                                     BP, a.segs, a.k, a.tau);
    }
}

template <int M>
void bound_metric(const MultiFilterScreenArgs& a, hipStream_t s) {
    if (a.sscale) ivf_filter_screen_bound_multi<M, true><<<item_grid(a), kWaves * 64, 0, s>>>(a);
    else ivf_filter_screen_bound_multi<M, false><<<item_grid(a), kWaves * 64, 0, s>>>(a);
}

}  // namespace

void launch_filter_screen_thresh_multi(int metric, const MultiFilterScreenArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) thresh_metric<kL2>(a, s);
    else thresh_metric<kIP>(a, s);
}

void launch_filter_screen_bound_multi(int metric, const MultiFilterScreenArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) bound_metric<kL2>(a, s);
    else bound_metric<kIP>(a, s);
}

}  // namespace vdbk
