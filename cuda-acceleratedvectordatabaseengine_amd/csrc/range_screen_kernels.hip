// range_screen_kernels.hip — device side of vdb_ivf_range_search_screened (gfx950, wave64).
//
//   ivf_range_screen   persistent workgroups of 4 waves over the items of the pair grouping
//                      (scan_items.hip with a group of 16, decoded by scan_items.hpp): one
//                      segment of one list against up to 16 of the pairs that probe it, the
//                      16 rows of one MFMA A operand. A workgroup takes its next item from one
//                      device counter; its waves take the segment's blocks in turn. Per block a
//                      wave streams the block's shadow (the B operands as ivf_screen_build(_i8)
//                      laid them out: per k-step four 1 KiB vector tiles, non-temporal 16-byte
//                      loads, kDepth k-steps in flight) through v_mfma_i32_16x16x64_i8 or
//                      v_mfma_f32_16x16x32_bf16 against the pairs' A rows (launch_screen_pairs),
//                      and turns each of the 16 x 64 dot products into the screened search's
//                      lower bound lb = approx - del: the operations of collect_segment
//                      (screen.hip) in its order, contraction off, so the two agree bit for bit.
//                      The threshold is the call's radius, known before the scan and never
//                      moved: no top-k, no upper bounds, no state shared between blocks. A (pair,
//                      slot) is a candidate unless lb > radius (so a NaN or -inf bound, which is
//                      what a huge or non-finite row, query or centroid gives, is a candidate);
//                      the block's candidates are appended wave-aggregated (sixteen ballots, one
//                      atomic add of their popcounts by one lane, the base broadcast) as {query,
//                      slot}. Past the buffer's capacity nothing is written and the cursor keeps
//                      counting. With a prepared filter's masks a block whose mask is zero is
//                      skipped unread and a candidate needs its slot's bit.
//                      Nothing is asked for ahead of a block: the loads in flight are k-steps of
//                      the block in hand, so no byte beyond the item's own blocks is read and the
//                      shadow's slack blocks are never touched. The kernel has no LDS array sized
//                      by the item width (the item's norms and scales are read where they are
//                      used); an item wider than the A operand is refused all the same.
//   ivf_range_recheck  one wave per 64 candidates, lane i owning candidate i: the exact distance
//                      (the reference's sequential fp32 sum, acc4 / dist_finish) of its row of
//                      the row-major copy against its query. The rows are staged as
//                      ivf_range_scan stages a block's: eight lanes read one row's 128-byte run
//                      into the wave's LDS tile (kRangeChunk4 float4 of each of the 64 rows, the
//                      next chunk in flight while the current one is summed), then lane i reads
//                      row i back, so each row's sum stays in sequence order. The queries differ
//                      per lane and are read where they are used (a batch's queries stay in the
//                      caches). A hit (d <= radius) is appended exactly as ivf_range_scan
//                      appends one, the id read for hit lanes only.
#pragma clang fp contract(off)
#include "range_screen_kernels.hpp"

#include <algorithm>

#include "scan_common.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup
// k-steps of a block's shadow in flight per wave (4 KiB each). 2 keeps every instantiation at
// two workgroups per CU without scratch; with 4 the inner-product ones spill.
constexpr int kDepth = 2;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 ld_nt_u4(const uint4* p) {
    const u32x4 v = __builtin_nontemporal_load((const u32x4*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ bf16x8 as_bf16x8(const uint4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ i32x4 as_i32x4(const uint4 v) { return __builtin_bit_cast(i32x4, v); }

// (as in range_kernels.hip)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Blocks b_lo + wave, + kWaves, ... < b_hi of the list at arena block `base` (cnt rows) against
// the np <= 16 pairs inv[p0 ..).
template <int M, bool I8, bool MASKED>
__device__ __forceinline__ void range_screen_blocks(const RangeScreenArgs& a, uint32_t p0, int np, uint32_t b_lo,
                                                    uint32_t b_hi, uint64_t base, uint32_t cnt) {
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const uint32_t dp = a.dp, ks = dp >> (I8 ? 6 : 5);  // (k-steps of 64 int8 or 32 bf16 dims)
    // the bound's rounding coefficients (collect_segment's)
    const float cm = (float)(4 * dp + 16) * 0x1.02p-24f;
    const float cr = (float)(dp + 2) * 0x1.02p-24f;
    const float cu = 0x1.02p-23f;
    // the MFMA A row of this lane: pair (lane & 15) of the item (rows at or above np repeat the
    // last pair and are dropped), its 16 bytes (lane >> 4) of each k-step's 64
    const uint32_t pa = a.inv[p0 + (uint32_t)min(lane & 15, np - 1)];
    const uint4* qa_row = (const uint4*)((const char*)a.qres + (size_t)pa * dp * (I8 ? 1 : 2)) + (lane >> 4);
    // the D rows of this lane: pairs 4 (lane >> 4) + r of the item
    uint32_t pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pr[r] = a.inv[p0 + (uint32_t)min(4 * (lane >> 4) + r, np - 1)];
    using AccT = std::conditional_t<I8, i32x4, f32x4>;

    for (uint32_t b = b_lo + wave; b < b_hi; b += kWaves) {
        const uint64_t gb = base + b;
        unsigned long long allow = ~0ull;
        if constexpr (MASKED) {
            const unsigned long long m = a.allow[gb];
            allow = rd_lane((uint64_t)m, 0);
            if (allow == 0) continue;  // (wave-uniform) no shadow byte of this block is read
        }
        // the block's k-steps through the matrix cores, kDepth of them in flight, none beyond the block
        const uint4* sp = a.shadow + gb * (uint64_t)ks * 256 + lane;
        uint4 xa[kDepth][4], qa[kDepth];
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            if ((uint32_t)u < ks) {  // (wave-uniform)
#pragma unroll
                for (int vt = 0; vt < 4; ++vt) xa[u][vt] = ld_nt_u4(sp + (size_t)(u * 4 + vt) * 64);
                qa[u] = qa_row[4 * u];
            }
        }
        AccT acc[4];
#pragma unroll
        for (int vt = 0; vt < 4; ++vt) acc[vt] = AccT{0, 0, 0, 0};
        for (uint32_t s0 = 0; s0 < ks; s0 += kDepth) {
            static_for<0, kDepth>([&](auto uu) {
                constexpr int u = decltype(uu)::value;
                if (s0 + u < ks) {  // (wave-uniform)
                    if constexpr (I8) {
                        const i32x4 A = as_i32x4(qa[u]);
#pragma unroll
                        for (int vt = 0; vt < 4; ++vt)
                            acc[vt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, as_i32x4(xa[u][vt]), acc[vt], 0, 0, 0);
                    } else {
                        const bf16x8 A = as_bf16x8(qa[u]);
#pragma unroll
                        for (int vt = 0; vt < 4; ++vt)
                            acc[vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, as_bf16x8(xa[u][vt]), acc[vt], 0, 0, 0);
                    }
                    const uint32_t nxt = s0 + u + kDepth;
                    if (nxt < ks) {
#pragma unroll
                        for (int vt = 0; vt < 4; ++vt) xa[u][vt] = ld_nt_u4(sp + ((size_t)nxt * 4 + vt) * 64);
                        qa[u] = qa_row[4 * nxt];
                    }
                }
            });
        }
        // the lower bounds of the block's 64 x 16 pairs, in place of the dot products
        float4 pst[4];
        float qsc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pst[r] = a.pst[pr[r]];
            qsc[r] = 0.0f;
            if constexpr (I8) qsc[r] = a.qscale[pr[r]];
        }
        float lb[4][4];
#pragma unroll
        for (int vt = 0; vt < 4; ++vt) {
            const uint64_t mslot = gb * 64 + 16 * vt + (lane & 15);
            const float4 mt = a.meta[mslot];
            float vsc = 0.0f;
            if constexpr (I8) vsc = a.sscale[mslot];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float dot;
                if constexpr (I8) dot = (float)acc[vt][r] * (qsc[r] * vsc);
                else dot = acc[vt][r];
                const float4 ps = pst[r];
                const float approx = M == kL2 ? (ps.x + mt.x) - 2.0f * dot : -(ps.x + dot);
                const float an = ps.y + ps.z, bn = mt.y + mt.z;
                const float cs = an * mt.z + ps.z * bn + ps.z * mt.z;
                float del;
                if (M == kL2) {
                    const float rest = 2.0f * (cs + cm * (an * bn)) + cu * (ps.x + mt.x + fabsf(approx));
                    del = rest + cr * (fabsf(approx) + rest);
                } else {
                    del = cs + cm * (an * bn) + cr * (ps.y * mt.w) + cu * (ps.y * ps.w + an * bn + fabsf(approx));
                }
                del = del * 1.001f + 1e-30f;
                lb[vt][r] = approx - del;
            }
        }
        // candidates: slot below the list's count, pair of the item, allowed, and not above the radius
        auto is_cand = [&](int vt, int r) {
            const uint32_t v = 16 * vt + (lane & 15);
            bool c = b * 64 + v < cnt && 4 * (lane >> 4) + r < np && !(lb[vt][r] > a.radius);
            if constexpr (MASKED) c = c && ((allow >> v) & 1ull);
            return c;
        };
        uint32_t tot = 0;
#pragma unroll
        for (int vt = 0; vt < 4; ++vt)
#pragma unroll
            for (int r = 0; r < 4; ++r) tot += (uint32_t)__popcll(__ballot(is_cand(vt, r)));
        if (tot) {  // (wave-uniform)
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(a.ctrl + kRsCursor, (unsigned long long)tot);
            at = rd_lane((uint64_t)at, 0);
#pragma unroll
            for (int vt = 0; vt < 4; ++vt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool c = is_cand(vt, r);
                    const unsigned long long mm = __ballot(c);
                    const unsigned long long idx =
                        at + __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
                    if (c && idx < a.cand_cap)
                        a.cand[idx] = make_uint2(pr[r] / a.P, (uint32_t)(gb * 64 + 16 * vt + (lane & 15)));
                    at += (unsigned long long)__popcll(mm);
                }
            }
        }
    }
}

template <int M, bool I8, bool MASKED>
__global__ __launch_bounds__(kWaves * 64, 2) void ivf_range_screen(const RangeScreenArgs a) {
    if (a.dp == 0 || a.dp % (I8 ? 64u : 32u) != 0) {  // (the host guard refuses this first: range_screen_serves_shape)
        if (threadIdx.x == 0) atomicOr(a.ctrl + kRsStatus, kRangeUnserved);
        return;
    }
    const uint32_t total = a.item_start[a.nlist];
    __shared__ uint32_t s_item;
    for (;;) {
        if (threadIdx.x == 0) s_item = (uint32_t)atomicAdd(a.ctrl + kRsNext, 1ull);
        __syncthreads();
        const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_item);  // (the same in every wave)
        __syncthreads();               // (read by all before thread 0 writes the next)
        if (item >= total) break;
        const ExactScanItem it =
            decode_scan_item<kRangeScreenGroup>(item, a.item_start, a.pair_start, a.count, a.nlist, a.segs);
        const int np = (int)it.np;
        if (np < 1 || np > (int)kRangeScreenGroup) {  // (never decoded: an item is one A operand at most)
            if (threadIdx.x == 0) atomicOr(a.ctrl + kRsStatus, kRangeUnserved);
            continue;
        }
        const uint32_t cnt = a.count[it.list];
        const uint64_t base = a.block_off[it.list];
        if (it.seg == 0 && threadIdx.x == 0)
            atomicAdd(a.ctrl + kRsPairs, (unsigned long long)np * (MASKED ? a.allowed[it.list] : cnt));
        range_screen_blocks<M, I8, MASKED>(a, it.p0, np, it.b_lo, it.b_hi, base, cnt);
    }
}

constexpr int kC4 = (int)kRangeChunk4;
// one tile per wave: 64 rows x kC4 float4, a row padded by one float4 (as ivf_range_scan's)
typedef float4 RecheckTile[64][kC4 + 1];

template <int M>
__global__ __launch_bounds__(kWaves * 64) void ivf_range_recheck(const RangeRecheckArgs a) {
    constexpr int C4 = kC4;
    __shared__ RecheckTile s_x[kWaves];
    const uint32_t d4 = a.d4;
    if (d4 == 0 || d4 % C4 != 0) {  // (the host guard refuses this first: range_recheck_serves)
        if (threadIdx.x == 0) atomicOr(a.ctrl + kRangeStatus, kRangeUnserved);
        return;
    }
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    float4(*tile)[C4 + 1] = s_x[wave];
    const uint64_t rounds = (a.n + 63) / 64;
    for (uint64_t rd = (uint64_t)blockIdx.x * kWaves + wave; rd < rounds; rd += (uint64_t)gridDim.x * kWaves) {
        const uint64_t c0 = rd * 64;
        const uint32_t live = (uint32_t)min((uint64_t)64, a.n - c0);  // >= 1
        const bool act = (uint32_t)lane < live;
        const uint2 ent = a.cand[c0 + (act ? (uint32_t)lane : live - 1)];  // (a lane past the end repeats the last candidate)
        const uint32_t qi = ent.x, slot = ent.y;
        const float4* __restrict__ q4 = (const float4*)(a.q + (size_t)qi * d4 * 4);
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
        const bool hit = act && dv <= a.radius;  // (false for a NaN distance)
        const unsigned long long m = __ballot(hit);
        if (m) {  // (wave-uniform)
            uint64_t id = 0;
            if (hit) id = a.ids[slot];
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(a.ctrl + kRangeCursor, (unsigned long long)__popcll(m));
            at = rd_lane((uint64_t)at, 0);
            at += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (hit && at < a.cap) {
                a.hit_key[at] = ((uint64_t)qi << 32) | ord_enc(dv);
                a.hit_id[at] = id;
            }
        }
    }
}

template <int M>
void screen_metric(const RangeScreenArgs& a, hipStream_t s) {
    // persistent over the items (their number is known on the device only): the workgroups the
    // whole chip holds at once
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)a.B * a.P * a.segs, 256 * 8);
    if (a.sscale) {
        if (a.allow) ivf_range_screen<M, true, true><<<grid, kWaves * 64, 0, s>>>(a);
        else ivf_range_screen<M, true, false><<<grid, kWaves * 64, 0, s>>>(a);
    } else {
        if (a.allow) ivf_range_screen<M, false, true><<<grid, kWaves * 64, 0, s>>>(a);
        else ivf_range_screen<M, false, false><<<grid, kWaves * 64, 0, s>>>(a);
    }
}

}  // namespace

void launch_range_screen(int metric, const RangeScreenArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) screen_metric<kL2>(a, s);
    else screen_metric<kIP>(a, s);
}

void launch_range_recheck(int metric, const RangeRecheckArgs& a, hipStream_t s) {
    if (!a.n) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((a.n + 64 * kWaves - 1) / (64 * kWaves), 256 * 4);
    if (metric == kL2) ivf_range_recheck<kL2><<<grid, kWaves * 64, 0, s>>>(a);
    else ivf_range_recheck<kIP><<<grid, kWaves * 64, 0, s>>>(a);
}

}  // namespace vdbk
