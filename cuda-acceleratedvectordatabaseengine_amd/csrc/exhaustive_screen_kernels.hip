// exhaustive_screen_kernels.hip — device side of vdb_ivf_search_exhaustive_screened (gfx950,
// wave64): the exact unique-id top-k over every stored row, from two passes over the screen's
// shadow and one over the few rows the bounds cannot discard.
//
// The two shadow kernels share one stream. The arena is one run of 64-row blocks; a persistent
// grid walks it in storage order across list boundaries, a wave taking `chunk` consecutive blocks
// at a time from an atomic cursor (as ivf_exhaustive_scan does). Per block the wave
//   * reads the block's stored-row count (ivf_exh_valid_*: pad and stale slots are never offered;
//     a block no list owns is skipped unread) and its list (screen_blist);
//   * points two MFMA A operands at that list's pairs of the tile (pair g * nlist + list, queries
//     0..15 and 16..31; rows at or above nq repeat the last query and are dropped), read from
//     qres through L2; a tile of 16 or fewer queries runs one operand;
//   * loads each k-step of the block's shadow once, non-temporally (4 x 1 KiB), two k-steps in
//     flight and none beyond the block, and feeds it to both operands: 8 x
//     v_mfma_i32_16x16x64_i8 or 8 x v_mfma_f32_16x16x32_bf16 per k-step;
//   * turns the 32 x 64 dot products into `approx` and `del`, screen_bound.hpp's formulas term
//     for term (a two-operand copy of sbound::block_bounds: the B registers are shared);
//   * turns the MFMA D layout through its LDS tile [query][slot] so that lane i holds slot i.
//
//   ivf_exh_screen_thresh  ub = approx + del. Per (wave, query) a unique-id list of the 64
//                      smallest (ub, id) in LDS (WaveTopK<1>::offer_unique). A row's id is read
//                      only where its ub is below the gate: the smaller of the list's own k-th and
//                      the tile's shared threshold of that query, to which a wave publishes its
//                      k-th (ord_enc, atomicMin) once its list holds k distinct ids. NaN and
//                      infinite ub are never offered. At the end the four wave lists fold to one
//                      unique partial per (workgroup, query); ivf_exhaustive_merge folds the
//                      grid's, and T_q is the ub of its k-th entry (FLT_MAX with fewer than k).
//   ivf_exh_screen_bound   lb = approx - del. Every valid (query, row) with !(lb > T_q) is
//                      appended as its 32-bit slot to the query's region of the candidate buffer:
//                      per (wave, query, block) one ballot, one mbcnt compaction, one atomicAdd
//                      by one lane, plain vector stores. Past the region nothing is written and
//                      the count goes on.
//   ivf_exh_screen_select  one workgroup per query; a lane takes a candidate and sums its own row
//                      from screen_rows in dimension order from +0.0f (dist_term, dist_finish, no
//                      FMA: the reference's bits); (d, id) through offer_unique; the four waves
//                      fold; unfilled entries (FLT_MAX, UINT64_MAX).
// No kernel reads a shadow byte, a norm, an id or a row beyond the arena's blocks or the
// candidates' own slots.
#pragma clang fp contract(off)
#include "exhaustive_screen_kernels.hpp"

#include <cfloat>
#include <stdexcept>
#include <type_traits>

#include "scan_common.hpp"
#include "screen_bound.hpp"
#include "screen_klist.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace {

constexpr int TQ = (int)kExsTile;
constexpr int kDepth = sbound::kDepth;
using sbound::as_bf16x8;
using sbound::as_i32x4;
using sbound::f32x4;
using sbound::i32x4;
using sbound::ld_nt_u4;

__device__ __forceinline__ bool bad_shape(const ExhScreenArgs& a, bool i8, size_t lds) {
    return a.lds < lds || a.dp == 0 || a.dp % (i8 ? 64u : 32u) != 0 || a.k < 1 || a.k > kExsMaxK || a.nq < 1 ||
           a.nq > kExsTile || a.nlist == 0 || a.chunk == 0;
}

// The next `chunk` blocks nobody has taken: [c0, c0 + cb), cb == 0 when the arena is done.
__device__ __forceinline__ unsigned long long take_chunk(unsigned long long* cursor, uint32_t chunk, uint64_t nb,
                                                         int lane, uint32_t& cb) {
    unsigned long long c0 = 0;
    if (lane == 0) c0 = atomicAdd(cursor, (unsigned long long)chunk);
    c0 = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(uint32_t)(c0 >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)c0);
    cb = c0 < nb ? (uint32_t)min((unsigned long long)chunk, nb - c0) : 0u;
    return c0;
}

// Arena block gb of list `list` against the tile's queries: emit(g, v, approx, del) for query
// g = 16 h + 4 (lane >> 4) + r < nq and slot v = 16 vt + (lane & 15). sbound::block_bounds with
// two A operands on one B stream; the arithmetic after the MFMAs is its, term for term.
template <int M, bool I8, class Emit>
__device__ __forceinline__ void block_bounds2(const ExhScreenArgs& a, uint32_t list, uint64_t gb, int lane, Emit&& emit) {
    const uint32_t dp = a.dp, ks = dp >> (I8 ? 6 : 5);
    const int nq = (int)a.nq;
    const bool two = nq > 16;  // (wave-uniform)
    const float cm = (float)(4 * dp + 16) * 0x1.02p-24f;
    const float cr = (float)(dp + 2) * 0x1.02p-24f;
    const float cu = 0x1.02p-23f;
    using AccT = std::conditional_t<I8, i32x4, f32x4>;
    // the A rows of this lane: query 16 h + (lane & 15), its 16 bytes (lane >> 4) of each k-step's 64
    const uint4* qa_row[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t g = (uint32_t)min(16 * h + (lane & 15), nq - 1);
        qa_row[h] = (const uint4*)((const char*)a.qres + ((size_t)g * a.nlist + list) * dp * (I8 ? 1 : 2)) + (lane >> 4);
    }
    const uint4* sp = a.shadow + gb * (uint64_t)ks * 256 + lane;
    uint4 xa[kDepth][4], qa[kDepth][2];
#pragma unroll
    for (int u = 0; u < kDepth; ++u) {
        if ((uint32_t)u < ks) {  // (wave-uniform)
#pragma unroll
            for (int vt = 0; vt < 4; ++vt) xa[u][vt] = ld_nt_u4(sp + (size_t)(u * 4 + vt) * 64);
            qa[u][0] = qa_row[0][4 * u];
            if (two) qa[u][1] = qa_row[1][4 * u];
        }
    }
    AccT acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int vt = 0; vt < 4; ++vt) acc[h][vt] = AccT{0, 0, 0, 0};
    for (uint32_t s0 = 0; s0 < ks; s0 += kDepth) {
        static_for<0, kDepth>([&](auto uu) {
            constexpr int u = decltype(uu)::value;
            if (s0 + u < ks) {  // (wave-uniform)
                if constexpr (I8) {
#pragma unroll
                    for (int vt = 0; vt < 4; ++vt)
                        acc[0][vt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(as_i32x4(qa[u][0]), as_i32x4(xa[u][vt]), acc[0][vt], 0, 0, 0);
                    if (two) {
#pragma unroll
                        for (int vt = 0; vt < 4; ++vt)
                            acc[1][vt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(as_i32x4(qa[u][1]), as_i32x4(xa[u][vt]), acc[1][vt], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int vt = 0; vt < 4; ++vt)
                        acc[0][vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(qa[u][0]), as_bf16x8(xa[u][vt]), acc[0][vt], 0, 0, 0);
                    if (two) {
#pragma unroll
                        for (int vt = 0; vt < 4; ++vt)
                            acc[1][vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(qa[u][1]), as_bf16x8(xa[u][vt]), acc[1][vt], 0, 0, 0);
                    }
                }
                const uint32_t nxt = s0 + u + kDepth;
                if (nxt < ks) {
#pragma unroll
                    for (int vt = 0; vt < 4; ++vt) xa[u][vt] = ld_nt_u4(sp + ((size_t)nxt * 4 + vt) * 64);
                    qa[u][0] = qa_row[0][4 * nxt];
                    if (two) qa[u][1] = qa_row[1][4 * nxt];
                }
            }
        });
    }
    float4 mt[4];
    float vsc[4];
#pragma unroll
    for (int vt = 0; vt < 4; ++vt) {
        const uint64_t mslot = gb * 64 + 16 * vt + (lane & 15);
        mt[vt] = a.meta[mslot];
        vsc[vt] = 0.0f;
        if constexpr (I8) vsc[vt] = a.sscale[mslot];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1 && !two) break;
        float4 pst[4];
        float qsc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t pr = (size_t)min(16 * h + 4 * (lane >> 4) + r, nq - 1) * a.nlist + list;
            pst[r] = a.pst[pr];
            qsc[r] = 0.0f;
            if constexpr (I8) qsc[r] = a.qscale[pr];
        }
#pragma unroll
        for (int vt = 0; vt < 4; ++vt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float dot;
                if constexpr (I8) dot = (float)acc[h][vt][r] * (qsc[r] * vsc[vt]);
                else dot = acc[h][vt][r];
                const float4 ps = pst[r];
                const float4 m = mt[vt];
                const float approx = M == kL2 ? (ps.x + m.x) - 2.0f * dot : -(ps.x + dot);
                const float an = ps.y + ps.z, bn = m.y + m.z;
                const float cs = an * m.z + ps.z * bn + ps.z * m.z;
                float del;
                if (M == kL2) {
                    const float rest = 2.0f * (cs + cm * (an * bn)) + cu * (ps.x + m.x + fabsf(approx));
                    del = rest + cr * (fabsf(approx) + rest);
                } else {
                    del = cs + cm * (an * bn) + cr * (ps.y * m.w) + cu * (ps.y * ps.w + an * bn + fabsf(approx));
                }
                del = del * 1.001f + 1e-30f;
                const int g = 16 * h + 4 * (lane >> 4) + r;
                if (g < nq) emit(g, 16 * vt + (lane & 15), approx, del);
            }
        }
    }
}

// Fold entries sd/si[0..n) (ascending by key; 64 at a time) into the unique-id list tk of capacity
// k. Stops at the first 64 with nothing below the k-th key. (As in exhaustive_kernels.hip.)
__device__ __forceinline__ void fold_sorted(WaveTopK<1>& tk, const float* sd, const uint64_t* si, int n, int k, float& kd,
                                            uint64_t& ki) {
    const int lane = lane_id();
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        const float cd = e < n ? sd[e] : __builtin_inff();
        const uint64_t ci = e < n ? si[e] : kNoId;
        uint64_t mask = __ballot(key_less(cd, ci, kd, ki));
        if (!mask) break;
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            tk.offer_unique(rd_lane(cd, l), rd_lane(ci, l), k, kd, ki);
        }
    }
}

__global__ void ivf_exs_probes(uint32_t* __restrict__ probes, uint32_t n, uint32_t nlist) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) probes[e] = e % nlist;
}

__global__ void ivf_exs_stage(unsigned long long* __restrict__ ctrl, uint32_t* __restrict__ shared_thr,
                              uint32_t* __restrict__ cnt, uint32_t nq) {
    const uint32_t t = threadIdx.x;
    if (t == 0) ctrl[kExsCursorT] = ctrl[kExsCursorB] = 0;
    if (t < kExsTile) shared_thr[t] = kThrInf;
    if (t < nq) cnt[t] = 0u;
}

template <int M, bool I8>
__global__ __launch_bounds__(64 * kExsWaves) void ivf_exh_screen_thresh(const ExhScreenArgs a) {
    extern __shared__ __align__(16) unsigned char exs_smem[];
    // the launcher's guard, restated: the lists and the tile must fit the LDS the launch gave
    if (bad_shape(a, I8, kExsThreshLds)) return;
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const int k = (int)a.k;
    const int nq = (int)a.nq;
    const float inf = __builtin_inff();
    uint64_t* all_i = (uint64_t*)exs_smem;                   // [waves][TQ][64]
    float* all_d = (float*)(all_i + kExsWaves * TQ * 64);    // [waves][TQ][64]
    float* all_t = all_d + kExsWaves * TQ * 64;              // [waves][TQ][64]: a block's ub, [query][slot]
    uint64_t* tk_i = all_i + (size_t)wave * TQ * 64;
    float* tk_d = all_d + (size_t)wave * TQ * 64;
    float* tile = all_t + (size_t)wave * TQ * 64;
    for (int e = lane; e < TQ * 64; e += 64) {
        tk_d[e] = inf;
        tk_i[e] = kNoId;
    }
    float kdv = inf;  // lane g: the k-th ub of this wave's list of query g
    for (;;) {
        uint32_t cb;
        const unsigned long long c0 = take_chunk(a.ctrl + kExsCursorT, a.chunk, a.nb, lane, cb);
        if (cb == 0) break;
        for (uint32_t j = 0; j < cb; ++j) {
            const uint64_t gb = c0 + j;  // < nb
            const uint32_t nvalid = rd_lane_u32((uint32_t)a.valid[gb], 0);
            if (nvalid == 0) continue;  // (wave-uniform) no shadow byte of this block is read
            const uint32_t list = rd_lane_u32(min(a.blist[gb], a.nlist - 1), 0);
            wave_sync();  // (the previous block's tile is read)
            block_bounds2<M, I8>(a, list, gb, lane, [&](int g, int v, float approx, float del) { tile[g * 64 + v] = approx + del; });
            wave_sync();
            // the gate per query: this list's k-th or what any wave of the grid has published
            float gate_v = kdv;
            if (lane < TQ) gate_v = fminf(kdv, ord_dec(__hip_atomic_load(a.shared_thr + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
            for (int g = 0; g < nq; ++g) {
                const float ub = tile[g * 64 + lane];
                const float gate = rd_lane(gate_v, g);
                const bool want = (uint32_t)lane < nvalid && ub < gate;  // (a NaN or +inf ub never counts)
                uint64_t mask = __ballot(want);
                if (!mask) continue;  // (wave-uniform)
                const uint64_t id = want ? a.ids[gb * 64 + lane] : kNoId;
                WaveTopK<1> tk;
                tk.d[0] = tk_d[g * 64 + lane];
                tk.id[0] = tk_i[g * 64 + lane];
                float nkd;
                uint64_t nki;
                tk.at(k - 1, nkd, nki);
                while (mask) {
                    const int l = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    tk.offer_unique(rd_lane(ub, l), rd_lane(id, l), k, nkd, nki);
                }
                tk_d[g * 64 + lane] = tk.d[0];
                tk_i[g * 64 + lane] = tk.id[0];
                if (lane == g) kdv = nkd;
                // k distinct ids at or below nkd: a bound on T_g every wave may use
                if (nkd < gate && lane == 0) atomicMin(a.shared_thr + g, ord_enc(nkd));
            }
        }
    }
    // the workgroup's 4 wave lists to one per query, then out as this workgroup's partial
    __syncthreads();
    for (int g = (int)wave; g < nq; g += (int)kExsWaves) {
        WaveTopK<1> tk;
        tk.d[0] = all_d[(size_t)g * 64 + lane];  // wave 0's
        tk.id[0] = all_i[(size_t)g * 64 + lane];
        float fd;
        uint64_t fi;
        tk.at(k - 1, fd, fi);
        for (uint32_t v = 1; v < kExsWaves; ++v)
            fold_sorted(tk, all_d + ((size_t)v * TQ + g) * 64, all_i + ((size_t)v * TQ + g) * 64, k, k, fd, fi);
        const size_t o = ((size_t)blockIdx.x * TQ + g) * k;
        if (lane < k) {
            a.part_d[o + lane] = tk.d[0];
            a.part_i[o + lane] = tk.id[0];
        }
    }
}

template <int M, bool I8>
__global__ __launch_bounds__(64 * kExsWaves) void ivf_exh_screen_bound(const ExhScreenArgs a) {
    extern __shared__ __align__(16) unsigned char exs_smem[];
    if (bad_shape(a, I8, kExsTileLds)) return;
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const int nq = (int)a.nq;
    float* tile = (float*)exs_smem + (size_t)wave * TQ * 64;  // a block's lb, [query][slot]
    // lane g: T_g, fixed before this launch; fewer than k distinct ids discard nothing
    float tv = __builtin_inff();
    if (lane < nq) {
        tv = a.thr[(size_t)lane * a.k + a.k - 1];
        if (!(tv < FLT_MAX)) tv = __builtin_inff();
    }
    unsigned long long rows = 0;
    for (;;) {
        uint32_t cb;
        const unsigned long long c0 = take_chunk(a.ctrl + kExsCursorB, a.chunk, a.nb, lane, cb);
        if (cb == 0) break;
        for (uint32_t j = 0; j < cb; ++j) {
            const uint64_t gb = c0 + j;  // < nb
            const uint32_t nvalid = rd_lane_u32((uint32_t)a.valid[gb], 0);
            if (nvalid == 0) continue;
            const uint32_t list = rd_lane_u32(min(a.blist[gb], a.nlist - 1), 0);
            rows += nvalid;
            wave_sync();
            block_bounds2<M, I8>(a, list, gb, lane, [&](int g, int v, float approx, float del) { tile[g * 64 + v] = approx - del; });
            wave_sync();
            for (int g = 0; g < nq; ++g) {
                const float lb = tile[g * 64 + lane];
                const bool c = (uint32_t)lane < nvalid && !(lb > rd_lane(tv, g));  // (a NaN bound is kept)
                const uint64_t mm = __ballot(c);
                if (!mm) continue;  // (wave-uniform)
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(a.cnt + g, (uint32_t)__popcll(mm));
                at = rd_lane_u32(at, 0);
                const uint64_t idx = (uint64_t)at + __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
                if (c && idx < a.cap) a.cand[(size_t)g * a.cap + idx] = (uint32_t)(gb * 64 + lane);
            }
        }
    }
    if (lane == 0 && rows) atomicAdd(a.ctrl + kExsRows, rows * (unsigned long long)nq);
}

template <int M>
__global__ __launch_bounds__(64 * kExsWaves) void ivf_exh_screen_select(const ExhSelectArgs a) {
    __shared__ float s_d[kExsWaves][64];
    __shared__ uint64_t s_i[kExsWaves][64];
    if (a.k < 1 || a.k > kExsMaxK || a.d4 == 0 || blockIdx.x >= a.nq) return;
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const int k = (int)a.k;
    const uint32_t q = blockIdx.x, d4 = a.d4;
    const uint64_t n = a.cnt[q];
    if (n > a.cap) return;  // (workgroup-uniform) the tile falls back: nothing is written
    const float4* __restrict__ q4 = (const float4*)(a.q + (size_t)q * d4 * 4);  // (wave-uniform reads)
    const uint32_t* __restrict__ cand = a.cand + (size_t)q * a.cap;
    WaveTopK<1> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    for (uint64_t c0 = (uint64_t)wave * 64; c0 < n; c0 += 64 * kExsWaves) {
        const bool act = c0 + lane < n;
        const uint32_t slot = cand[act ? c0 + lane : n - 1];  // (a lane past the end repeats the last)
        const float4* __restrict__ row = a.rows + (uint64_t)slot * d4;
        float acc = 0.0f;
        for (uint32_t t0 = 0; t0 < d4; t0 += 8) {
            float4 x[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = t0 + t < d4 ? load_nt(row + t0 + t) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t0 + t < d4) acc = acc4<M>(acc, q4[t0 + t], x[t]);
        }
        const float dv = dist_finish<M>(acc);
        const uint64_t id = act ? a.ids[slot] : kNoId;
        uint64_t mask = __ballot(act && dv <= kd);
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            tk.offer_unique(rd_lane(dv, l), rd_lane(id, l), k, kd, ki);
        }
    }
    s_d[wave][lane] = tk.d[0];
    s_i[wave][lane] = tk.id[0];
    __syncthreads();
    if (wave != 0) return;
    for (uint32_t v = 1; v < kExsWaves; ++v) fold_sorted(tk, s_d[v], s_i[v], k, k, kd, ki);
    if (lane < k) {
        const bool real = tk.id[0] != kNoId;
        a.out_d[(size_t)q * k + lane] = real ? tk.d[0] : FLT_MAX;
        a.out_i[(size_t)q * k + lane] = tk.id[0];
    }
}

void guard(const ExhScreenArgs& a, size_t lds, const char* what) {
    const bool i8 = a.sscale != nullptr;
    if (lds > kLdsBytes || a.lds != lds || a.k < 1 || a.k > kExsMaxK || a.nq < 1 || a.nq > kExsTile || a.dp == 0 ||
        a.dp % (i8 ? 64u : 32u) != 0 || a.nlist == 0 || a.chunk == 0)
        throw std::length_error(what);
}

template <int M, bool I8>
void thresh_t(const ExhScreenArgs& a, uint32_t grid, hipStream_t s) {
    static const bool once = [] {
        (void)hipFuncSetAttribute((const void*)ivf_exh_screen_thresh<M, I8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kExsThreshLds);
        return true;
    }();
    (void)once;
    ivf_exh_screen_thresh<M, I8><<<grid, 64 * kExsWaves, a.lds, s>>>(a);
}

template <int M, bool I8>
void bound_t(const ExhScreenArgs& a, uint32_t grid, hipStream_t s) {
    ivf_exh_screen_bound<M, I8><<<grid, 64 * kExsWaves, a.lds, s>>>(a);
}

}  // namespace

void launch_exs_probes(uint32_t* probes, uint32_t tile, uint32_t nlist, hipStream_t s) {
    const uint32_t n = tile * nlist;
    if (!n) return;
    ivf_exs_probes<<<std::min<uint32_t>((n + 255) / 256, 1024), 256, 0, s>>>(probes, n, nlist);
}

void launch_exs_stage(unsigned long long* ctrl, uint32_t* shared_thr, uint32_t* cnt, uint32_t nq, hipStream_t s) {
    ivf_exs_stage<<<1, 64, 0, s>>>(ctrl, shared_thr, cnt, std::min(nq, kExsTile));
}

void launch_exs_thresh(int metric, const ExhScreenArgs& a, uint32_t grid, hipStream_t s) {
    guard(a, kExsThreshLds, "ivf_exh_screen_thresh: the tile's threshold lists do not fit the LDS");
    if (!grid) return;
    const bool i8 = a.sscale != nullptr;
    if (metric == kL2) i8 ? thresh_t<kL2, true>(a, grid, s) : thresh_t<kL2, false>(a, grid, s);
    else i8 ? thresh_t<kIP, true>(a, grid, s) : thresh_t<kIP, false>(a, grid, s);
}

void launch_exs_bound(int metric, const ExhScreenArgs& a, uint32_t grid, hipStream_t s) {
    guard(a, kExsTileLds, "ivf_exh_screen_bound: the tile's bounds do not fit the LDS");
    if (!grid) return;
    const bool i8 = a.sscale != nullptr;
    if (metric == kL2) i8 ? bound_t<kL2, true>(a, grid, s) : bound_t<kL2, false>(a, grid, s);
    else i8 ? bound_t<kIP, true>(a, grid, s) : bound_t<kIP, false>(a, grid, s);
}

void launch_exs_select(int metric, const ExhSelectArgs& a, hipStream_t s) {
    if (a.k < 1 || a.k > kExsMaxK) throw std::length_error("ivf_exh_screen_select: k does not fit one list register");
    if (!a.nq) return;
    if (metric == kL2) ivf_exh_screen_select<kL2><<<a.nq, 64 * kExsWaves, 0, s>>>(a);
    else ivf_exh_screen_select<kIP><<<a.nq, 64 * kExsWaves, 0, s>>>(a);
}

}  // namespace vdbk
