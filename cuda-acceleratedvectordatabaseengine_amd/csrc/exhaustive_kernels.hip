// exhaustive_kernels.hip — the kernels behind vdb_ivf_search_exhaustive (gfx950, wave64).
//
// ivf_exhaustive_scan: the arena is one run of 64-row blocks, and a persistent grid walks it
// in storage order whatever list a block belongs to. A wave takes `chunk` consecutive blocks
// at a time from an atomic cursor and streams them once for the whole tile of TQ queries:
//   * lane = row. Rows arrive as the wide scan's do: one float4 column per wave load (1 KiB,
//     non-temporal) from the interleaved arena, or 16 bytes of the lane's own row from the
//     row-major copy, 8 columns in flight per lane; the prefetch stops at the chunk's last
//     column (it is re-read, never passed), so nothing past the wave's blocks is touched.
//   * the queries are wave-uniform: the tile is staged dimension-major (qt[d][TQ]) and read
//     through the constant address space, so a dimension's TQ values arrive as scalar loads
//     into SGPR pairs (q[2p][d], q[2p+1][d]) and feed the packed v_pk_add_f32 / v_pk_mul_f32
//     as their one scalar operand. No LDS and no VGPR is spent on queries.
//   * TQ fp32 accumulators per lane, two queries per packed instruction; each half rounds as
//     the scalar diff = a - b; acc = acc + diff * diff does, d = 0..D-1 from +0.0f (sub, mul,
//     add stay separate: 1.5 packed instructions per query-dimension for L2, 1 for IP).
//   * per query a unique-id list of 64 R entries per wave in LDS; only the k-th distance stays
//     in registers. A block is tested with one compare and a ballot per query; survivors go
//     through WaveTopK::offer_unique (a ballot search for the id, then the ordered insert).
//     Pad lanes (lane >= the block's valid rows) compute like the others and are never offered.
// At the end of the tile the workgroup's 4 wave lists fold to one per query and go out as the
// workgroup's partial. ivf_exhaustive_merge folds the grid's partials per query.
//
// Unique partials are what makes the fold exact: a row left out of a unique partial has k
// distinct ids with smaller keys before it in that partial's rows, so k distinct ids beat it
// in the whole index too. A multiset partial lacks that (two copies of one id count twice).
#pragma clang fp contract(off)
#include "exhaustive_kernels.hpp"

#include <cfloat>
#include <stdexcept>

#include "scan_common.hpp"
#include "wave_topk.hpp"

namespace vdbk {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef const f2 __attribute__((address_space(4))) cf2;  // wave-uniform reads: scalar loads

constexpr int kExhPipe = 8;  // float4 columns in flight per lane

// Packed term for the query pair q (an SGPR pair) against one row value held in half H of the
// aligned register pair x; the broadcast is an op_sel, as in the wide scan.
template <int H>
__device__ __forceinline__ f2 pk_sub_s(f2 q, f2 x) {
    f2 r;
    if constexpr (H == 0)
        asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "s"(q), "v"(x));
    else
        asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "s"(q), "v"(x));
    return r;
}
template <int H>
__device__ __forceinline__ f2 pk_mul_s(f2 q, f2 x) {
    f2 r;
    if constexpr (H == 0)
        asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "s"(q), "v"(x));
    else
        asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "s"(q), "v"(x));
    return r;
}
template <int M, int H>
__device__ __forceinline__ f2 exh_term2(f2 acc, f2 q, f2 x) {
    if constexpr (M == kL2) {
        const f2 diff = pk_sub_s<H>(q, x);
        return acc + diff * diff;
    } else if constexpr (M == kIP) {
        return acc + pk_mul_s<H>(q, x);
    } else {
        return acc;
    }
}

// Fold entries sd/si[0..n) (ascending by key; this lane's view of them, 64 at a time) into the
// unique-id list tk of capacity k. Stops at the first 64 with nothing below the k-th key.
template <int R>
__device__ __forceinline__ void fold_sorted(WaveTopK<R>& tk, const float* sd, const uint64_t* si, int n, int k,
                                            float& kd, uint64_t& ki) {
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

template <int R>
__device__ __forceinline__ void list_load(WaveTopK<R>& tk, const float* sd, const uint64_t* si) {
    const int lane = lane_id();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        tk.d[r] = sd[r * 64 + lane];
        tk.id[r] = si[r * 64 + lane];
    }
}

__global__ void ivf_exh_valid_clear(uint64_t nb, uint8_t* __restrict__ valid) {
    for (uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * blockDim.x)
        valid[b] = 0;
}

// one wave per list, lanes over its blocks
__global__ void ivf_exh_valid_fill(const uint64_t* __restrict__ block_off, const uint32_t* __restrict__ count,
                                   uint32_t nlist, uint64_t nb, uint8_t* __restrict__ valid) {
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t l = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); l < nlist; l += waves) {
        const uint32_t c = count[l];
        const uint64_t b0 = block_off[l];
        const uint32_t blocks = (c + 63) >> 6;
        for (uint32_t b = lane; b < blocks; b += 64)
            if (b0 + b < nb) valid[b0 + b] = (uint8_t)min(64u, c - b * 64);
    }
}

__global__ void ivf_exh_stage(const float* __restrict__ q, uint32_t nq, uint32_t dp, uint32_t tile,
                              float* __restrict__ qt, unsigned long long* __restrict__ cursor) {
    const uint32_t n = dp * tile;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const uint32_t d = e / tile, g = e % tile;
        qt[e] = g < nq ? q[(size_t)g * dp + d] : 0.0f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *cursor = 0;
}

template <int M, bool ROWS, int TQ>
__global__ __launch_bounds__(64 * kExhWaves) void ivf_exhaustive_scan(const ExhScanArgs a) {
    constexpr int R = (int)kExhMaxTile / TQ;
    constexpr int GP = TQ / 2;
    constexpr int CAP = 64 * R;
    constexpr int T = kExhPipe;
    extern __shared__ __align__(16) unsigned char exh_smem[];
    // the launcher's guard, restated: the lists must fit the LDS the launch gave
    if (a.lds < (uint32_t)(kExhWaves * TQ * CAP * 12) || a.k == 0 || a.k > (uint32_t)CAP || a.nq == 0 ||
        a.nq > (uint32_t)TQ)
        return;
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const int k = (int)a.k;
    const int nq = (int)a.nq;
    const uint32_t d4 = a.d4;
    uint64_t* all_i = (uint64_t*)exh_smem;                // [waves][TQ][CAP]
    float* all_d = (float*)(all_i + kExhWaves * TQ * CAP);  // [waves][TQ][CAP]
    uint64_t* tk_i = all_i + (size_t)wave * TQ * CAP;
    float* tk_d = all_d + (size_t)wave * TQ * CAP;
    for (int e = lane; e < TQ * CAP; e += 64) {
        tk_d[e] = __builtin_inff();
        tk_i[e] = kNoId;
    }
    cf2* qc = (cf2*)(uintptr_t)a.qt;

    float kd[TQ];
    f2 acc[GP];
#pragma unroll
    for (int g = 0; g < TQ; ++g) kd[g] = __builtin_inff();
#pragma unroll
    for (int p = 0; p < GP; ++p) acc[p] = f2{0.0f, 0.0f};
    auto qsum = [&](int g) -> float { return (g & 1) ? acc[g >> 1].y : acc[g >> 1].x; };

    for (;;) {
        unsigned long long c0 = 0;
        if (lane == 0) c0 = atomicAdd(a.cursor, (unsigned long long)a.chunk);
        c0 = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(uint32_t)(c0 >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)c0);
        if (c0 >= a.nb) break;
        const uint32_t cb = (uint32_t)min((unsigned long long)a.chunk, a.nb - c0);  // blocks [c0, c0 + cb) < nb

        const float4* base = ROWS ? a.lists + (c0 * 64 + (uint64_t)lane) * d4 : a.lists + c0 * d4 * 64 + lane;
        // the prefetch position, clamped to the chunk's last column
        uint32_t pj = 0, pt = 0;
        auto fetch = [&]() -> float4 {
            float4 v;
            if constexpr (ROWS) v = base[(size_t)pj * 64 * d4 + pt];
            else v = load_nt(base + ((size_t)pj * d4 + pt) * 64);
            if (pt + 1 < d4) ++pt;
            else if (pj + 1 < cb) ++pj, pt = 0;
            return v;
        };
        float4 x[T];
        if constexpr (M != kCos) {
#pragma unroll
            for (int t = 0; t < T; ++t) x[t] = fetch();
        }
        for (uint32_t j = 0; j < cb; ++j) {
            const uint64_t id = __builtin_nontemporal_load(a.ids + (c0 + j) * 64 + lane);
            const uint32_t nvalid = a.valid[c0 + j];
            if constexpr (M != kCos) {
                for (uint32_t t0 = 0; t0 < d4; t0 += T) {  // (d4 is a multiple of 16)
                    static_for<0, T>([&](auto u) {
                        constexpr int t = decltype(u)::value;
                        const f2 xlo = {x[t].x, x[t].y}, xhi = {x[t].z, x[t].w};
                        cf2* qr = qc + (size_t)(t0 + t) * 4 * GP;  // dims 4 (t0 + t) .. + 3, GP pairs each
#pragma unroll
                        for (int p = 0; p < GP; ++p) {
                            acc[p] = exh_term2<M, 0>(acc[p], qr[p], xlo);
                            acc[p] = exh_term2<M, 1>(acc[p], qr[GP + p], xlo);
                            acc[p] = exh_term2<M, 0>(acc[p], qr[2 * GP + p], xhi);
                            acc[p] = exh_term2<M, 1>(acc[p], qr[3 * GP + p], xhi);
                        }
                        x[t] = fetch();
                    });
                }
            }
            // the block's distances against each query's k-th: one compare and a ballot
            const bool valid = (uint32_t)lane < nvalid;
            uint32_t pend = 0;
#pragma unroll
            for (int g = 0; g < TQ; ++g) {
                const float dist = dist_finish<M>(qsum(g));
                if (g < nq && __ballot(valid && dist <= kd[g])) pend |= 1u << g;
            }
            while (pend) {
                const int gs = __builtin_ctz(pend);
                pend &= pend - 1;
                float dist = 0.0f, kdg = 0.0f;
#pragma unroll
                for (int g = 0; g < TQ; ++g)
                    if (g == gs) {
                        dist = dist_finish<M>(qsum(g));
                        kdg = kd[g];
                    }
                float* sd = tk_d + gs * CAP;
                uint64_t* si = tk_i + gs * CAP;
                WaveTopK<R> tk;
                list_load<R>(tk, sd, si);
                float nkd;
                uint64_t nki;
                tk.at(k - 1, nkd, nki);
                uint64_t mask = __ballot(valid && dist <= kdg);
                while (mask) {
                    const int l = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    tk.offer_unique(rd_lane(dist, l), rd_lane(id, l), k, nkd, nki);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    sd[r * 64 + lane] = tk.d[r];
                    si[r * 64 + lane] = tk.id[r];
                }
#pragma unroll
                for (int g = 0; g < TQ; ++g)
                    if (g == gs) kd[g] = nkd;
            }
#pragma unroll
            for (int p = 0; p < GP; ++p) acc[p] = f2{0.0f, 0.0f};
        }
    }

    // the workgroup's 4 wave lists to one per query, then out as this workgroup's partial
    __syncthreads();
    for (int g = (int)wave; g < nq; g += (int)kExhWaves) {
        WaveTopK<R> tk;
        list_load<R>(tk, all_d + (size_t)g * CAP, all_i + (size_t)g * CAP);  // wave 0's
        float fd;
        uint64_t fi;
        tk.at(k - 1, fd, fi);
        for (uint32_t v = 1; v < kExhWaves; ++v)
            fold_sorted<R>(tk, all_d + ((size_t)v * TQ + g) * CAP, all_i + ((size_t)v * TQ + g) * CAP, k, k, fd, fi);
        const size_t o = ((size_t)blockIdx.x * TQ + g) * k;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = r * 64 + lane;
            if (e < k) {
                a.part_d[o + e] = tk.d[r];
                a.part_i[o + e] = tk.id[r];
            }
        }
    }
}

template <int R>
__global__ __launch_bounds__(64) void ivf_exhaustive_merge(const float* __restrict__ part_d,
                                                           const uint64_t* __restrict__ part_i, uint32_t grid,
                                                           uint32_t tile, uint32_t k, float* __restrict__ out_d,
                                                           uint64_t* __restrict__ out_i) {
    if (k == 0 || k > 64u * R) return;
    const int lane = lane_id();
    const uint32_t q = blockIdx.x;
    WaveTopK<R> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    for (uint32_t w = 0; w < grid; ++w) {
        const size_t o = ((size_t)w * tile + q) * k;
        fold_sorted<R>(tk, part_d + o, part_i + o, (int)k, (int)k, kd, ki);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t e = r * 64 + lane;
        if (e < k) {
            const bool real = tk.id[r] != kNoId;
            out_d[(size_t)q * k + e] = real ? tk.d[r] : FLT_MAX;
            out_i[(size_t)q * k + e] = tk.id[r];
        }
    }
}

template <int M, bool ROWS, int TQ>
void launch_scan_t(const ExhScanArgs& a, uint32_t grid, hipStream_t s) {
    static const bool once = [] {
        (void)hipFuncSetAttribute((const void*)ivf_exhaustive_scan<M, ROWS, TQ>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)exhaustive_sizing(1).lds);
        return true;
    }();
    (void)once;
    ivf_exhaustive_scan<M, ROWS, TQ><<<grid, 64 * kExhWaves, a.lds, s>>>(a);
}

template <int M, bool ROWS>
void launch_scan_m(const ExhScanArgs& a, uint32_t tile, uint32_t grid, hipStream_t s) {
    switch (tile) {
        case 32: return launch_scan_t<M, ROWS, 32>(a, grid, s);
        case 16: return launch_scan_t<M, ROWS, 16>(a, grid, s);
        case 8: return launch_scan_t<M, ROWS, 8>(a, grid, s);
        case 4: return launch_scan_t<M, ROWS, 4>(a, grid, s);
        default: return launch_scan_t<M, ROWS, 2>(a, grid, s);
    }
}

}  // namespace

void launch_exh_block_valid(const uint64_t* block_off, const uint32_t* count, uint32_t nlist, uint64_t nb,
                            uint8_t* valid, hipStream_t s) {
    if (nb == 0) return;
    ivf_exh_valid_clear<<<(unsigned)std::min<uint64_t>((nb + 255) / 256, 1024), 256, 0, s>>>(nb, valid);
    if (nlist) ivf_exh_valid_fill<<<std::min<uint32_t>((nlist + 3) / 4, 1024), 256, 0, s>>>(block_off, count, nlist, nb, valid);
}

void launch_exh_stage(const float* q, uint32_t nq, uint32_t dp, uint32_t tile, float* qt, unsigned long long* cursor,
                      hipStream_t s) {
    ivf_exh_stage<<<std::min<uint32_t>((dp * tile + 255) / 256, 256), 256, 0, s>>>(q, nq, dp, tile, qt, cursor);
}

void launch_exh_scan(int metric, const ExhScanArgs& a, uint32_t grid, hipStream_t s) {
    const ExhSizing z = exhaustive_sizing(a.k);
    if (a.k == 0 || a.k > (uint32_t)kMaxK || z.lds > kLdsBytes || a.lds != z.lds || a.nq == 0 || a.nq > z.tile)
        throw std::length_error("ivf_exhaustive_scan: the tile's top-k lists do not fit the LDS");
    const bool rows = a.rows != 0;
    if (metric == kL2) rows ? launch_scan_m<kL2, true>(a, z.tile, grid, s) : launch_scan_m<kL2, false>(a, z.tile, grid, s);
    else if (metric == kIP) rows ? launch_scan_m<kIP, true>(a, z.tile, grid, s) : launch_scan_m<kIP, false>(a, z.tile, grid, s);
    else launch_scan_m<kCos, false>(a, z.tile, grid, s);  // (no row is read: every distance is 0.0f)
}

void launch_exh_merge(const float* part_d, const uint64_t* part_i, uint32_t grid, uint32_t tile, uint32_t nq,
                      uint32_t k, float* out_d, uint64_t* out_i, hipStream_t s) {
    if (nq == 0) return;
    switch (topk_regs(k)) {
        case 1: ivf_exhaustive_merge<1><<<nq, 64, 0, s>>>(part_d, part_i, grid, tile, k, out_d, out_i); break;
        case 2: ivf_exhaustive_merge<2><<<nq, 64, 0, s>>>(part_d, part_i, grid, tile, k, out_d, out_i); break;
        case 4: ivf_exhaustive_merge<4><<<nq, 64, 0, s>>>(part_d, part_i, grid, tile, k, out_d, out_i); break;
        case 8: ivf_exhaustive_merge<8><<<nq, 64, 0, s>>>(part_d, part_i, grid, tile, k, out_d, out_i); break;
        default: ivf_exhaustive_merge<16><<<nq, 64, 0, s>>>(part_d, part_i, grid, tile, k, out_d, out_i); break;
    }
}

}  // namespace vdbk
