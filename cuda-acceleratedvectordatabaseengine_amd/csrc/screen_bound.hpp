// screen_bound.hpp — what the two shadow kernels of vdb_ivf_search_prepared_screened share on
// the device (filter_screen_kernels.hip; gfx950, wave64): one block's shadow streamed through the
// matrix cores against up to 16 pairs, and every (pair, slot)'s `approx` and `del`, the
// operations of collect_segment (screen.hip) in its order. A file that includes this is compiled
// with contraction off, so lb = approx - del and ub = approx + del agree with the screened search
// bit for bit. ivf_range_screen (range_screen_kernels.hip) holds the same stream as a copy of its
// own: calling this header from it changed that kernel's register allocation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "scan_common.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace sbound {

// k-steps of a block's shadow in flight per wave (4 KiB each), as in ivf_range_screen.
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

// The handle's screen and the batch's pairs, as the bound needs them.
struct BoundSrc {
    const uint4* shadow;   // per block dp / 32 (bf16) or dp / 64 (int8) k-steps x 4 vector tiles x 64 lanes
    const float4* meta;    // per slot {|b|^2, |b| up, |b - b'| up, |x| up}
    const float* sscale;   // int8: per slot s_b
    const float4* pst;     // per pair (launch_screen_pairs)
    const float* qscale;   // int8: per pair s_a
    uint32_t dp;
};

// The MFMA A row of this lane for the item's pairs inv[p0 .. p0 + np): pair (lane & 15) (rows at
// or above np repeat the last pair and are dropped by the caller), its 16 bytes (lane >> 4) of
// each k-step's 64.
template <bool I8>
__device__ __forceinline__ const uint4* a_row(const void* qres, const uint32_t* inv, uint32_t p0, int np, uint32_t dp,
                                              int lane) {
    const uint32_t pa = inv[p0 + (uint32_t)min(lane & 15, np - 1)];
    return (const uint4*)((const char*)qres + (size_t)pa * dp * (I8 ? 1 : 2)) + (lane >> 4);
}

// Arena block gb against the 16 A rows at qa_row: emit(vt, r, approx, del) for the 16 (pair,
// slot) of this lane, slot 16 vt + (lane & 15) of the block, pair pr[r] (row 4 (lane >> 4) + r of
// the item). The block's k-steps go through the matrix cores kDepth in flight, none beyond the
// block.
template <int M, bool I8, class Emit>
__device__ __forceinline__ void block_bounds(const BoundSrc& a, const uint4* qa_row, const uint32_t (&pr)[4],
                                             uint64_t gb, int lane, Emit&& emit) {
    const uint32_t dp = a.dp, ks = dp >> (I8 ? 6 : 5);  // (k-steps of 64 int8 or 32 bf16 dims)
    // the bound's rounding coefficients (collect_segment's)
    const float cm = (float)(4 * dp + 16) * 0x1.02p-24f;
    const float cr = (float)(dp + 2) * 0x1.02p-24f;
    const float cu = 0x1.02p-23f;
    using AccT = std::conditional_t<I8, i32x4, f32x4>;
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
    float4 pst[4];
    float qsc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pst[r] = a.pst[pr[r]];
        qsc[r] = 0.0f;
        if constexpr (I8) qsc[r] = a.qscale[pr[r]];
    }
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
            emit(vt, r, approx, del);
        }
    }
}

}  // namespace sbound
}  // namespace vdbk
