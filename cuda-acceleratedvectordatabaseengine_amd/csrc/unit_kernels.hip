// unit_kernels.hip — the two kernels behind Metric::CosineDistance (gfx950, wave64).
//
// ivf_unit_rows: one wavefront per row. The row is read once (its first kKeep * 256 floats stay
// in registers, a longer row's tail is read again from cache), its squares are summed in the
// fixed order unit_kernels.hpp states, and the unit row is written zero-padded to dp floats:
// the bytes launch_pad_rows moves, plus one wave reduction. Bandwidth-bound.
//
// ivf_cos_finish: the distance mapping on a batch's final output, element-wise.
//
// Built with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt (the Makefile's
// FLAGS): the plain *, +, / and sqrt below are each one correctly rounded fp32 operation. (HIP's
// __fsqrt_rn is the native approximation unless OCML's rounded operations are compiled in: not
// used.) The pragma keeps the products and sums apart whatever flags a build passes.
#include "unit_kernels.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace vdbk {
namespace {

constexpr int kKeep = 4;  // float4 groups per lane kept in registers between the two passes (dim <= 1024)

// Group j of a row: elements 4j .. 4j + 3, missing ones +0.
template <bool VEC>
__device__ __forceinline__ float4 load_group(const float* __restrict__ row, uint32_t j, uint32_t dim) {
    const uint64_t i = (uint64_t)j * 4;
    if constexpr (VEC) {  // (the row base is 16-byte aligned and dim % 4 == 0: a group is whole or absent)
        return *(const float4*)(row + i);
    } else {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i + 0 < dim) v.x = row[i + 0];
        if (i + 1 < dim) v.y = row[i + 1];
        if (i + 2 < dim) v.z = row[i + 2];
        if (i + 3 < dim) v.w = row[i + 3];
        return v;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_group(float* __restrict__ row, uint32_t j, uint32_t dp, float4 v) {
    const uint64_t i = (uint64_t)j * 4;
    if constexpr (VEC) {
        *(float4*)(row + i) = v;
    } else {
        if (i + 0 < dp) row[i + 0] = v.x;
        if (i + 1 < dp) row[i + 1] = v.y;
        if (i + 2 < dp) row[i + 2] = v.z;
        if (i + 3 < dp) row[i + 3] = v.w;
    }
}

// p + x^2 + y^2 + z^2 + w^2 in ascending element order: each product rounded, each sum rounded.
__device__ __forceinline__ float add_squares(float p, float4 v) {
    p = p + v.x * v.x;
    p = p + v.y * v.y;
    p = p + v.z * v.z;
    p = p + v.w * v.w;
    return p;
}

__device__ __forceinline__ float4 scaled(float4 v, float norm, bool ok) {
    if (!ok) return v;
    return make_float4(v.x / norm, v.y / norm, v.z / norm, v.w / norm);
}

template <bool VIN, bool VOUT>
__global__ void __launch_bounds__(256)
ivf_unit_rows(const float* __restrict__ src, uint64_t n, uint32_t dim, uint32_t dp, float* __restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    const uint32_t gin = dim / 4 + (dim % 4 != 0);  // groups holding an input element
    const uint32_t gout = dp / 4 + (dp % 4 != 0);   // groups holding an output element (dp >= dim)
    for (uint64_t r = wave; r < n; r += nwaves) {
        const float* x = src + r * dim;
        float* y = dst + r * dp;
        float4 keep[kKeep];
        float p = 0.0f;
#pragma unroll
        for (int c = 0; c < kKeep; ++c) {
            const uint32_t j = lane + 64u * c;
            keep[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (j < gin) {
                keep[c] = load_group<VIN>(x, j, dim);
                p = add_squares(p, keep[c]);
            }
        }
        for (uint32_t j = lane + 64u * kKeep; j < gin; j += 64) p = add_squares(p, load_group<VIN>(x, j, dim));
        // p[l] += p[l + s], s = 32 .. 1, as a xor butterfly: every lane ends with lane 0's bits
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s, 64);
        const float norm = __builtin_sqrtf(p);
        const bool ok = norm > 0.0f && norm < INFINITY;  // (a NaN fails both)
#pragma unroll
        for (int c = 0; c < kKeep; ++c) {
            const uint32_t j = lane + 64u * c;
            if (j < gout) store_group<VOUT>(y, j, dp, scaled(keep[c], norm, ok));  // (past the input: the +0 pad)
        }
        for (uint32_t j = lane + 64u * kKeep; j < gout; j += 64) {
            const float4 v = j < gin ? load_group<VIN>(x, j, dim) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            store_group<VOUT>(y, j, dp, scaled(v, norm, ok));
        }
    }
}

__global__ void __launch_bounds__(256)
ivf_cos_finish(float* __restrict__ dist, const uint64_t* __restrict__ ids, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (ids[i] != ~0ull) dist[i] = 1.0f + dist[i];
}

inline uint32_t grid_for(uint64_t items, uint32_t per_block) {
    const uint64_t b = (items + per_block - 1) / per_block;
    return (uint32_t)(b < (1ull << 20) ? (b ? b : 1) : (1ull << 20));
}

}  // namespace

void launch_unit_rows(const float* src, uint64_t n, uint32_t dim, uint32_t dp_out, float* dst, hipStream_t s) {
    if (!n || !dp_out) return;
    const bool vin = ((uintptr_t)src & 15) == 0 && dim % 4 == 0;
    const bool vout = ((uintptr_t)dst & 15) == 0 && dp_out % 4 == 0;
    const uint32_t g = grid_for(n, 4);  // one wavefront per row, four per workgroup
    if (vin && vout) ivf_unit_rows<true, true><<<g, 256, 0, s>>>(src, n, dim, dp_out, dst);
    else if (vin) ivf_unit_rows<true, false><<<g, 256, 0, s>>>(src, n, dim, dp_out, dst);
    else if (vout) ivf_unit_rows<false, true><<<g, 256, 0, s>>>(src, n, dim, dp_out, dst);
    else ivf_unit_rows<false, false><<<g, 256, 0, s>>>(src, n, dim, dp_out, dst);
}

void launch_cos_finish(float* dist, const uint64_t* ids, uint64_t n, hipStream_t s) {
    if (!n) return;
    ivf_cos_finish<<<grid_for(n, 256), 256, 0, s>>>(dist, ids, n);
}

}  // namespace vdbk
