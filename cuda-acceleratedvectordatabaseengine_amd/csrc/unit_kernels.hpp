// unit_kernels.hpp — launchers of the two kernels behind Metric::CosineDistance
// (unit_kernels.hip, gfx950, wave64): rows to unit length once when they enter the index or a
// batch, and the distance mapping on a batch's final output. Everything between the two is the
// inner-product machinery, unchanged.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vdbk {

// dst[r] = unit(src[r]) zero-padded to dp_out floats, one wavefront per row. src is row-major
// [n][dim], dst row-major [n][dp_out], dp_out >= dim; dst may not alias src (src is only read).
//
// unit(x), fixed so that a host restatement gives the same bits: with j = i / 4, element i
// belongs to lane j % 64; a lane adds the squares of its elements in ascending i (fp32, the
// product rounded, then the sum rounded, no fused multiply-add); the 64 partials combine by
// p[l] += p[l + s] for s = 32, 16, 8, 4, 2, 1 (a xor butterfly: the same bits in every lane);
// norm = sqrt of that sum, correctly rounded; if norm is finite and > 0 every element becomes
// x[i] / norm (a correctly rounded division, not a multiply by a reciprocal), otherwise (a zero
// row, an overflowing sum, a NaN) the row is kept as it is.
//
// 16-byte loads where src's base and dim allow, 16-byte stores where dst's base and dp_out
// allow, scalar otherwise; the ownership rule is the same either way.
void launch_unit_rows(const float* src, uint64_t n, uint32_t dim, uint32_t dp_out, float* dst, hipStream_t s);

// dist[i] = 1.0f + dist[i] where ids[i] != UINT64_MAX (one fp32 add; unfilled slots stay).
void launch_cos_finish(float* dist, const uint64_t* ids, uint64_t n, hipStream_t s);

}  // namespace vdbk
