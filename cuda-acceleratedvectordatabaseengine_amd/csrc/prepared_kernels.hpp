// prepared_kernels.hpp — launchers of the kernels behind the prepared filters
// (prepared_kernels.hip, gfx950, wave64): the device sort of a filter's ids and the combination
// of two filters' masks. The marking itself is filter_kernels.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vdbk {

// Bytes of scratch launch_filter_sort needs for n ids.
hipError_t filter_sort_temp_bytes(uint32_t n, size_t& bytes);
// out[0..n) = in[0..n) ascending (repeats stay: ivf_filter_mark's binary search does not mind).
// `in` is left as it is.
hipError_t launch_filter_sort(void* temp, size_t temp_bytes, const uint64_t* in, uint64_t* out, uint32_t n,
                              hipStream_t s);

// out[b] = a[b] & b[b] (op 0), a[b] | b[b] (op 1) or a[b] & ~b[b] (op 2) for the nblocks arena
// blocks. None of the three sets a bit that neither input has, so a mask keeps no bit at or
// above its block's valid count. out may be neither input.
void launch_filter_combine(const unsigned long long* a, const unsigned long long* b, uint64_t nblocks, int op,
                           unsigned long long* out, hipStream_t s);

}  // namespace vdbk
