// prepared_kernels.hip — device side of the prepared filters (gfx950, wave64).
//   filter sort          hipcub's radix sort of the filter's ids, all 64 key bits, on the
//                        handle's stream: what the one-shot call does on the host.
//   ivf_filter_combine   one pass over the arena's blocks: a word of each input in, a word out.
//                        Grid-stride, one thread per block word; ivf_filter_count follows it.
#include "prepared_kernels.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace vdbk {
namespace {

template <int OP>
__global__ __launch_bounds__(256) void ivf_filter_combine(const unsigned long long* __restrict__ a,
                                                          const unsigned long long* __restrict__ b, uint64_t nblocks,
                                                          unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks; i += stride) {
        const unsigned long long x = a[i], y = b[i];
        out[i] = OP == 0 ? (x & y) : OP == 1 ? (x | y) : (x & ~y);
    }
}

}  // namespace

hipError_t filter_sort_temp_bytes(uint32_t n, size_t& bytes) {
    const uint64_t* in = nullptr;
    uint64_t* out = nullptr;
    bytes = 0;
    return hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, in, out, (int)n, 0, 64, nullptr);
}

hipError_t launch_filter_sort(void* temp, size_t temp_bytes, const uint64_t* in, uint64_t* out, uint32_t n,
                              hipStream_t s) {
    if (!n) return hipSuccess;
    return hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, in, out, (int)n, 0, 64, s);
}

void launch_filter_combine(const unsigned long long* a, const unsigned long long* b, uint64_t nblocks, int op,
                           unsigned long long* out, hipStream_t s) {
    if (!nblocks) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nblocks + 255) / 256, 256 * 8);
    if (op == 0) ivf_filter_combine<0><<<grid, 256, 0, s>>>(a, b, nblocks, out);
    else if (op == 1) ivf_filter_combine<1><<<grid, 256, 0, s>>>(a, b, nblocks, out);
    else ivf_filter_combine<2><<<grid, 256, 0, s>>>(a, b, nblocks, out);
}

}  // namespace vdbk
