// screen_klist.hpp — what the threshold kernels of the screened filter searches share on the
// device (filter_screen_kernels.hip, multi_filter_screen_kernels.hip; gfx950, wave64): a wave's k
// smallest floats as one sorted float per lane, the wave-level LDS hand-over, and the persistent
// workgroups' item counter.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_common.hpp"
#include "wave_topk.hpp"

namespace vdbk {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- a wave's k smallest floats: one per lane, ascending, +inf where there is none ----------
template <int J>
__device__ __forceinline__ void cmpx_f(float& d, bool keep_min) {
    const float od = xor_f<J>(d);
    const bool take = keep_min ? od < d : d < od;
    d = take ? od : d;
}
__device__ __forceinline__ void sort64_f(float& d) {
    const int lane = lane_id();
    static_for<1, 7>([&](auto ks) {
        constexpr int KK = 1 << decltype(ks)::value;
        const bool asc = (lane & KK) == 0;
        static_for<0, decltype(ks)::value>([&](auto js) {
            constexpr int J = (KK >> 1) >> decltype(js)::value;
            cmpx_f<J>(d, ((lane & J) == 0) == asc);
        });
    });
}
// a and b ascending: a becomes the 64 smallest of both, ascending
__device__ __forceinline__ void merge64_f(float& a, float b) {
    const int lane = lane_id();
    const float r = shfl_f(b, 63 - lane);
    a = r < a ? r : a;
    static_for<0, 6>([&](auto js) {
        constexpr int J = 32 >> decltype(js)::value;
        cmpx_f<J>(a, (lane & J) == 0);
    });
}
// a wave-uniform c below the list's last element
__device__ __forceinline__ void insert_f(float& d, float c) {
    const int lane = lane_id();
    const int pos = __popcll(__ballot(d < c));
    const float up = __uint_as_float(up1_u32(__float_as_uint(d), 0u));
    d = lane > pos ? up : (lane == pos ? c : d);
}

// The workgroup's next item from the device counter ctrl[word] (the same in every wave).
__device__ __forceinline__ uint32_t next_item(unsigned long long* ctrl, int word, uint32_t* s_item) {
    if (threadIdx.x == 0) *s_item = (uint32_t)atomicAdd(ctrl + word, 1ull);
    __syncthreads();
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)*s_item);
    __syncthreads();  // (read by all before thread 0 writes the next)
    return item;
}

}  // namespace vdbk
