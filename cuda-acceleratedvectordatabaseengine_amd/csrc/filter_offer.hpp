// filter_offer.hpp — what the merges of filter_kernels.hip and multi_filter_kernels.hip share
// on the device (gfx950, wave64).
#pragma once

#include "wave_topk.hpp"

namespace vdbk {

// Offer a slot list's k entries to a de-duplicating list (merge_results): ids == UINT64_MAX
// are not results.
__device__ __forceinline__ void offer_slot_unique(WaveTopK<1>& tk, const float* __restrict__ sd,
                                                  const uint64_t* __restrict__ si, uint32_t k, float& kd,
                                                  uint64_t& ki) {
    const uint32_t c = (uint32_t)lane_id();
    const bool valid = c < k;
    const float d = valid ? sd[c] : __builtin_inff();
    const uint64_t id = valid ? si[c] : kNoId;
    uint64_t mask = __ballot(valid && id != kNoId && d <= kd);
    while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        tk.offer_unique(rd_lane(d, l), rd_lane(id, l), (int)k, kd, ki);
    }
}

}  // namespace vdbk
