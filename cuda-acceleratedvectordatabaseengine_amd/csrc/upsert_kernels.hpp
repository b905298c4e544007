// upsert_kernels.hpp — launchers of the kernels that resolve a vdb_ivf_upsert request
// (upsert_kernels.hip, gfx950, wave64): which entries win, and the winners' rows and ids made
// dense in request order. The move itself is remove_kernels.hpp's compact and kernels.hpp's scatter.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vdbk {

// Stable radix sort (hipCUB, all 64 key bits) of the pairs (ids_in[i], pos_in[i]), i < n.
// temp == nullptr queries temp_bytes. The inputs are left as they are.
hipError_t upsert_sort_pairs(void* temp, size_t& temp_bytes, const uint64_t* ids_in, uint64_t* ids_out,
                             const uint32_t* pos_in, uint32_t* pos_out, uint32_t n, hipStream_t s);

// win[pos[j]] = 1 iff j == n - 1 or sorted_ids[j + 1] != sorted_ids[j], else 0, over the sorted
// pairs of a request whose positions were 0..n-1: every byte of win[0..n) is written.
void launch_upsert_winners(const uint64_t* sorted_ids, const uint32_t* pos, uint32_t n, uint8_t* win, hipStream_t s);

// Per 64 request entries: mask[g] bit i = win[g * 64 + i] (0 past n), cnt[g] = its bits set.
// cdiv(n, 64) words each.
void launch_upsert_ballot(const uint8_t* win, uint32_t n, unsigned long long* mask, uint32_t* cnt, hipStream_t s);

// Winner number base[g] + (bits of mask[g] below i) takes the raw row and the id of request
// entry g * 64 + i: out_rows [winners][dim], out_ids [winners]. base[g] is the exclusive sum of
// cnt[0..g). rows / out_rows need only float alignment.
void launch_upsert_pack(const float* rows, const uint64_t* ids, uint32_t n, uint32_t dim,
                        const unsigned long long* mask, const uint32_t* base, float* out_rows, uint64_t* out_ids,
                        hipStream_t s);

}  // namespace vdbk
