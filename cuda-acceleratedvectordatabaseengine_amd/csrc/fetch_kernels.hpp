// fetch_kernels.hpp — launchers of the kernels behind vdb_ivf_fetch_ids and vdb_ivf_search_ids
// (fetch_kernels.hip, gfx950, wave64): the reverse map from a requested id to the arena slot
// that stores it, and the gather of the rows from either fp32 layout of the lists. The sort
// of the request is prepared_kernels.hpp's launch_filter_sort.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vdbk {

constexpr unsigned long long kFetchNone = ~0ull;  // loc[j] of a requested id no stored row carries

// loc[j] = min(loc[j], b * 64 + i) for every slot i < valid[b] of every arena block b whose id
// equals sorted[j], j the FIRST entry of the run of equal ids in sorted[0..n) (ascending,
// repeats allowed). loc is preset to kFetchNone by the caller. Arena blocks ascend with the
// list id and slots with the add order, so the smallest slot is the row at the lowest (list,
// position). Reads the ids of slots below valid[b] only (8 bytes per stored row).
void launch_fetch_locate(const uint64_t* arena_ids, const uint32_t* valid, uint64_t nblocks, const uint64_t* sorted,
                         uint32_t n, unsigned long long* loc, hipStream_t s);

// One wave per request entry i < n: its id's first entry j in sorted, then loc[j].
//   found (may be null): found[i] = 1 if a row carries req[i], else 0.
//   out (may be null): row dst[i] of out ([..][dim] floats, dense; dst == null: row i) takes the
//   stored row's dim floats, or dim zeros when there is none; an entry with dst[i] == UINT32_MAX
//   writes no row. Never a float past dim.
//   n_found (may be null; device): grows by the entries found.
// lists: rows == 0 the interleaved arena [block][d4][64] float4, rows != 0 the row-major copy
// in slot order with stride 4 * d4 floats. Only rows that loc names are read.
void launch_fetch_gather(const float4* lists, int rows, uint32_t d4, uint32_t dim, const uint64_t* req, uint32_t n,
                         const uint64_t* sorted, const unsigned long long* loc, const uint32_t* dst, float* out,
                         uint8_t* found, unsigned long long* n_found, hipStream_t s);

}  // namespace vdbk
