// remove_kernels.hpp — launchers of the two kernels behind vdb_ivf_remove_ids
// (remove_kernels.hip, gfx950, wave64: one wavefront per 64-slot arena block).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vdbk {

// keepmask[b] bit i = slot i of block b holds a row (i < valid[b]) whose id is not one of
// sorted[0..n) (ascending; repeats do no harm, the lookup is a lower bound: remove passes each
// id once, upsert the whole request as sorted). Reads the ids only (8 bytes per slot).
void launch_remove_mark(const uint64_t* arena_ids, const uint32_t* valid, uint64_t nblocks, const uint64_t* sorted,
                        uint32_t n, unsigned long long* keepmask, hipStream_t s);

// Every kept slot of the old arena ([block][d4][64] float4, ids beside it) into the fresh
// one: the j-th kept slot of block b goes to arena slot base[b] + j. The fresh arena is
// zeroed (ids 0xFF) by the caller; nothing else is written.
void launch_remove_compact(const float4* old_arena, const uint64_t* old_ids, const unsigned long long* keepmask,
                           const uint64_t* base, uint64_t nblocks, uint32_t d4, float4* new_arena, uint64_t* new_ids,
                           hipStream_t s);

}  // namespace vdbk
