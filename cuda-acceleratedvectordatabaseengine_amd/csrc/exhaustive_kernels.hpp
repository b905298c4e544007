// exhaustive_kernels.hpp — launchers of the kernels behind vdb_ivf_search_exhaustive
// (exhaustive_kernels.hip, gfx950, wave64): one pass over every stored row per tile of
// queries, in storage order, no coarse step, no pair plan, no per-list slots.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.hpp"

namespace vdbk {

constexpr uint32_t kExhWaves = 4;      // waves per scan workgroup
constexpr uint32_t kExhMaxTile = 32;   // queries per tile at k <= 64

// The sizing of a call, one function for the workspace and the launch. A wave keeps per query
// of the tile a list of 64 R entries in LDS (R = topk_regs(k): 1, 2, 4, 8, 16), 12 bytes each,
// so the tile shrinks as R grows and the lists always take 4 waves x 32 x 64 x 12 B = 96 KiB:
//   k      1..64  65..128  129..256  257..512  513..1024
//   R        1       2        4         8         16
//   tile    32      16        8         4          2
// 96 KiB leaves one workgroup per CU (160 KiB), so the persistent grid is one workgroup per CU.
struct ExhSizing {
    uint32_t regs = 0;   // R
    uint32_t tile = 0;   // TQ: queries per pass over the rows
    size_t lds = 0;      // dynamic LDS of a scan workgroup, bytes
};
inline ExhSizing exhaustive_sizing(uint32_t k) {
    ExhSizing z;
    z.regs = (uint32_t)topk_regs(k);
    z.tile = std::max(2u, kExhMaxTile / z.regs);
    z.lds = (size_t)kExhWaves * z.tile * 64 * z.regs * (sizeof(float) + sizeof(uint64_t));
    return z;
}

// valid[b] = stored rows of arena block b (0 for a block no list owns), from the list
// directory: list l owns blocks block_off[l] .. + cdiv(count[l], 64). nb bytes.
void launch_exh_block_valid(const uint64_t* block_off, const uint32_t* count, uint32_t nlist, uint64_t nb,
                            uint8_t* valid, hipStream_t s);

// The tile's queries as the scan reads them: qt[d][tile] = q[g][d] for g < nq, +0.0f for the
// tile's unused columns (q row-major [nq][dp], zero pads). Resets the scan's block cursor.
void launch_exh_stage(const float* q, uint32_t nq, uint32_t dp, uint32_t tile, float* qt, unsigned long long* cursor,
                      hipStream_t s);

struct ExhScanArgs {
    const float4* lists = nullptr;   // the interleaved arena, or the row-major rows (rows != 0)
    const uint64_t* ids = nullptr;   // [nb * 64]
    const uint8_t* valid = nullptr;  // [nb]
    const float* qt = nullptr;       // [dp][tile]
    unsigned long long* cursor = nullptr;  // next arena block nobody has taken
    uint64_t nb = 0;                 // arena blocks
    uint32_t d4 = 0, k = 0, nq = 0, chunk = 0;  // chunk: blocks a wave takes from the cursor at once
    uint32_t rows = 0;
    uint32_t lds = 0;                // dynamic LDS the launch gives (the kernel's own guard)
    float* part_d = nullptr;         // [grid][tile][k]: per (workgroup, query) the unique-id top-k
    uint64_t* part_i = nullptr;      //   of the rows its waves took, ascending, (+inf, no id) after
};
// grid workgroups of kExhWaves waves. metric: 0 L2, 1 IP, 2 Cosine (every distance 0.0f).
// Throws std::length_error if the sizing does not fit the CU's LDS.
void launch_exh_scan(int metric, const ExhScanArgs& a, uint32_t grid, hipStream_t s);

// One workgroup per query of the tile: the unique-id top-k of the grid's partials into
// out_d / out_i [nq][k], unfilled entries (FLT_MAX, UINT64_MAX).
void launch_exh_merge(const float* part_d, const uint64_t* part_i, uint32_t grid, uint32_t tile, uint32_t nq,
                      uint32_t k, float* out_d, uint64_t* out_i, hipStream_t s);

}  // namespace vdbk
