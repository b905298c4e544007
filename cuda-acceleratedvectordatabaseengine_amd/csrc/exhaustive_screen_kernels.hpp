// exhaustive_screen_kernels.hpp — launchers of the kernels behind
// vdb_ivf_search_exhaustive_screened (exhaustive_screen_kernels.hip, gfx950, wave64): two passes
// over the screen's shadow per tile of queries and one over the rows the bounds cannot discard.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace vdbk {

constexpr uint32_t kExsWaves = 4;   // waves per workgroup of the two shadow kernels and the select
constexpr uint32_t kExsTile = 32;   // queries per tile: two MFMA A operands
constexpr uint32_t kExsMaxK = 64;   // one WaveTopK register per list
// Dynamic LDS of a threshold workgroup: per wave the block's bounds [32][64] fp32 and the tile's
// lists [32][64] x (id, ub); of a bound workgroup: the bounds only.
constexpr size_t kExsTileLds = (size_t)kExsWaves * kExsTile * 64 * sizeof(float);
constexpr size_t kExsThreshLds = kExsTileLds + (size_t)kExsWaves * kExsTile * 64 * (sizeof(float) + sizeof(uint64_t));

// control words of a call (unsigned long long each)
constexpr int kExsCursorT = 0;  // next arena block of the threshold pass
constexpr int kExsCursorB = 1;  // ... of the bound pass
constexpr int kExsRows = 2;     // (query, stored row) pairs the bound pass judged, summed over the call
constexpr int kExsCtrlWords = 4;

struct ExhScreenArgs {
    // the handle's screen
    const uint4* shadow = nullptr;
    const float4* meta = nullptr;
    const float* sscale = nullptr;     // int8 only: selects the int8 kernels
    const uint32_t* blist = nullptr;   // the list of every arena block
    const uint8_t* valid = nullptr;    // stored rows of every arena block (launch_exh_block_valid)
    const uint64_t* ids = nullptr;     // [nb * 64]
    // the tile's pairs (launch_screen_pairs, identity probes): pair g * nlist + list
    const void* qres = nullptr;
    const float4* pst = nullptr;
    const float* qscale = nullptr;
    uint64_t nb = 0;
    uint32_t nlist = 0, dp = 0, k = 0, nq = 0, chunk = 0;
    uint32_t lds = 0;                  // dynamic LDS the launch gives (the kernel's own guard)
    unsigned long long* ctrl = nullptr;
    uint32_t* shared_thr = nullptr;    // [kExsTile] ord_enc of the tile's shared thresholds
    float* part_d = nullptr;           // threshold: [grid][kExsTile][k] unique partials
    uint64_t* part_i = nullptr;
    const float* thr = nullptr;        // bound: [nq][k] merged lists, T_q = thr[q * k + k - 1]
    uint32_t* cand = nullptr;          // bound: [kExsTile][cap] slots
    uint32_t* cnt = nullptr;           // bound: [nq] candidates counted (may exceed cap)
    uint64_t cap = 0;
};

// The identity probe table of a tile: probes[g * nlist + l] = l.
void launch_exs_probes(uint32_t* probes, uint32_t tile, uint32_t nlist, hipStream_t s);
// Before a tile's passes: both cursors to 0, the shared thresholds to +inf, cnt[0 .. nq) to 0.
void launch_exs_stage(unsigned long long* ctrl, uint32_t* shared_thr, uint32_t* cnt, uint32_t nq, hipStream_t s);
// grid workgroups of kExsWaves waves. metric: 0 L2, 1 IP. Both throw std::length_error when the
// launch's lists or tile do not fit the LDS given.
void launch_exs_thresh(int metric, const ExhScreenArgs& a, uint32_t grid, hipStream_t s);
void launch_exs_bound(int metric, const ExhScreenArgs& a, uint32_t grid, hipStream_t s);

struct ExhSelectArgs {
    const uint32_t* cand = nullptr;   // [nq][cap]
    const uint32_t* cnt = nullptr;    // [nq]
    uint64_t cap = 0;
    const float4* rows = nullptr;     // screen_rows: row-major fp32
    const uint64_t* ids = nullptr;
    const float* q = nullptr;         // the tile's padded queries [nq][4 d4]
    uint32_t d4 = 0, k = 0, nq = 0;
    float* out_d = nullptr;           // [nq][k]
    uint64_t* out_i = nullptr;
};
// One workgroup per query; a query whose count exceeds cap is left unwritten (its tile falls back).
void launch_exs_select(int metric, const ExhSelectArgs& a, hipStream_t s);

}  // namespace vdbk
