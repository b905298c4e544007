// multi_filter_kernels.hip — device side of vdb_ivf_search_prepared_multi (gfx950, wave64): the
// masked exact scan of filter_kernels.hip for a batch whose queries each name their own
// prepared filter.
//
// The host hands over allow_tab[F] (per filter the address of its per-block allow masks),
// allowed_tab[F] (per filter the address of its per-list allowed counts) and qf[B], the filter
// of every query of the batch, ascending (multi_filter_plan.hpp).
//   ivf_pair_gate           gate[pair] = the rows the pair's own filter allows in the pair's list.
//   ivf_filter_scan_multi   ivf_filter_scan's item loop, LDS fold and output layout; the items
//                           come from the grouping gated per pair (launch_scan_group_pairs). Per
//                           block the wave reads the masks of the item's (up to 4) queries, 8
//                           bytes each at wave-uniform addresses, and skips the block unread
//                           when their union is zero. Row-major layout: only the union's lanes
//                           load their rows; interleaved layout: the wave reads the block. The
//                           distance chains are ivf_filter_scan's (acc4, dist_finish, the same
//                           order), and lane l offers its row to query g only if bit l of query
//                           g's own mask is set: the union decides what is read, never what a
//                           query may see.
//   ivf_filter_fold_multi   ivf_filter_fold with gate[pair] for allowed[list].
//   ivf_filter_merge_multi  ivf_filter_merge with gate[pair], the stale walk-back over the
//                           earlier queries of the same filter only;
//   ivf_filter_carry_multi  the slot content of the batch's last filter that survives into the
//                           call's next batch.
// The promise of filter_kernels.hip holds here too: no kernel reads a block, an id or a slot
// list it was not given, nothing is prefetched beyond a segment, and the arena's slack block is
// never touched.
#pragma clang fp contract(off)
#include "multi_filter_kernels.hpp"

#include <algorithm>
#include <cfloat>

#include "filter_offer.hpp"
#include "scan_common.hpp"
#include "wave_topk.hpp"

namespace vdbk {
namespace {

constexpr uint32_t kWaves = 4;  // wavefronts per workgroup

__global__ void ivf_pair_gate(const uint32_t* __restrict__ probes, const uint32_t* __restrict__ qf,
                              const uint32_t* const* __restrict__ allowed_tab, uint32_t BP, uint32_t P,
                              uint32_t* __restrict__ gate) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BP) return;
    gate[i] = allowed_tab[qf[i / P]][probes[i]];
}

template <int M, bool ROWS>
__global__ __launch_bounds__(kWaves * 64) void ivf_filter_scan_multi(const MultiFilterScanArgs a) {
    constexpr int G = (int)kFilterGroup;
    static_assert(kFilterGroup <= kWaves, "one wave folds one query of the group");
    __shared__ float s_d[kWaves][G][64];
    __shared__ uint64_t s_i[kWaves][G][64];
    const int lane = lane_id();
    const uint32_t wave = wave_index();
    const uint32_t d4 = a.d4;
    const int k = (int)a.k;
    const uint32_t total = a.item_start[a.nlist];
    for (uint32_t item = blockIdx.x; item < total; item += gridDim.x) {  // (the same in every wave)
        const ExactScanItem it = decode_scan_item<kFilterGroup>(item, a.item_start, a.pair_start, a.count, a.nlist, a.segs);
        const uint32_t seg = it.seg, p0 = it.p0, b_lo = it.b_lo, b_hi = it.b_hi;
        const int np = (int)it.np;  // >= 1; slots g >= np repeat the last query
        const uint64_t base = a.block_off[it.list];
        const float4* __restrict__ q4[G];                // (wave-uniform reads)
        const unsigned long long* __restrict__ am[G];    // query g's masks of this list's blocks
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t q = a.inv[p0 + (g < np ? g : np - 1)] / a.P;
            q4[g] = (const float4*)(a.q + (size_t)q * d4 * 4);
            am[g] = a.allow_tab[a.qf[q]] + base;
        }

        WaveTopK<1> tk[G];
        float kd[G];
        uint64_t ki[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            tk[g].init();
            kd[g] = __builtin_inff();
            ki[g] = kNoId;
        }
        for (uint32_t b = b_lo + wave; b < b_hi; b += kWaves) {
            const uint64_t gb = base + b;
            unsigned long long m[G], u = 0;
#pragma unroll
            for (int g = 0; g < G; ++g) {  // (slots g >= np repeat a mask the union already holds)
                m[g] = am[g][b];
                u |= m[g];
            }
            if (u == 0) continue;  // no row byte of this block is read
            const bool mine = (u >> lane) & 1ull;
            float acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.0f;
            if constexpr (M != kCos) {
                if constexpr (ROWS) {
                    if (mine) {
                        const float4* __restrict__ p = a.lists + (gb * 64 + (uint64_t)lane) * d4;
#pragma unroll 8
                        for (uint32_t t = 0; t < d4; ++t) {
                            const float4 x = p[t];
#pragma unroll
                            for (int g = 0; g < G; ++g) acc[g] = acc4<M>(acc[g], q4[g][t], x);
                        }
                    }
                } else {
                    const float4* __restrict__ p = a.lists + gb * d4 * 64 + lane;
#pragma unroll 8
                    for (uint32_t t = 0; t < d4; ++t) {
                        const float4 x = load_nt(p + (size_t)t * 64);
#pragma unroll
                        for (int g = 0; g < G; ++g) acc[g] = acc4<M>(acc[g], q4[g][t], x);
                    }
                }
            }
            const uint64_t id = mine ? a.ids[gb * 64 + lane] : kNoId;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g < np) {
                    const bool own = (m[g] >> lane) & 1ull;  // the query's own filter allows the row
                    const float dv = dist_finish<M>(acc[g]);
                    offer_lanes<1>(tk[g], own && dv <= kd[g], dv, id, k, kd[g], ki[g]);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            s_d[wave][g][lane] = tk[g].d[0];
            s_i[wave][g][lane] = tk[g].id[0];
        }
        __syncthreads();
        if ((int)wave < np) {  // wave g folds the four waves' lists of the group's query g
            WaveTopK<1> f;
            f.d[0] = s_d[0][wave][lane];
            f.id[0] = s_i[0][wave][lane];
            float fkd;
            uint64_t fki;
            f.at(k - 1, fkd, fki);
            for (uint32_t w = 1; w < kWaves; ++w) {
                const float dv = s_d[w][wave][lane];
                const uint64_t iv = s_i[w][wave][lane];
                offer_lanes<1>(f, dv <= fkd, dv, iv, k, fkd, fki);
            }
            if (lane < k) {
                const size_t o = ((size_t)a.inv[p0 + wave] * a.segs + seg) * k + lane;
                a.part_d[o] = f.d[0];
                a.part_i[o] = f.id[0];
            }
        }
        __syncthreads();  // (the lists in LDS are read before the next item's are written)
    }
}

__global__ __launch_bounds__(kWaves * 64) void ivf_filter_fold_multi(const float* __restrict__ part_d,
                                                                      const uint64_t* __restrict__ part_i,
                                                                      const uint32_t* __restrict__ probes,
                                                                      const uint32_t* __restrict__ gate,
                                                                      const uint32_t* __restrict__ count,
                                                                      uint32_t BP, uint32_t segs, uint32_t k,
                                                                      float* __restrict__ slot_d,
                                                                      uint64_t* __restrict__ slot_i) {
    const uint32_t i = blockIdx.x * kWaves + wave_index();
    if (i >= BP) return;
    if (gate[i] == 0) return;  // (the scan wrote no partial)
    const uint32_t list = probes[i];
    const int lane = lane_id();
    WaveTopK<1> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    const uint32_t n = scan_segs((count[list] + 63) >> 6, segs) * k;  // the list's segments are the pair's first
    const size_t base = (size_t)i * segs * k;
    for (uint32_t e0 = 0; e0 < n; e0 += 64) {
        const uint32_t e = e0 + lane;
        const bool v = e < n;
        const float dv = v ? part_d[base + e] : __builtin_inff();
        const uint64_t iv = v ? part_i[base + e] : kNoId;
        offer_lanes<1>(tk, v && dv <= kd, dv, iv, (int)k, kd, ki);
    }
    if ((uint32_t)lane < k) {
        slot_d[(size_t)i * k + lane] = tk.d[0];
        slot_i[(size_t)i * k + lane] = tk.id[0];
    }
}

__global__ __launch_bounds__(kWaves * 64) void ivf_filter_merge_multi(const uint32_t* __restrict__ gate,
                                                                       const uint32_t* __restrict__ qf,
                                                                       const float* __restrict__ slot_d,
                                                                       const uint64_t* __restrict__ slot_i,
                                                                       const float* __restrict__ carry_d,
                                                                       const uint64_t* __restrict__ carry_i,
                                                                       int carry_same, uint32_t B, uint32_t P,
                                                                       uint32_t k, int stale,
                                                                       float* __restrict__ out_d,
                                                                       uint64_t* __restrict__ out_i,
                                                                       unsigned long long* __restrict__ pairs) {
    const uint32_t q = blockIdx.x * kWaves + wave_index();
    if (q >= B) return;
    const int lane = lane_id();
    const uint32_t f = qf[q];
    WaveTopK<1> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    unsigned long long rows = 0;  // this lane's share of the rows the query's filter allows in its lists
    for (uint32_t p = lane; p < P; p += 64) rows += gate[(size_t)q * P + p];
    for (uint32_t p = 0; p < P; ++p) {
        const float* sd = nullptr;
        const uint64_t* si = nullptr;
        if (gate[(size_t)q * P + p] > 0) {
            sd = slot_d + ((size_t)q * P + p) * k;
            si = slot_i + ((size_t)q * P + p) * k;
        } else if (stale) {
            uint32_t q2 = q;
            bool found = false;
            while (q2 > 0 && qf[q2 - 1] == f) {  // the earlier queries of the same filter only
                --q2;
                if (gate[(size_t)q2 * P + p] > 0) {
                    found = true;
                    break;
                }
            }
            if (found) {
                sd = slot_d + ((size_t)q2 * P + p) * k;
                si = slot_i + ((size_t)q2 * P + p) * k;
            } else if (q2 == 0 && carry_same) {  // an earlier batch, same filter (ids UINT64_MAX where there is none)
                sd = carry_d + (size_t)p * k;
                si = carry_i + (size_t)p * k;
            }
        }
        if (sd) offer_slot_unique(tk, sd, si, k, kd, ki);
    }
    if ((uint32_t)lane < k) {
        const bool real = tk.id[0] != kNoId;
        out_d[(size_t)q * k + lane] = real ? tk.d[0] : FLT_MAX;
        out_i[(size_t)q * k + lane] = tk.id[0];
    }
    if (rows) atomicAdd(pairs, rows);
}

__global__ void ivf_filter_carry_multi(const uint32_t* __restrict__ gate, const uint32_t* __restrict__ qf,
                                       int carry_same, uint32_t B, uint32_t P, uint32_t k,
                                       const float* __restrict__ slot_d, const uint64_t* __restrict__ slot_i,
                                       float* __restrict__ carry_d, uint64_t* __restrict__ carry_i) {
    __shared__ int s_q;  // >= 0: that query's slot; -1: the carry keeps what it has; -2: it holds nothing
    const uint32_t p = blockIdx.x;
    if (threadIdx.x == 0) {
        const uint32_t f = qf[B - 1];
        int found = -2;
        int q = (int)B - 1;
        for (; q >= 0 && qf[q] == f; --q)
            if (gate[(size_t)q * P + p] > 0) {
                found = q;
                break;
            }
        if (found < 0 && q < 0 && carry_same) found = -1;  // the run is the whole batch, the carry its filter's
        s_q = found;
    }
    __syncthreads();
    if (s_q == -1) return;
    if (s_q == -2) {
        for (uint32_t e = threadIdx.x; e < k; e += blockDim.x) carry_i[(size_t)p * k + e] = kNoId;
        return;
    }
    const size_t src = ((size_t)s_q * P + p) * k;
    for (uint32_t e = threadIdx.x; e < k; e += blockDim.x) {
        carry_d[(size_t)p * k + e] = slot_d[src + e];
        carry_i[(size_t)p * k + e] = slot_i[src + e];
    }
}

template <int M>
void scan_metric(const MultiFilterScanArgs& a, hipStream_t s) {
    // persistent over the items (their number is known on the device only): 8 workgroups per CU at most
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)a.B * a.P * a.segs, 256 * 8);
    if (a.rows) ivf_filter_scan_multi<M, true><<<grid, kWaves * 64, 0, s>>>(a);
    else ivf_filter_scan_multi<M, false><<<grid, kWaves * 64, 0, s>>>(a);
}

}  // namespace

void launch_pair_gate(const uint32_t* probes, const uint32_t* qf, const uint32_t* const* allowed_tab, uint32_t B,
                      uint32_t P, uint32_t* gate, hipStream_t s) {
    const uint32_t BP = B * P;
    if (!BP) return;
    ivf_pair_gate<<<(BP + 255) / 256, 256, 0, s>>>(probes, qf, allowed_tab, BP, P, gate);
}

void launch_filter_scan_multi(int metric, const MultiFilterScanArgs& a, hipStream_t s) {
    if (!a.B || !a.P) return;
    if (metric == kL2) scan_metric<kL2>(a, s);
    else if (metric == kIP) scan_metric<kIP>(a, s);
    else scan_metric<kCos>(a, s);
}

void launch_filter_fold_multi(const float* part_d, const uint64_t* part_i, const uint32_t* probes,
                              const uint32_t* gate, const uint32_t* count, uint32_t BP, uint32_t segs, uint32_t k,
                              float* slot_d, uint64_t* slot_i, hipStream_t s) {
    if (!BP) return;
    ivf_filter_fold_multi<<<(BP + kWaves - 1) / kWaves, kWaves * 64, 0, s>>>(part_d, part_i, probes, gate, count, BP,
                                                                          segs, k, slot_d, slot_i);
}

void launch_filter_merge_multi(const uint32_t* gate, const uint32_t* qf, const float* slot_d, const uint64_t* slot_i,
                               float* carry_d, uint64_t* carry_i, int carry_same, uint32_t B, uint32_t P, uint32_t k,
                               int stale, float* out_d, uint64_t* out_i, unsigned long long* pairs, hipStream_t s) {
    if (!B) return;
    ivf_filter_merge_multi<<<(B + kWaves - 1) / kWaves, kWaves * 64, 0, s>>>(
        gate, qf, slot_d, slot_i, carry_d, carry_i, carry_same, B, P, k, stale, out_d, out_i, pairs);
    if (stale) ivf_filter_carry_multi<<<P, 64, 0, s>>>(gate, qf, carry_same, B, P, k, slot_d, slot_i, carry_d, carry_i);
}

}  // namespace vdbk
