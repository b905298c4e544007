// wave_topk_test — the wave64 top-k primitives of csrc/wave_topk.hpp, alone, against a plain
// host reference, for every register count R = 1, 2, 4, 8, 16.
//
// The contract checked is the one the header's first comment block states: a candidate is the
// pair (dist, id) ordered like std::pair (smaller dist first, ties by smaller id; -0.0f and
// +0.0f are one distance); a wave keeps the k best in element order e = r * 64 + lane,
// ascending; unused elements hold (+inf, UINT64_MAX). The reference below is std::stable_sort
// and std::map over such pairs and shares no code with the header.
//
// One wave (a 64-thread block) serves one case; every driver launches all its cases of one R
// as one grid. A case reads a stream of 64-wide steps of (dist, id, valid) slots and a
// capacity k from device memory and writes its 64 * R list elements (and its running k-th
// key) back; the host compares ids and distance bits of the elements below k. Nothing is
// printed or asserted on the device.
//
// Exit status 0 and a last line "mismatches: 0" mean every case agreed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "wave_topk.hpp"

using namespace vdbk;

#define HIPCHECK(x)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                              \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(2);                                                                    \
        }                                                                                    \
    } while (0)

// ---- device side ------------------------------------------------------------------------
struct Case {
    uint32_t off;     // first slot of the stream (a multiple of 64)
    uint32_t nslots;  // slots of the stream (a multiple of 64)
    uint32_t k;       // list capacity
    uint32_t aux;     // remove: the element to remove
    uint32_t out;     // first output element of the case
};

__device__ __forceinline__ Case load_case(const Case* cases) {
    Case c = cases[blockIdx.x];
    c.off = __builtin_amdgcn_readfirstlane(c.off);
    c.nslots = __builtin_amdgcn_readfirstlane(c.nslots);
    c.k = __builtin_amdgcn_readfirstlane(c.k);
    c.aux = __builtin_amdgcn_readfirstlane(c.aux);
    c.out = __builtin_amdgcn_readfirstlane(c.out);
    return c;
}

template <int R>
__device__ __forceinline__ void store_list(const WaveTopK<R>& tk, uint32_t out, float* od, uint64_t* oi) {
    const int lane = lane_id();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        od[out + r * 64 + lane] = tk.d[r];
        oi[out + r * 64 + lane] = tk.id[r];
    }
}

template <int R>
__device__ __forceinline__ void load_list(WaveTopK<R>& tk, uint32_t off, const float* sd, const uint64_t* si) {
    const int lane = lane_id();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        tk.d[r] = sd[off + r * 64 + lane];
        tk.id[r] = si[off + r * 64 + lane];
    }
}

// Multiset top-k, driven as the scans drive it: 64 candidates a step, want = valid && d <= kd.
// Output: 64 R elements, then (kd, ki).
template <int R>
__global__ __launch_bounds__(64) void run_multiset(const Case* __restrict__ cases, const float* __restrict__ sd,
                                                   const uint64_t* __restrict__ si, const uint8_t* __restrict__ sv,
                                                   float* __restrict__ od, uint64_t* __restrict__ oi) {
    const Case c = load_case(cases);
    const int lane = lane_id();
    WaveTopK<R> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    for (uint32_t s = 0; s < c.nslots; s += 64) {
        const uint32_t e = c.off + s + lane;
        const float d = sd[e];
        const uint64_t id = si[e];
        const bool valid = sv[e] != 0;
        offer_lanes<R>(tk, valid && d <= kd, d, id, (int)c.k, kd, ki);
    }
    store_list<R>(tk, c.out, od, oi);
    if (lane == 0) {
        od[c.out + 64 * R] = kd;
        oi[c.out + 64 * R] = ki;
    }
}

// Unique-id top-k, driven as the merges drive it: ballot, then one wave-uniform offer per set
// lane, entries without an id skipped.
template <int R>
__global__ __launch_bounds__(64) void run_unique(const Case* __restrict__ cases, const float* __restrict__ sd,
                                                 const uint64_t* __restrict__ si, const uint8_t* __restrict__ sv,
                                                 float* __restrict__ od, uint64_t* __restrict__ oi) {
    const Case c = load_case(cases);
    const int lane = lane_id();
    WaveTopK<R> tk;
    tk.init();
    float kd = __builtin_inff();
    uint64_t ki = kNoId;
    for (uint32_t s = 0; s < c.nslots; s += 64) {
        const uint32_t e = c.off + s + lane;
        const float d = sd[e];
        const uint64_t id = si[e];
        const bool valid = sv[e] != 0;
        uint64_t mask = __ballot(valid && id != kNoId && d <= kd);
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            tk.offer_unique(rd_lane(d, l), rd_lane(id, l), (int)c.k, kd, ki);
        }
    }
    store_list<R>(tk, c.out, od, oi);
    if (lane == 0) {
        od[c.out + 64 * R] = kd;
        oi[c.out + 64 * R] = ki;
    }
}

// remove(aux) on a list loaded as it stands. Output: 64 R elements.
template <int R>
__global__ __launch_bounds__(64) void run_remove(const Case* __restrict__ cases, const float* __restrict__ sd,
                                                 const uint64_t* __restrict__ si, float* __restrict__ od,
                                                 uint64_t* __restrict__ oi) {
    const Case c = load_case(cases);
    WaveTopK<R> tk;
    load_list<R>(tk, c.off, sd, si);
    tk.remove((int)c.aux);
    store_list<R>(tk, c.out, od, oi);
}

// at(e) for every e of a list loaded as it stands. Output: 64 R elements as at() gave them.
template <int R>
__global__ __launch_bounds__(64) void run_at(const Case* __restrict__ cases, const float* __restrict__ sd,
                                             const uint64_t* __restrict__ si, float* __restrict__ od,
                                             uint64_t* __restrict__ oi) {
    const Case c = load_case(cases);
    const int lane = lane_id();
    WaveTopK<R> tk;
    load_list<R>(tk, c.off, sd, si);
    for (int e = 0; e < 64 * R; ++e) {
        float d;
        uint64_t id;
        tk.at(e, d, id);
        if (lane == 0) {
            od[c.out + e] = d;
            oi[c.out + e] = id;
        }
    }
}

// bitonic_sort64 of one step. Output: 64 elements.
__global__ __launch_bounds__(64) void run_sort(const Case* __restrict__ cases, const float* __restrict__ sd,
                                               const uint64_t* __restrict__ si, float* __restrict__ od,
                                               uint64_t* __restrict__ oi) {
    const Case c = load_case(cases);
    const int lane = lane_id();
    float d = sd[c.off + lane];
    uint64_t id = si[c.off + lane];
    bitonic_sort64(d, id);
    od[c.out + lane] = d;
    oi[c.out + lane] = id;
}

// bitonic_merge64 of a sorted list (first step) with a sorted batch (second step). Output: 64.
__global__ __launch_bounds__(64) void run_merge(const Case* __restrict__ cases, const float* __restrict__ sd,
                                                const uint64_t* __restrict__ si, float* __restrict__ od,
                                                uint64_t* __restrict__ oi) {
    const Case c = load_case(cases);
    const int lane = lane_id();
    float ad = sd[c.off + lane];
    uint64_t ai = si[c.off + lane];
    bitonic_merge64(ad, ai, sd[c.off + 64 + lane], si[c.off + 64 + lane]);
    od[c.out + lane] = ad;
    oi[c.out + lane] = ai;
}

// The lane exchanges: block b reads in[b][64] and writes out[b][8][64]:
// xor 1, 2, 4, 8, 16, 32, then up1 and down1 with the fill value in[b][lane 0] ^ 0xA5A5A5A5.
constexpr int kLaneOps = 8;
__global__ __launch_bounds__(64) void run_lane_ops(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const int lane = lane_id();
    const uint32_t v = in[blockIdx.x * 64 + lane];
    const uint32_t fill = rd_lane_u32(v, 0) ^ 0xA5A5A5A5u;
    uint32_t* o = out + (size_t)blockIdx.x * kLaneOps * 64;
    o[0 * 64 + lane] = xor_u32<1>(v);
    o[1 * 64 + lane] = xor_u32<2>(v);
    o[2 * 64 + lane] = xor_u32<4>(v);
    o[3 * 64 + lane] = xor_u32<8>(v);
    o[4 * 64 + lane] = xor_u32<16>(v);
    o[5 * 64 + lane] = xor_u32<32>(v);
    o[6 * 64 + lane] = up1_u32(v, fill);
    o[7 * 64 + lane] = down1_u32(v, fill);
}

// ---- host side: streams -------------------------------------------------------------------
static const uint64_t NOID = ~0ull;
static const float INF = std::numeric_limits<float>::infinity();

struct Cand {
    float d;
    uint64_t id;
    bool valid;
};
typedef std::pair<float, uint64_t> Key;

static uint32_t fbits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float bits_f(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// The order of the header's first comment block, written as std::pair's operator< is.
static bool key_before(const Key& a, const Key& b) { return a.first < b.first || (!(b.first < a.first) && a.second < b.second); }

struct Stream {
    std::string name;
    uint32_t off = 0, nslots = 0;
    std::vector<Cand> c;  // the slots, a whole number of 64-wide steps
};

// All streams in one device image.
static std::vector<float> g_sd;
static std::vector<uint64_t> g_si;
static std::vector<uint8_t> g_sv;
static std::vector<Stream> g_streams;

static int add_stream(const std::string& name, std::vector<Cand> c) {
    while (c.size() % 64) c.push_back(Cand{INF, NOID, false});
    if (c.empty()) c.assign(64, Cand{INF, NOID, false});
    Stream s;
    s.name = name;
    s.off = (uint32_t)g_sd.size();
    s.nslots = (uint32_t)c.size();
    for (const Cand& x : c) {
        g_sd.push_back(x.d);
        g_si.push_back(x.id);
        g_sv.push_back(x.valid ? 1 : 0);
    }
    s.c = std::move(c);
    g_streams.push_back(std::move(s));
    return (int)g_streams.size() - 1;
}

static const float kTie8[8] = {-2.0f, -0.5f, 0.25f, 0.25000003f, 1.0f, 3.0f, 1.0e10f, 1.0e-3f};
// -0 and +0 (one distance), subnormals, the largest finite value, real candidates at +inf,
// the smallest normal, negative distances (inner product).
static const uint32_t kSpecialBits[] = {0x80000000u, 0x00000000u, 0x00000001u, 0x00000002u, 0x007FFFFFu, 0x80000001u,
                                        0x7F7FFFFFu, 0x7F800000u, 0x00800000u, 0xFF7FFFFFu, 0xBFC00000u, 0x3F800000u};
constexpr int kNSpecial = (int)(sizeof(kSpecialBits) / sizeof(kSpecialBits[0]));

static uint64_t random_id(std::mt19937_64& g) {
    uint64_t v = g();
    switch (g() % 4) {
        case 0: v &= 0xFFFFull; break;                               // small
        case 1: v = (v & 0x3FFull) | ((g() % 5) << 32); break;       // equal low words, differing high words
        case 2: v |= 1ull << 63; break;                              // the top bit set
        default: break;
    }
    return v == NOID ? 12345 : v;
}

// n distinct ids in a random order, with equal low words among them.
static std::vector<uint64_t> distinct_ids(std::mt19937_64& g, size_t n) {
    std::vector<uint64_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = ((uint64_t)(i % 3) << 32) | ((uint64_t)(i % 7 == 0) << 63) | (i / 3 * 5 + 1);
    std::shuffle(v.begin(), v.end(), g);
    return v;
}

static const int kSizes[] = {1, 63, 64, 65, 1000, 4096};

static std::vector<int> g_multiset_streams;

static void build_multiset_streams() {
    std::mt19937_64 g(20241);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    for (int n : kSizes) {
        const std::string sn = " n=" + std::to_string(n);
        std::vector<Cand> c(n);
        // ascending in (d, id), with runs of one distance: nothing is inserted after the first k
        for (int i = 0; i < n; ++i) c[i] = Cand{(float)(i / 3) * 0.5f - 100.0f, (uint64_t)i * 3 + (1ull << 34), true};
        g_multiset_streams.push_back(add_stream("ascending" + sn, c));
        // strictly descending: every candidate lands at element 0
        for (int i = 0; i < n; ++i) c[i] = Cand{(float)(n - i) * 0.5f, random_id(g), true};
        g_multiset_streams.push_back(add_stream("descending" + sn, c));
        // one distance, ids descending: the order is by id alone
        for (int i = 0; i < n; ++i) c[i] = Cand{1.25f, (uint64_t)(n - i) * 7 + (1ull << 33), true};
        g_multiset_streams.push_back(add_stream("one-distance" + sn, c));
        // 8 distances, ids from a small set: heavy ties and repeated (d, id) pairs
        for (int i = 0; i < n; ++i)
            c[i] = Cand{kTie8[g() % 8], ((uint64_t)(g() % 3) << 32) | (g() % 2000), true};
        g_multiset_streams.push_back(add_stream("ties8" + sn, c));
        for (int i = 0; i < n; ++i) c[i] = Cand{nd(g), random_id(g), true};
        g_multiset_streams.push_back(add_stream("normal" + sn, c));
        // special values alone and mixed into a random stream; distinct ids, so that -0 and +0
        // of one id never meet
        std::vector<uint64_t> ids = distinct_ids(g, n);
        for (int i = 0; i < n; ++i) c[i] = Cand{bits_f(kSpecialBits[g() % kNSpecial]), ids[i], true};
        g_multiset_streams.push_back(add_stream("special" + sn, c));
        ids = distinct_ids(g, n);
        for (int i = 0; i < n; ++i) c[i] = Cand{g() % 2 ? bits_f(kSpecialBits[g() % kNSpecial]) : nd(g), ids[i], true};
        g_multiset_streams.push_back(add_stream("special-mixed" + sn, c));
        // -0 and +0 only, ids interleaved
        ids = distinct_ids(g, n);
        for (int i = 0; i < n; ++i) c[i] = Cand{bits_f(i % 2 ? 0x80000000u : 0u), ids[i], true};
        g_multiset_streams.push_back(add_stream("zeros" + sn, c));
    }
    // Steps of a chosen number of wanting lanes (R = 1: up to 6 the serial path, from 7 the
    // bitonic batch): first 40 lanes into the empty list (the shortcut), then 20 (a merge), then
    // both paths interleaved. Descending distances make every valid lane want; the random
    // variant lets the threshold thin the steps out.
    const int counts[] = {40, 20, 1, 7, 2, 64, 3, 8, 4, 33, 5, 63, 6, 12, 6, 7, 1, 1, 64, 2, 9, 3, 6, 7};
    for (int variant = 0; variant < 3; ++variant) {
        std::vector<Cand> c;
        float next = 5000.0f;
        for (int cnt : counts) {
            std::vector<int> lanes(64);
            for (int i = 0; i < 64; ++i) lanes[i] = i;
            std::shuffle(lanes.begin(), lanes.end(), g);
            std::vector<Cand> step(64, Cand{INF, NOID, false});
            for (int j = 0; j < cnt; ++j) {
                float d = variant == 0 ? (next -= 1.0f) : (variant == 1 ? nd(g) : kTie8[g() % 8]);
                step[lanes[j]] = Cand{d, random_id(g), true};
            }
            c.insert(c.end(), step.begin(), step.end());
        }
        static const char* names[] = {"steps-descending", "steps-normal", "steps-ties8"};
        g_multiset_streams.push_back(add_stream(names[variant], c));
    }
}

// Unique driver: ids from a pool of `pool` values, so that duplicates arrive both better and
// worse than the stored copy; a few entries carry no id and must be skipped.
static std::vector<int> build_unique_streams(int k, std::mt19937_64& g) {
    std::vector<int> out;
    std::normal_distribution<float> nd(0.0f, 1.0f);
    const int pools[3] = {std::max(1, k / 2), k, 2 * k};
    for (int pool : pools) {
        std::vector<uint64_t> ids = distinct_ids(g, pool);
        for (int n : kSizes) {
            const std::string sn = " pool=" + std::to_string(pool) + " n=" + std::to_string(n);
            for (int kind = 0; kind < 3; ++kind) {
                std::vector<Cand> c(n);
                for (int i = 0; i < n; ++i) {
                    const uint64_t id = ids[g() % pool];
                    float d;
                    if (kind == 0) d = kTie8[g() % 8];
                    else if (kind == 1) d = nd(g);
                    else {  // special values; the sign of a zero follows the id
                        uint32_t b = kSpecialBits[g() % kNSpecial];
                        if ((b & 0x7FFFFFFFu) == 0) b = (id & 1) ? 0x80000000u : 0u;
                        d = g() % 3 ? bits_f(b) : nd(g);
                    }
                    c[i] = g() % 20 == 0 ? Cand{FLT_MAX, NOID, true} : Cand{d, id, true};
                }
                static const char* names[] = {"ties8", "normal", "special-mixed"};
                out.push_back(add_stream(std::string(names[kind]) + sn, c));
            }
        }
    }
    // The stored copy on element p (63, 64, 127, 128, ... below k), then a better duplicate of
    // it that lands at the front, one element lower (across the register edge) or in place.
    for (int p = 63; p < k; p += (p % 64 == 63 ? 1 : 63)) {
        for (int dest = 0; dest < 3; ++dest) {
            std::vector<uint64_t> ids = distinct_ids(g, k);
            std::vector<Cand> c(k);
            for (int e = 0; e < k; ++e) c[e] = Cand{10.0f + (float)e, ids[e], true};
            const float better = dest == 0 ? 1.0f : (dest == 1 ? 10.0f + (float)p - 1.5f : 10.0f + (float)p - 0.5f);
            c.push_back(Cand{better, ids[p], true});
            c.push_back(Cand{10.0f + (float)p + 0.25f, ids[p], true});  // a worse copy: dropped
            static const char* names[] = {"to-front", "one-down", "in-place"};
            out.push_back(add_stream("stored-at-" + std::to_string(p) + " " + names[dest], c));
        }
    }
    return out;
}

// ---- host side: the reference ---------------------------------------------------------------
static std::vector<Key> ref_multiset(const Stream& s, int k) {
    std::vector<Key> v;
    for (const Cand& x : s.c)
        if (x.valid) v.push_back(Key(x.d, x.id));
    std::stable_sort(v.begin(), v.end(), key_before);
    v.resize(k, Key(INF, NOID));  // (cuts or pads)
    return v;
}

static std::vector<Key> ref_unique(const Stream& s, int k) {
    std::map<uint64_t, float> best;
    for (const Cand& x : s.c) {
        if (!x.valid || x.id == NOID) continue;
        auto it = best.find(x.id);
        if (it == best.end()) best[x.id] = x.d;
        else if (x.d < it->second) it->second = x.d;
    }
    std::vector<Key> v;
    for (auto& kv : best) v.push_back(Key(kv.second, kv.first));
    std::stable_sort(v.begin(), v.end(), key_before);
    v.resize(k, Key(INF, NOID));
    return v;
}

// ---- host side: running and comparing ---------------------------------------------------------
struct Expect {
    std::string label;
    std::vector<Key> want;  // compared with the output elements [0, want.size())
};

static long g_mismatches = 0;
static int g_printed = 0;

static void compare(const char* driver, int R, const std::vector<Case>& cases, const std::vector<Expect>& exp,
                    const std::vector<float>& od, const std::vector<uint64_t>& oi) {
    long failed = 0, elems = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        long bad = 0;
        for (size_t e = 0; e < exp[i].want.size(); ++e) {
            const float gd = od[cases[i].out + e];
            const uint64_t gi = oi[cases[i].out + e];
            if (fbits(gd) != fbits(exp[i].want[e].first) || gi != exp[i].want[e].second) {
                if (!bad && g_printed < 40) {
                    ++g_printed;
                    std::printf("  MISMATCH %s R=%d %s: element %zu is (%.9g [%08x], %llu), expected (%.9g [%08x], %llu)\n",
                                driver, R, exp[i].label.c_str(), e, gd, fbits(gd), (unsigned long long)gi,
                                exp[i].want[e].first, fbits(exp[i].want[e].first),
                                (unsigned long long)exp[i].want[e].second);
                }
                ++bad;
            }
        }
        failed += bad != 0;
        elems += bad;
    }
    g_mismatches += elems;
    std::printf("%-10s R=%-2d cases=%-5zu failed=%-5ld mismatched elements=%ld\n", driver, R, cases.size(), failed, elems);
}

template <class T>
static T* to_device(const std::vector<T>& v) {
    T* p = nullptr;
    HIPCHECK(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) HIPCHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

static float* d_sd;
static uint64_t* d_si;
static uint8_t* d_sv;

enum Driver { kMultiset, kUnique, kRemove, kAt, kSort, kMerge };

template <int R>
static void launch(Driver drv, const char* name, std::vector<Case>& cases, const std::vector<Expect>& exp,
                   uint32_t out_per_case) {
    if (cases.empty()) return;
    for (size_t i = 0; i < cases.size(); ++i) cases[i].out = (uint32_t)(i * out_per_case);
    const size_t total = cases.size() * (size_t)out_per_case;
    Case* dc = to_device(cases);
    float* od = nullptr;
    uint64_t* oi = nullptr;
    HIPCHECK(hipMalloc(&od, total * sizeof(float)));
    HIPCHECK(hipMalloc(&oi, total * sizeof(uint64_t)));
    HIPCHECK(hipMemset(od, 0xCD, total * sizeof(float)));
    HIPCHECK(hipMemset(oi, 0xCD, total * sizeof(uint64_t)));
    const dim3 grid((unsigned)cases.size());
    switch (drv) {
        case kMultiset:
        case kUnique: std::abort();  // (run_plan launches these two: their output carries the threshold too)
        case kRemove: run_remove<R><<<grid, 64>>>(dc, d_sd, d_si, od, oi); break;
        case kAt: run_at<R><<<grid, 64>>>(dc, d_sd, d_si, od, oi); break;
        case kSort: run_sort<<<grid, 64>>>(dc, d_sd, d_si, od, oi); break;
        case kMerge: run_merge<<<grid, 64>>>(dc, d_sd, d_si, od, oi); break;
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    std::vector<float> hd(total);
    std::vector<uint64_t> hi(total);
    HIPCHECK(hipMemcpy(hd.data(), od, total * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hi.data(), oi, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
    compare(name, R, cases, exp, hd, hi);
    HIPCHECK(hipFree(dc));
    HIPCHECK(hipFree(od));
    HIPCHECK(hipFree(oi));
}

// The cases of one register count, built before the device image is uploaded.
struct Plan {
    std::vector<Case> multiset, unique, remove, at;
    std::vector<Expect> multiset_x, unique_x, remove_x, at_x;
};

static std::vector<int> capacities(int R) {
    std::vector<int> ks = {1, 64 * (R - 1) + 1, 64 * R - 1, 64 * R};
    if (R == 1) ks = {1, 10, 63, 64};
    return ks;
}

static void add_case(std::vector<Case>& cases, std::vector<Expect>& exps, const Stream& s, int k, uint32_t aux,
                     const std::string& label, std::vector<Key> want) {
    cases.push_back(Case{s.off, s.nslots, (uint32_t)k, aux, 0});
    exps.push_back(Expect{label, std::move(want)});
}

static Plan plan_for(int R, std::map<int, std::vector<int>>& unique_streams) {
    Plan p;
    std::mt19937_64 g(777 + R);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    for (int k : capacities(R)) {
        const std::string sk = "k=" + std::to_string(k) + " ";
        for (int si : g_multiset_streams) {
            const Stream& s = g_streams[si];
            add_case(p.multiset, p.multiset_x, s, k, 0, sk + s.name, ref_multiset(s, k));
        }
        if (!unique_streams.count(k)) unique_streams[k] = build_unique_streams(k, g);
        for (int si : unique_streams[k]) {
            const Stream& s = g_streams[si];
            add_case(p.unique, p.unique_x, s, k, 0, sk + s.name, ref_unique(s, k));
        }
    }
    // remove(e) and at(e): a full and a half-empty sorted list
    for (int fill : {64 * R, 32 * R}) {
        std::vector<uint64_t> ids = distinct_ids(g, 64 * R);
        std::vector<Cand> c(64 * R, Cand{INF, NOID, true});
        for (int e = 0; e < fill; ++e) c[e] = Cand{(float)(e / 2) * 0.75f - 3.0f, ids[e], true};
        std::sort(c.begin(), c.begin() + fill,
                  [](const Cand& a, const Cand& b) { return key_before(Key(a.d, a.id), Key(b.d, b.id)); });
        const Stream& s = g_streams[add_stream("list", c)];
        std::vector<Key> list;
        for (const Cand& x : c) list.push_back(Key(x.d, x.id));
        std::vector<int> es = {0, 63, 64, 64 * R - 1, 32 * R + 5, 32 * R - 1, 32 * R, 17};
        std::sort(es.begin(), es.end());
        es.erase(std::unique(es.begin(), es.end()), es.end());
        for (int e : es) {
            if (e < 0 || e >= 64 * R) continue;
            std::vector<Key> want = list;
            want.erase(want.begin() + e);
            want.push_back(Key(INF, NOID));
            add_case(p.remove, p.remove_x, s, 64 * R, (uint32_t)e,
                     "fill=" + std::to_string(fill) + " e=" + std::to_string(e), want);
        }
        add_case(p.at, p.at_x, s, 64 * R, 0, "sorted fill=" + std::to_string(fill), list);
    }
    {  // at(e) on unsorted content: every element distinct
        std::vector<Cand> c(64 * R);
        for (int e = 0; e < 64 * R; ++e) c[e] = Cand{nd(g), random_id(g), true};
        const Stream& s = g_streams[add_stream("unsorted", c)];
        std::vector<Key> list;
        for (const Cand& x : c) list.push_back(Key(x.d, x.id));
        add_case(p.at, p.at_x, s, 64 * R, 0, "unsorted", list);
    }
    return p;
}

template <int R>
static void run_plan(Plan& p) {
    // Elements [0, k) are compared (k .. 64 R - 1 hold what fell out of the list and are not part
    // of the contract), then the running threshold behind the 64 R elements: it is element k - 1.
    auto with_threshold = [&](Driver drv, const char* name, std::vector<Case>& cases, std::vector<Expect>& exps) {
        std::vector<Expect> thr(exps.size());
        for (size_t i = 0; i < exps.size(); ++i) thr[i] = Expect{exps[i].label + " (threshold)", {exps[i].want.back()}};
        if (cases.empty()) return;
        for (size_t i = 0; i < cases.size(); ++i) cases[i].out = (uint32_t)(i * (64 * R + 1));
        const size_t total = cases.size() * (size_t)(64 * R + 1);
        Case* dc = to_device(cases);
        float* od = nullptr;
        uint64_t* oi = nullptr;
        HIPCHECK(hipMalloc(&od, total * sizeof(float)));
        HIPCHECK(hipMalloc(&oi, total * sizeof(uint64_t)));
        HIPCHECK(hipMemset(od, 0xCD, total * sizeof(float)));
        HIPCHECK(hipMemset(oi, 0xCD, total * sizeof(uint64_t)));
        const dim3 grid((unsigned)cases.size());
        if (drv == kMultiset) run_multiset<R><<<grid, 64>>>(dc, d_sd, d_si, d_sv, od, oi);
        else run_unique<R><<<grid, 64>>>(dc, d_sd, d_si, d_sv, od, oi);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        std::vector<float> hd(total);
        std::vector<uint64_t> hi(total);
        HIPCHECK(hipMemcpy(hd.data(), od, total * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hi.data(), oi, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        compare(name, R, cases, exps, hd, hi);
        std::vector<Case> tc = cases;
        for (Case& c : tc) c.out += 64 * R;
        compare((std::string(name) + "-kth").c_str(), R, tc, thr, hd, hi);
        HIPCHECK(hipFree(dc));
        HIPCHECK(hipFree(od));
        HIPCHECK(hipFree(oi));
    };
    with_threshold(kMultiset, "multiset", p.multiset, p.multiset_x);
    with_threshold(kUnique, "unique", p.unique, p.unique_x);
    launch<R>(kRemove, "remove", p.remove, p.remove_x, 64 * R);
    launch<R>(kAt, "at", p.at, p.at_x, 64 * R);
}

// ---- the R-independent primitives ---------------------------------------------------------------
struct PrimPlan {
    std::vector<Case> sort, merge;
    std::vector<Expect> sort_x, merge_x;
};

static PrimPlan plan_primitives() {
    PrimPlan p;
    std::mt19937_64 g(4242);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    auto keys_of = [](const std::vector<Cand>& c) {
        std::vector<Key> v;
        for (const Cand& x : c) v.push_back(Key(x.d, x.id));
        return v;
    };
    auto make_step = [&](int kind) {
        std::vector<Cand> c(64);
        std::vector<uint64_t> ids = distinct_ids(g, 64);
        const int holes = kind == 5 ? (int)(g() % 64) : 0;
        for (int i = 0; i < 64; ++i) {
            switch (kind) {
                case 0: c[i] = Cand{nd(g), random_id(g), true}; break;
                case 1: c[i] = Cand{kTie8[g() % 8], ids[i], true}; break;
                case 2: c[i] = Cand{1.25f, ids[i], true}; break;
                case 3: c[i] = Cand{bits_f(kSpecialBits[g() % kNSpecial]), ids[i], true}; break;
                case 4: c[i] = Cand{(float)(64 - i), ids[i], true}; break;  // reversed
                default: c[i] = i < holes ? Cand{INF, NOID, true} : Cand{nd(g), ids[i], true}; break;  // a thin batch
            }
        }
        if (kind == 5) std::shuffle(c.begin(), c.end(), g);
        return c;
    };
    for (int rep = 0; rep < 8; ++rep)
        for (int kind = 0; kind < 6; ++kind) {
            std::vector<Cand> c = make_step(kind);
            const Stream& s = g_streams[add_stream("sort", c)];
            std::vector<Key> want = keys_of(c);
            std::stable_sort(want.begin(), want.end(), key_before);
            add_case(p.sort, p.sort_x, s, 64, 0, "kind=" + std::to_string(kind) + " rep=" + std::to_string(rep), want);
            // already sorted input
            std::vector<Cand> sorted(64);
            for (int i = 0; i < 64; ++i) sorted[i] = Cand{want[i].first, want[i].second, true};
            const Stream& s2 = g_streams[add_stream("sorted", sorted)];
            add_case(p.sort, p.sort_x, s2, 64, 0, "sorted kind=" + std::to_string(kind), want);
        }
    for (int rep = 0; rep < 8; ++rep)
        for (int ka = 0; ka < 7; ++ka)
            for (int kb = 0; kb < 6; ++kb) {
                std::vector<Cand> a = ka == 6 ? std::vector<Cand>(64, Cand{INF, NOID, true}) : make_step(ka);  // 6: the empty list
                std::vector<Cand> b = make_step(kb);
                auto by_key = [](const Cand& x, const Cand& y) { return key_before(Key(x.d, x.id), Key(y.d, y.id)); };
                std::stable_sort(a.begin(), a.end(), by_key);
                std::stable_sort(b.begin(), b.end(), by_key);
                std::vector<Key> want = keys_of(a), kb_ = keys_of(b);
                want.insert(want.end(), kb_.begin(), kb_.end());
                std::stable_sort(want.begin(), want.end(), key_before);
                want.resize(64);
                // (ids of a and b may coincide at one distance; those pairs are bit-equal or
                // differ in the distance, except -0 / +0 of one id: redraw such a case)
                bool ambiguous = false;
                for (const Cand& x : a)
                    for (const Cand& y : b)
                        if (x.id == y.id && x.d == y.d && fbits(x.d) != fbits(y.d)) ambiguous = true;
                if (ambiguous) continue;
                a.insert(a.end(), b.begin(), b.end());
                const Stream& s = g_streams[add_stream("merge", a)];
                add_case(p.merge, p.merge_x, s, 64, 0,
                         "list kind=" + std::to_string(ka) + " batch kind=" + std::to_string(kb), want);
            }
    return p;
}

static void run_lane_op_checks() {
    const int blocks = 4;
    std::mt19937_64 g(99);
    std::vector<uint32_t> in(blocks * 64);
    for (int b = 0; b < blocks; ++b)
        for (int l = 0; l < 64; ++l) in[b * 64 + l] = b == 0 ? (uint32_t)l : (uint32_t)g();  // block 0: the lane number itself
    uint32_t* din = to_device(in);
    uint32_t* dout = nullptr;
    const size_t total = (size_t)blocks * kLaneOps * 64;
    HIPCHECK(hipMalloc(&dout, total * 4));
    HIPCHECK(hipMemset(dout, 0xCD, total * 4));
    run_lane_ops<<<blocks, 64>>>(din, dout);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint32_t> out(total);
    HIPCHECK(hipMemcpy(out.data(), dout, total * 4, hipMemcpyDeviceToHost));
    static const char* names[kLaneOps] = {"xor_u32<1>", "xor_u32<2>", "xor_u32<4>", "xor_u32<8>",
                                          "xor_u32<16>", "xor_u32<32>", "up1_u32", "down1_u32"};
    for (int op = 0; op < kLaneOps; ++op) {
        long bad = 0;
        for (int b = 0; b < blocks; ++b) {
            const uint32_t* v = &in[b * 64];
            const uint32_t fill = v[0] ^ 0xA5A5A5A5u;
            for (int l = 0; l < 64; ++l) {
                uint32_t want;
                if (op < 6) want = v[l ^ (1 << op)];
                else if (op == 6) want = l == 0 ? fill : v[l - 1];
                else want = l == 63 ? fill : v[l + 1];
                const uint32_t got = out[((size_t)b * kLaneOps + op) * 64 + l];
                if (got != want) {
                    if (!bad && g_printed < 40) {
                        ++g_printed;
                        std::printf("  MISMATCH %s block %d lane %d: got %08x, expected %08x\n", names[op], b, l, got, want);
                    }
                    ++bad;
                }
            }
        }
        g_mismatches += bad;
        std::printf("%-12s cases=%d mismatched lanes=%ld\n", names[op], blocks, bad);
    }
    HIPCHECK(hipFree(din));
    HIPCHECK(hipFree(dout));
}

int main() {
    build_multiset_streams();
    std::map<int, std::vector<int>> unique_streams;
    Plan p1 = plan_for(1, unique_streams), p2 = plan_for(2, unique_streams), p4 = plan_for(4, unique_streams),
         p8 = plan_for(8, unique_streams), p16 = plan_for(16, unique_streams);
    PrimPlan pp = plan_primitives();
    d_sd = to_device(g_sd);
    d_si = to_device(g_si);
    d_sv = to_device(g_sv);
    std::printf("wave_topk_test: %zu streams, %zu slots\n", g_streams.size(), g_sd.size());
    run_lane_op_checks();
    launch<1>(kSort, "sort64", pp.sort, pp.sort_x, 64);
    launch<1>(kMerge, "merge64", pp.merge, pp.merge_x, 64);
    run_plan<1>(p1);
    run_plan<2>(p2);
    run_plan<4>(p4);
    run_plan<8>(p8);
    run_plan<16>(p16);
    std::printf("mismatches: %ld\n", g_mismatches);
    return g_mismatches ? 1 : 0;
}
