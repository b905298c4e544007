// cosine_map_test.cpp — CPU test of csrc/cosine_map.hpp: the radius of a CosineDistance range
// search (in reported distances, fl(1.0f + d)) mapped to the scan's threshold in -dot.
// Stand-alone: g++ -std=c++17, plain and with -fsanitize=address,undefined (tests/test_cosine_map.py).
//
// For every radius r: t = cos_threshold(r) satisfies fl(1 + t) <= r, and the next float above t
// does not (unless t is FLT_MAX or infinite): t is the largest such float, so "reported
// distance <= r" is exactly "-dot <= t".
#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/cosine_map.hpp"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int failures = 0;

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static void check(bool ok, const char* what, float r, float t) {
    if (ok) return;
    ++failures;
    std::printf("FAILED %s: radius %.9g (0x%08x) threshold %.9g (0x%08x)\n", what, r, bits(r), t, bits(t));
}

// (volatile: the add is the rounded fp32 add, whatever the optimiser would like to fold)
static float map1(float d) {
    volatile float one = 1.0f, x = d;
    volatile float s = one + x;
    return s;
}

static void check_radius(float r) {
    const float t = vdbe::cos_threshold(r);
    check(!std::isnan(t), "threshold is a number", r, t);
    check(map1(t) <= r, "fl(1 + t) <= r", r, t);
    if (t == FLT_MAX || std::isinf(t)) return;
    const float up = std::nextafterf(t, HUGE_VALF);
    check(map1(up) > r, "fl(1 + next(t)) > r", r, t);
    check(bits(vdbe::cos_map(t)) == bits(map1(t)), "cos_map is the fp32 add", r, t);
}

int main() {
    const float inf = HUGE_VALF;
    std::vector<float> radii = {0.0f, 1.0f, 2.0f, 0.5f, -1.0f, 3.0f, 1.0f - std::ldexp(1.0f, -24),
                                1.0f + std::ldexp(1.0f, -23), 1e-8f, FLT_MAX, inf, -inf,
                                -0.0f, -1e-8f, 1e-30f, -1e-30f, -FLT_MAX, 1e10f, -1e10f, FLT_MIN, 16777216.0f};
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> u(-1.0f, 3.0f);
    for (int i = 0; i < 5000; ++i) radii.push_back(u(gen));
    // every float around 0, 1 and 2, where the map's spacing changes
    for (float c : {0.0f, 1.0f, 2.0f}) {
        float lo = c, hi = c;
        for (int i = 0; i < 40; ++i) {
            lo = std::nextafterf(lo, -inf);
            hi = std::nextafterf(hi, inf);
            radii.push_back(lo);
            radii.push_back(hi);
        }
    }
    for (float r : radii) check_radius(r);

    // the fixed points the header names
    check(vdbe::cos_threshold(inf) == inf, "+inf -> +inf", inf, vdbe::cos_threshold(inf));
    check(vdbe::cos_threshold(-inf) == -inf, "-inf -> -inf", -inf, vdbe::cos_threshold(-inf));
    check(vdbe::cos_threshold(FLT_MAX) == FLT_MAX, "FLT_MAX -> FLT_MAX", FLT_MAX, vdbe::cos_threshold(FLT_MAX));
    check(std::isnan(vdbe::cos_threshold(NAN)), "NaN comes back", NAN, vdbe::cos_threshold(NAN));
    // hand-derived: radius 0 admits -dot <= -1 (1 + (-1 + 2^-24) = 2^-24 > 0); radius 1 admits
    // -dot up to 2^-24 (1 + 2^-24 is a tie, to even: 1.0); radius 2 up to 1 + 2^-23 (2 + 2^-23 is
    // a tie, to even: 2.0)
    check(vdbe::cos_threshold(0.0f) == -1.0f, "radius 0 -> -1", 0.0f, vdbe::cos_threshold(0.0f));
    check(vdbe::cos_threshold(1.0f) == std::ldexp(1.0f, -24), "radius 1 -> 2^-24", 1.0f, vdbe::cos_threshold(1.0f));
    check(vdbe::cos_threshold(2.0f) == 1.0f + std::ldexp(1.0f, -23), "radius 2 -> 1 + 2^-23", 2.0f,
          vdbe::cos_threshold(2.0f));

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("%zu radii: all checks passed\n", radii.size());
    return 0;
}
