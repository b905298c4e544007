// cosine_map.hpp — the host side of Metric::CosineDistance's distance mapping. Host-only: no
// device headers, so a plain C++ compiler builds and tests it (tests/cpp/cosine_map_test.cpp).
//
// A CosineDistance handle is an inner-product handle over unit rows; a reported distance is
// cos_map(d) = fl(1.0f + d) of the handle's own d = -dot. The map is monotone but not
// one-to-one, so a radius given in mapped distances becomes the scan's threshold in -dot:
// cos_threshold(radius) is the largest fp32 t with fl(1.0f + t) <= radius, and "mapped
// distance <= radius" is then exactly "d <= t".
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace vdbe {

// The same IEEE add the device applies (launch_cos_finish).
inline float cos_map(float d) { return 1.0f + d; }

// Floats as integers in their own order (-FLT_MAX .. -0, +0 .. FLT_MAX), and back.
inline uint32_t cos_ordered(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float cos_unordered(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// +inf -> +inf, -inf -> -inf, FLT_MAX -> FLT_MAX; a NaN radius is the caller's to refuse (it
// comes back as it went in). radius - 1.0f is the answer up to the add's rounding; where it is
// not (within a few nextafterf steps), the map's monotonicity settles it by bisection over the
// floats in order: near radius 1 the answers are 2^23 floats apart from radius - 1.0f, too many
// to step through.
inline float cos_threshold(float radius) {
    if (std::isnan(radius) || std::isinf(radius)) return radius;
    auto within = [&](float t) { return cos_map(t) <= radius; };
    auto largest = [&](float t) { return within(t) && (t == FLT_MAX || !within(std::nextafterf(t, HUGE_VALF))); };
    float t = radius - 1.0f;  // (finite: |radius| <= FLT_MAX)
    for (int step = 0; step < 4 && !largest(t); ++step) t = std::nextafterf(t, within(t) ? HUGE_VALF : -HUGE_VALF);
    if (largest(t)) return t;
    if (within(FLT_MAX)) return FLT_MAX;
    uint32_t lo = cos_ordered(-FLT_MAX), hi = cos_ordered(FLT_MAX);  // within(lo) (1 - FLT_MAX = -FLT_MAX), not within(hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (within(cos_unordered(mid))) lo = mid;
        else hi = mid;
    }
    return cos_unordered(lo);
}

}  // namespace vdbe
