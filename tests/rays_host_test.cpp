// rays_host_test.cpp -- rt_ray_guard.h on the host: rt::ray_usable, the predicate that decides which caller-supplied rays reach traversal
// (rt_trace_closest_device / rt_trace_any_device lay an unusable ray out as an empty one).  Cases: NaN, +inf and -inf in each of the eight
// components of an otherwise ordinary ray; a zero direction (+0 and -0); a denormal direction; maxt = +inf; mint > maxt; mint = -inf; the extreme
// records of the degenerate-ray classes of tests/edge_rays_cases.py (signed zeros next to an axis direction, scaled and denormal d); and a
// few thousand seeded random finite rays.  The verdict is also held against <cmath>'s classification, and the empty ray an unusable one
// becomes is checked to be usable and empty.  Stand-alone (tests/test_rays_host.py builds it under AddressSanitizer and
// UndefinedBehaviorSanitizer); no GPU, no HIP header.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "rt_ray_guard.h"

namespace {

unsigned long long g_checked = 0, g_failed = 0;

// the issue's definition, spelled with <cmath>
bool expected(const float *r) {
    for (int i = 0; i < 6; ++i) if (!std::isfinite(r[i])) return false;
    if (r[3] == 0.f && r[4] == 0.f && r[5] == 0.f) return false;
    return !std::isnan(r[6]) && !std::isnan(r[7]);
}

void check(const char *what, const float *r, bool want) {
    ++g_checked;
    const bool got = rt::ray_usable(r), got8 = rt::ray_usable(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
    if (got == want && got8 == want && expected(r) == want) return;
    if (g_failed++ < 10)
        std::fprintf(stderr, "CHECK(ray_usable) %s: o %g %g %g d %g %g %g mint %g maxt %g: got %d / %d, <cmath> says %d, expected %d\n", what,
                     r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], int(got), int(got8), int(expected(r)), int(want));
}

uint64_t mix(uint64_t &x) {                                             // splitmix64: the seeded rays
    uint64_t z = (x += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float denorm = std::numeric_limits<float>::denorm_min();
    const float base[8] = {278.f, 273.f, -800.f, .1f, -.2f, .97f, 0.f, 1000.f};
    check("an ordinary ray", base, true);

    // NaN, +inf, -inf in each component: o and d refuse all three, mint and maxt only NaN
    float snan; { const uint32_t b = 0x7f800001u; std::memcpy(&snan, &b, 4); }     // a signalling pattern, and one with the sign set
    float nnan; { const uint32_t b = 0xffc00000u; std::memcpy(&nnan, &b, 4); }
    const float bad[5] = {nan, snan, nnan, inf, -inf};
    for (int i = 0; i < 8; ++i)
        for (int k = 0; k < 5; ++k) {
            float r[8]; std::memcpy(r, base, sizeof r);
            r[i] = bad[k];
            const bool is_nan = k < 3;
            check(i < 6 ? "non-finite o / d" : "non-finite mint / maxt", r, i < 6 ? false : !is_nan);
        }

    {   // zero directions, every sign pattern
        for (int m = 0; m < 8; ++m) {
            float r[8]; std::memcpy(r, base, sizeof r);
            r[3] = (m & 1) ? -0.f : 0.f; r[4] = (m & 2) ? -0.f : 0.f; r[5] = (m & 4) ? -0.f : 0.f;
            check("zero direction", r, false);
        }
        for (int i = 3; i < 6; ++i) {                                    // one non-zero component is a direction: axis-aligned, and denormal
            float r[8]; std::memcpy(r, base, sizeof r);
            r[3] = r[4] = r[5] = 0.f; r[i] = -1.f;
            check("axis-aligned direction", r, true);
            r[i] = denorm;
            check("denormal direction", r, true);
            r[i] = -denorm;
            check("denormal direction", r, true);
        }
    }
    {   // the ordinary ends of a ray's range
        float r[8]; std::memcpy(r, base, sizeof r);
        r[7] = inf; check("maxt = +inf", r, true);
        r[6] = 5.f; r[7] = 1.f; check("mint > maxt", r, true);
        r[6] = -inf; r[7] = inf; check("mint = -inf", r, true);
        r[6] = std::numeric_limits<float>::max(); r[7] = -std::numeric_limits<float>::max(); check("mint > maxt at the ends of the range", r, true);
        r[0] = std::numeric_limits<float>::max(); r[1] = -std::numeric_limits<float>::max(); r[2] = denorm; check("o at the ends of the range", r, true);
    }
    {   // the extreme records of the degenerate-ray classes (tests/edge_rays_cases.py): all of them reach traversal
        for (int axis = 0; axis < 3; ++axis)                             // class a: an axis-aligned direction, the two zeros in every combination of +0.f and -0.f
            for (int m = 0; m < 8; ++m) {
                float r[8] = {7.1f, 13.35f, 18.2f, 0.f, 0.f, 0.f, 0.f, 1000.f};
                r[3 + axis] = (m & 4) ? -1.f : 1.f;
                r[3 + (axis + 1) % 3] = (m & 1) ? -0.f : 0.f; r[3 + (axis + 2) % 3] = (m & 2) ? -0.f : 0.f;
                check("axis-aligned direction, signed zeros", r, true);
            }
        for (int k = 0; k < 4; ++k) {                                    // class h: d scaled by 2^k with mint, maxt scaled by 2^-k ...
            const int e[4] = {-60, -20, 20, 60};
            float r[8]; std::memcpy(r, base, sizeof r);
            for (int i = 3; i < 6; ++i) r[i] = std::ldexp(r[i], e[k]);
            r[7] = std::ldexp(r[7], -e[k]);
            check("scaled direction", r, true);
        }
        {   // ... and into the denormal range, every component, where 1 / d overflows; maxt = +inf
            float r[8]; std::memcpy(r, base, sizeof r);
            for (int i = 3; i < 6; ++i) r[i] = std::ldexp(r[i], -140);
            r[7] = inf;
            ++g_checked;
            for (int i = 3; i < 6; ++i)
                if (std::fpclassify(r[i]) != FP_SUBNORMAL || std::isfinite(1.f / r[i])) { ++g_failed; std::fprintf(stderr, "CHECK(denormal d) %g is not one\n", r[i]); }
            check("denormal direction, maxt = +inf", r, true);
            r[4] = -0.f; r[5] = 0.f;
            check("denormal axis-aligned direction, signed zeros", r, true);
        }
        {   // class g: mint == maxt, and mint one step above maxt
            float r[8]; std::memcpy(r, base, sizeof r);
            r[6] = r[7] = 229.42726f; check("mint == maxt", r, true);
            r[6] = std::nextafter(r[7], inf); check("mint = nextafter(maxt)", r, true);
            r[6] = -500.f; r[7] = 1000.f; check("negative mint", r, true);
        }
    }
    {   // what an unusable ray becomes
        const float e[8] = {RT_EMPTY_RAY_O, RT_EMPTY_RAY_D, RT_EMPTY_RAY_MINT, RT_EMPTY_RAY_MAXT};
        check("the empty ray", e, true);
        ++g_checked;
        if (!(e[6] > e[7])) { ++g_failed; std::fprintf(stderr, "CHECK(empty ray) mint %g is not above maxt %g\n", e[6], e[7]); }
    }
    {   // seeded random finite rays: every finite bit pattern is allowed in o, d (not all zero), mint, maxt
        uint64_t seed = 20240607ull;
        auto finite_bits = [&]() { uint32_t b; do { b = uint32_t(mix(seed)); } while ((b & 0x7f800000u) == 0x7f800000u); float f; std::memcpy(&f, &b, 4); return f; };
        for (int n = 0; n < 4096; ++n) {
            float r[8];
            for (int i = 0; i < 8; ++i) r[i] = finite_bits();
            if (r[3] == 0.f && r[4] == 0.f && r[5] == 0.f) r[4] = 1.f;
            check("random finite ray", r, true);
        }
        for (int n = 0; n < 2048; ++n) {                                 // ... in the ranges scenes use
            float r[8];
            for (int i = 0; i < 6; ++i) r[i] = float(double(mix(seed) >> 11) / double(1ull << 53) * 2000.0 - 1000.0);
            r[6] = float(double(mix(seed) >> 11) / double(1ull << 53)); r[7] = r[6] + float(double(mix(seed) >> 11) / double(1ull << 53) * 1e4);
            if (r[3] == 0.f && r[4] == 0.f && r[5] == 0.f) r[4] = 1.f;
            check("random scene ray", r, true);
        }
    }
    if (g_failed) { std::fprintf(stderr, "rays_host_test: %llu of %llu checks FAILED\n", g_failed, g_checked); return 1; }
    std::printf("rays_host_test: ok (%llu rays)\n", g_checked);
    return 0;
}
