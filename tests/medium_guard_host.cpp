// tests/medium_guard_host.cpp -- rt::march_advances and rt::march_caps (pbrt-v1_amd/csrc/hip/rt_march_guard.h, no HIP header) with a host compiler:
// the predicate that keeps rt_medium_device from starting a march that could not advance, and the limits that refuse a step before any launch.
// Built and run by tests/test_medium_host.py; a stand-alone program, so it can be built with -fsanitize=address,undefined as it is.
#include <cmath>
#include <cstdio>
#include <limits>
#include "rt_march_guard.h"

static int failures = 0, checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #x); } } while (0)

// the loop the predicate speaks for, with a cap of its own: does `while (t < t1) t += step` from t0 end within `cap` additions?
static bool loop_ends(float t0, float t1, float step, int cap) {
    volatile float t = t0;
    for (int k = 0; k < cap; ++k) { if (!(t < t1)) return true; t = t + step; }
    return !(t < t1);
}

int main() {
    using namespace rt;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // t = 3e8 with step 10: the spacing of floats there is 32, t + 10 == t
    CHECK(3e8f + 10.f == 3e8f);
    CHECK(!march_advances(3e8f, 3e8f + 64.f, 10.f));
    CHECK(!march_advances(3e8f - 64.f, 3e8f, 10.f));
    CHECK(!loop_ends(3e8f, 3e8f + 64.f, 10.f, 1000));
    CHECK(march_advances(3e8f, 3e8f + 64.f, 32.f) && loop_ends(3e8f, 3e8f + 64.f, 32.f, 1000));
    CHECK(march_advances(3e8f, 3e8f + 64.f, 17.f));                      // above half a spacing: rounds up to the next float
    // t = 0 and negative t: the magnitude decides
    CHECK(march_advances(0.f, 0.f, 1e-30f));
    CHECK(march_advances(0.f, 5.f, .125f) && loop_ends(0.f, 5.f, .125f, 100));
    CHECK(march_advances(-5.f, -1.f, .125f) && loop_ends(-5.f, -1.f, .125f, 100));
    CHECK(!march_advances(-3e8f, 2.f, 10.f) && !loop_ends(-3e8f, 2.f, 10.f, 1000));
    CHECK(!march_advances(-3e8f, -3e8f + 64.f, 10.f));
    CHECK(!march_advances(1.f, 2.f, 1e-9f));                             // below half an ulp of 2
    CHECK(march_advances(1.f, 2.f, 2e-7f));
    // inf / NaN, and steps that are no steps
    CHECK(!march_advances(0.f, inf, 1.f) && !march_advances(-inf, 0.f, 1.f) && !march_advances(nan, 1.f, 1.f) && !march_advances(0.f, nan, 1.f));
    CHECK(!march_advances(0.f, 1.f, 0.f) && !march_advances(0.f, 1.f, -1.f) && !march_advances(0.f, 1.f, inf) && !march_advances(0.f, 1.f, nan));
    CHECK(!march_step_ok(0.f) && !march_step_ok(-0.f) && !march_step_ok(-1.f) && !march_step_ok(inf) && !march_step_ok(nan) && march_step_ok(1e-38f));
    // wherever the predicate says yes, the loop ends within the cap the host hands the kernel for that diagonal
    unsigned s = 12345u;
    auto rnd = [&s] { s = s * 1664525u + 1013904223u; return float(s >> 8) / float(1 << 24); };
    for (int i = 0; i < 20000; ++i) {
        const float t0 = (rnd() - .5f) * std::pow(10.f, rnd() * 9.f), len = rnd() * 8.f, step = .01f + rnd();
        MarchCaps c;
        if (march_caps(step, len, len, true, c) != MARCH_OK) continue;
        if (march_advances(t0, t0 + len, .5f * step)) CHECK(loop_ends(t0, t0 + len, .5f * step, 4 * c.taus + 64));
    }
    // the refusal limits: 65536 march steps and 2^20 Tau samples over the diagonal, plan_march's expressions
    MarchCaps c;
    CHECK(march_caps(0.f, 1., 1., true, c) == MARCH_BAD_STEP && march_caps(-1.f, 1., 1., false, c) == MARCH_BAD_STEP);
    CHECK(march_caps(inf, 1., 1., true, c) == MARCH_BAD_STEP && march_caps(nan, 1., 1., false, c) == MARCH_BAD_STEP);
    CHECK(march_caps(1.f, 65534., 0., false, c) == MARCH_OK && c.steps == 65536 && c.taus == 0);
    CHECK(march_caps(1.f, 65534.5, 0., false, c) == MARCH_TOO_MANY_STEPS);
    CHECK(march_caps(1.f, 10., 65534., true, c) == MARCH_OK && c.steps == 65536 && c.taus == 131070);
    CHECK(march_caps(1.f, 10., 65534.5, true, c) == MARCH_TOO_MANY_STEPS);
    // (a scaled region: few steps across its own diagonal, many across the world's) exactly 2^20 Tau samples pass that limit and meet the next one
    CHECK(march_caps(16.f, 10., 8. * ((1 << 20) - 2), true, c) == MARCH_TOO_MANY_STEPS);
    CHECK(march_caps(16.f, 10., 8. * ((1 << 20) - 2) + 1., true, c) == MARCH_TOO_MANY_TAUS);
    CHECK(march_caps(.25f, 4., 4., true, c) == MARCH_OK && c.steps == 18 && c.taus == 34);
    CHECK(RT_MARCH_MAX_TAUS == (1 << 20) && RT_MARCH_MAX_STEPS == 65536 && RT_MEDIUM_NO_ADVANCE == 1);
    if (failures) { std::printf("medium_guard_host: %d of %d checks failed\n", failures, checks); return 1; }
    std::printf("medium_guard_host: ok (%d checks)\n", checks);
    return 0;
}
