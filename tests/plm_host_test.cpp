// plm_host_test.cpp -- rt_libm_portable.h on the host, stand-alone (tests/test_plm_host.py builds it under AddressSanitizer and
// UndefinedBehaviorSanitizer; no GPU, no HIP header): the edge conventions one by one, and 2^20 seeded arguments per function against the
// C library's double functions, at most 1 float ulp apart (the double evaluation rounded once is within 0.5 + 2^-20).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "rt_libm_portable.h"

namespace {

unsigned long long g_checked = 0, g_failed = 0;
const float INF = std::numeric_limits<float>::infinity(), QNAN = std::numeric_limits<float>::quiet_NaN(), FMAX = std::numeric_limits<float>::max();
const float PI_F = 3.14159274f;

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

void same(const char *what, float got, float want) {            // bit for bit (signed zeros told apart), any NaN equals any NaN
    ++g_checked;
    if ((std::isnan(got) && std::isnan(want)) || bits(got) == bits(want)) return;
    if (g_failed++ < 20) std::fprintf(stderr, "CHECK(edge) %s: got %.9g (%08x), expected %.9g (%08x)\n", what, got, bits(got), want, bits(want));
}

uint64_t mix(uint64_t &x) {                                        // splitmix64
    uint64_t z = (x += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
double unit(uint64_t &s) { return double(mix(s) >> 11) * (1.0 / 9007199254740992.0); }
float range(uint64_t &s, double lo, double hi) { return float(lo + (hi - lo) * unit(s)); }

double worst[7];
void near(int fn, const char *name, float a, float b, float got, double want) {
    ++g_checked;
    const float w = float(want);
    if (std::isnan(w) || std::isinf(w) || w == 0.f) {              // outside float's range: the rounded value itself
        if ((std::isnan(got) && std::isnan(w)) || got == w) return;
        if (std::fabs(double(got) - want) <= 1.4012984643248171e-45) return;      // within one denormal step of an underflowing value
    } else {
        int e; std::frexp(w, &e);
        const double ulp = std::ldexp(1.0, (e < -125 ? -125 : e) - 24);
        const double err = std::fabs(double(got) - want) / ulp;
        if (err > worst[fn]) worst[fn] = err;
        if (err <= 1.0) return;
    }
    if (g_failed++ < 20) std::fprintf(stderr, "CHECK(ulp) %s(%.9g, %.9g): got %.9g, float64 %.17g\n", name, a, b, got, want);
}

void edges() {
    // sinf / cosf / sincosf
    same("sinf(+0)", plm_sinf(0.f), 0.f); same("sinf(-0)", plm_sinf(-0.f), -0.f); same("cosf(0)", plm_cosf(0.f), 1.f);
    same("sinf(inf)", plm_sinf(INF), QNAN); same("cosf(-inf)", plm_cosf(-INF), QNAN); same("sinf(nan)", plm_sinf(QNAN), QNAN);
    same("sinf(1e-40)", plm_sinf(1e-40f), 1e-40f); same("sinf(FLT_MAX)", plm_sinf(FMAX), 0.f); same("cosf(FLT_MAX)", plm_cosf(FMAX), 1.f);
    float s, c; plm_sincosf(0.5f, &s, &c); same("sincosf.s", s, plm_sinf(0.5f)); same("sincosf.c", c, plm_cosf(0.5f));
    plm_sincosf(QNAN, &s, &c); same("sincosf(nan).s", s, QNAN); same("sincosf(nan).c", c, QNAN);
    // acosf
    same("acosf(1)", plm_acosf(1.f), 0.f); same("acosf(-1)", plm_acosf(-1.f), PI_F); same("acosf(0)", plm_acosf(0.f), 1.57079637f);
    same("acosf(1.0000001)", plm_acosf(1.0000001f), QNAN); same("acosf(-2)", plm_acosf(-2.f), QNAN); same("acosf(nan)", plm_acosf(QNAN), QNAN);
    // atan2f: signed zeros, the axes, all quadrants, infinities (the quadrics add 2 pi when phi < 0)
    same("atan2f(+0,+0)", plm_atan2f(0.f, 0.f), 0.f); same("atan2f(-0,+0)", plm_atan2f(-0.f, 0.f), -0.f);
    same("atan2f(+0,-0)", plm_atan2f(0.f, -0.f), PI_F); same("atan2f(-0,-0)", plm_atan2f(-0.f, -0.f), -PI_F);
    same("atan2f(+0,1)", plm_atan2f(0.f, 1.f), 0.f); same("atan2f(-0,1)", plm_atan2f(-0.f, 1.f), -0.f);
    same("atan2f(+0,-1)", plm_atan2f(0.f, -1.f), PI_F); same("atan2f(-0,-1)", plm_atan2f(-0.f, -1.f), -PI_F);
    same("atan2f(1,0)", plm_atan2f(1.f, 0.f), 1.57079637f); same("atan2f(-1,-0)", plm_atan2f(-1.f, -0.f), -1.57079637f);
    same("atan2f(1,1)", plm_atan2f(1.f, 1.f), 0.785398185f); same("atan2f(1,-1)", plm_atan2f(1.f, -1.f), 2.35619450f);
    same("atan2f(-1,-1)", plm_atan2f(-1.f, -1.f), -2.35619450f); same("atan2f(-1,1)", plm_atan2f(-1.f, 1.f), -0.785398185f);
    same("atan2f(1,inf)", plm_atan2f(1.f, INF), 0.f); same("atan2f(-1,inf)", plm_atan2f(-1.f, INF), -0.f); same("atan2f(1,-inf)", plm_atan2f(1.f, -INF), PI_F);
    same("atan2f(inf,1)", plm_atan2f(INF, 1.f), 1.57079637f); same("atan2f(inf,inf)", plm_atan2f(INF, INF), 0.785398185f);
    same("atan2f(-inf,-inf)", plm_atan2f(-INF, -INF), -2.35619450f); same("atan2f(nan,1)", plm_atan2f(QNAN, 1.f), QNAN); same("atan2f(1,nan)", plm_atan2f(1.f, QNAN), QNAN);
    same("atan2f(FLT_MAX,FLT_MAX)", plm_atan2f(FMAX, FMAX), 0.785398185f); same("atan2f(1e-45,FLT_MAX)", plm_atan2f(1.4e-45f, FMAX), 0.f);
    // powf
    same("powf(0,2)", plm_powf(0.f, 2.f), 0.f); same("powf(0,0.5)", plm_powf(0.f, 0.5f), 0.f); same("powf(-0,3)", plm_powf(-0.f, 3.f), -0.f); same("powf(-0,2)", plm_powf(-0.f, 2.f), 0.f);
    same("powf(0,-1)", plm_powf(0.f, -1.f), INF); same("powf(-0,-3)", plm_powf(-0.f, -3.f), -INF);
    same("powf(5,0)", plm_powf(5.f, 0.f), 1.f); same("powf(nan,0)", plm_powf(QNAN, 0.f), 1.f); same("powf(0,0)", plm_powf(0.f, 0.f), 1.f); same("powf(-3,-0)", plm_powf(-3.f, -0.f), 1.f);
    same("powf(1,nan)", plm_powf(1.f, QNAN), 1.f); same("powf(1,inf)", plm_powf(1.f, INF), 1.f);
    same("powf(-2,0.5)", plm_powf(-2.f, 0.5f), QNAN); same("powf(-2,1.5)", plm_powf(-2.f, 1.5f), QNAN);
    same("powf(-2,3)", plm_powf(-2.f, 3.f), -8.f); same("powf(-2,2)", plm_powf(-2.f, 2.f), 4.f); same("powf(-2,-2)", plm_powf(-2.f, -2.f), 0.25f);
    same("powf(2,10)", plm_powf(2.f, 10.f), 1024.f); same("powf(4,0.5)", plm_powf(4.f, 0.5f), 2.f); same("powf(4,1.5)", plm_powf(4.f, 1.5f), 8.f);
    same("powf(2,128)", plm_powf(2.f, 128.f), INF); same("powf(2,-151)", plm_powf(2.f, -151.f), 0.f); same("powf(2,-149)", plm_powf(2.f, -149.f), 1.40129846e-45f);
    same("powf(-1,inf)", plm_powf(-1.f, INF), 1.f); same("powf(0.5,inf)", plm_powf(0.5f, INF), 0.f); same("powf(0.5,-inf)", plm_powf(0.5f, -INF), INF); same("powf(2,inf)", plm_powf(2.f, INF), INF);
    same("powf(inf,2)", plm_powf(INF, 2.f), INF); same("powf(inf,-2)", plm_powf(INF, -2.f), 0.f); same("powf(-inf,3)", plm_powf(-INF, 3.f), -INF); same("powf(-inf,2)", plm_powf(-INF, 2.f), INF);
    same("powf(-inf,-3)", plm_powf(-INF, -3.f), -0.f); same("powf(nan,1)", plm_powf(QNAN, 1.f), QNAN); same("powf(2,nan)", plm_powf(2.f, QNAN), QNAN);
    same("powf(-1,16777216)", plm_powf(-1.f, 16777216.f), 1.f);
    // expf
    same("expf(0)", plm_expf(0.f), 1.f); same("expf(-0)", plm_expf(-0.f), 1.f); same("expf(89)", plm_expf(89.f), INF); same("expf(inf)", plm_expf(INF), INF);
    same("expf(-104)", plm_expf(-104.f), 0.f); same("expf(-inf)", plm_expf(-INF), 0.f); same("expf(-1e30)", plm_expf(-1e30f), 0.f); same("expf(nan)", plm_expf(QNAN), QNAN);
    same("expf(88.72283)", plm_expf(88.72283f), float(std::exp(double(88.72283f))));
}

}  // namespace

int main() {
    edges();
    const unsigned long long n_edges = g_checked;
    const int N = 1 << 20;
    uint64_t seed = 20240911ull;
    for (int i = 0; i < N; ++i) {
        const int part = i & 3;
        const float x = part == 0 ? range(seed, -7.0, 7.0) : part == 1 ? float(std::exp(range(seed, -69.0, 11.5))) * (mix(seed) & 1 ? 1.f : -1.f) : range(seed, -1e5, 1e5);
        near(0, "sinf", x, 0, plm_sinf(x), std::sin(double(x)));
        near(1, "cosf", x, 0, plm_cosf(x), std::cos(double(x)));
        float s, c; plm_sincosf(x, &s, &c);
        near(2, "sincosf", x, 0, s, std::sin(double(x))); near(2, "sincosf", x, 1, c, std::cos(double(x)));
        const float u = part == 0 ? float(1.0 - std::exp(range(seed, -18.0, 0.0))) * (mix(seed) & 1 ? 1.f : -1.f) : range(seed, -1.0, 1.0);
        near(3, "acosf", u, 0, plm_acosf(u), std::acos(double(u)));
        const float sc = float(std::exp(range(seed, -46.0, 46.0)));
        const float y = range(seed, -1.0, 1.0) * sc, xx = range(seed, -1.0, 1.0) * (part == 0 ? float(std::exp(range(seed, -46.0, 46.0))) : sc);
        near(4, "atan2f", y, xx, plm_atan2f(y, xx), std::atan2(double(y), double(xx)));
        float base, expo;
        if (part == 0) { base = range(seed, 0.0, 1.0); expo = float(std::exp(range(seed, -6.9, 9.2))); }                // Blinn's D and pdf
        else if (part == 1) { base = range(seed, 0.0, 1.0); expo = 1.f / (1.f + float(std::exp(range(seed, -6.9, 9.2)))); }   // Blinn's sampled cosine
        else if (part == 2) { base = range(seed, 0.0, 4.0); expo = 1.5f; }                                               // the phase function
        else { base = float(std::exp(range(seed, -23.0, 23.0))); expo = range(seed, -10.0, 10.0); }
        near(5, "powf", base, expo, plm_powf(base, expo), std::pow(double(base), double(expo)));
        const float t = part == 0 ? range(seed, -1.0, 1.0) : range(seed, -104.0, 89.0);
        near(6, "expf", t, 0, plm_expf(t), std::exp(double(t)));
    }
    if (g_failed) { std::fprintf(stderr, "plm_host_test: %llu failures\n", g_failed); return 1; }
    std::printf("plm_host_test: ok (%llu edges, %d arguments per function; worst ulp sinf %.4f cosf %.4f sincosf %.4f acosf %.4f atan2f %.4f powf %.4f expf %.4f)\n",
                n_edges, N, worst[0], worst[1], worst[2], worst[3], worst[4], worst[5], worst[6]);
    return 0;
}
