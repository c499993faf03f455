// oracle/ref/portable_libm.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// C-linkage definitions of the libm functions the reference's render phase calls: sinf, cosf, sincosf (what GCC makes of a sinf / cosf
// pair of one argument), acosf, atan2f, powf, expf.  Linked into oracle/_ref/pbrt_ref_keyed_plm ahead of -lm with -rdynamic, so the
// executable's definitions are the ones the core and every dlopen()ed plugin bind to.  No reference source is modified, nothing is preloaded.
//
// Until plm_enable(1) each forwards to the C library's own function (dlsym(RTLD_NEXT, ...)): scene set-up -- transforms, cone cosines,
// quadric thetas, filter tables, shape refinement -- runs under glibc, as the product's host front end does.  keyed_rng_set_key() enables
// the portable functions (pbrt-v1_amd/csrc/hip/rt_libm_portable.h) at the first camera sample: from there on the reference computes what
// the device library's -DRT_PORTABLE_LIBM build computes, bit for bit.  Calls after enabling are counted per function.
#include <dlfcn.h>

#include "../../pbrt-v1_amd/csrc/hip/rt_libm_portable.h"

namespace {
int g_on = 0;
unsigned long long g_calls[7];      // sinf cosf sincosf acosf atan2f powf expf
template <class F> F next(const char *name) {
    void *p = dlsym(RTLD_NEXT, name);
    if (!p) __builtin_trap();
    return reinterpret_cast<F>(p);
}
}  // namespace

extern "C" {
void plm_enable(int on) { g_on = on; }
int plm_enabled() { return g_on; }
const unsigned long long *plm_call_counts() { return g_calls; }

float sinf(float x) noexcept {
    if (g_on) { ++g_calls[0]; return plm_sinf(x); }
    static float (*f)(float) = next<float (*)(float)>("sinf");
    return f(x);
}
float cosf(float x) noexcept {
    if (g_on) { ++g_calls[1]; return plm_cosf(x); }
    static float (*f)(float) = next<float (*)(float)>("cosf");
    return f(x);
}
void sincosf(float x, float *s, float *c) noexcept {
    if (g_on) { ++g_calls[2]; plm_sincosf(x, s, c); return; }
    static void (*f)(float, float *, float *) = next<void (*)(float, float *, float *)>("sincosf");
    f(x, s, c);
}
float acosf(float x) noexcept {
    if (g_on) { ++g_calls[3]; return plm_acosf(x); }
    static float (*f)(float) = next<float (*)(float)>("acosf");
    return f(x);
}
float atan2f(float y, float x) noexcept {
    if (g_on) { ++g_calls[4]; return plm_atan2f(y, x); }
    static float (*f)(float, float) = next<float (*)(float, float)>("atan2f");
    return f(y, x);
}
float powf(float x, float y) noexcept {
    if (g_on) { ++g_calls[5]; return plm_powf(x, y); }
    static float (*f)(float, float) = next<float (*)(float, float)>("powf");
    return f(x, y);
}
float expf(float x) noexcept {
    if (g_on) { ++g_calls[6]; return plm_expf(x); }
    static float (*f)(float) = next<float (*)(float)>("expf");
    return f(x);
}
}
