// oracle/plm_lib.cpp -- TEST INFRASTRUCTURE.  The portable libm functions (pbrt-v1_amd/csrc/hip/rt_libm_portable.h) alone, compiled by g++
// with the reference's floating-point flags into oracle/_build/libplm.so for ctypes: what the host tests measure against float64 and
// what the device's results are compared with bit for bit.  plm_eval runs one function over arrays (fn: 0 sinf, 1 cosf, 2 sincosf,
// 3 acosf, 4 atan2f, 5 powf, 6 expf; b is the second argument of atan2f(a, b) / powf(a, b); out2 receives sincosf's cosine).
#include <stddef.h>

#include "../pbrt-v1_amd/csrc/hip/rt_libm_portable.h"

#define PLM_EXPORT extern "C" __attribute__((visibility("default")))

PLM_EXPORT float plm_c_sinf(float x) { return plm_sinf(x); }
PLM_EXPORT float plm_c_cosf(float x) { return plm_cosf(x); }
PLM_EXPORT void plm_c_sincosf(float x, float *s, float *c) { plm_sincosf(x, s, c); }
PLM_EXPORT float plm_c_acosf(float x) { return plm_acosf(x); }
PLM_EXPORT float plm_c_atan2f(float y, float x) { return plm_atan2f(y, x); }
PLM_EXPORT float plm_c_powf(float x, float y) { return plm_powf(x, y); }
PLM_EXPORT float plm_c_expf(float x) { return plm_expf(x); }

PLM_EXPORT int plm_eval(int fn, const float *a, const float *b, float *out, float *out2, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        switch (fn) {
            case 0: out[i] = plm_sinf(a[i]); break;
            case 1: out[i] = plm_cosf(a[i]); break;
            case 2: plm_sincosf(a[i], &out[i], &out2[i]); break;
            case 3: out[i] = plm_acosf(a[i]); break;
            case 4: out[i] = plm_atan2f(a[i], b[i]); break;
            case 5: out[i] = plm_powf(a[i], b[i]); break;
            case 6: out[i] = plm_expf(a[i]); break;
            default: return 1;
        }
    }
    return 0;
}
