// rt_libm_portable.h -- the six libm functions the render phase calls (and sincosf, which GCC makes of a sinf / cosf pair), written so
// that every compiler and every machine gives the same bits: the argument is widened to double, everything is computed with IEEE
// double + - *, comparisons, integer conversions and bit casts, and the result is rounded to float once.  There is no
// libm call, no division and no square root: a quotient is a Newton reciprocal and a root a Newton reciprocal root, both made of
// + - * from an initial value taken from the bits, so they do not depend on how a target rounds f64 "/" or sqrt.  No contraction: the
// pragmas below say so whatever the command line says.  The error of the double evaluation is below 2^-45 relative, so a result
// is within 0.5 + 2^-20 float ulps of the true value.
//
// HIP-free.  PLM_FN is the one macro: the includer sets it to `__host__ __device__ inline` under hipcc (rt_libm.h); the default is a
// plain host function.  Used by the device library's test build (-DRT_PORTABLE_LIBM), by the CPU oracle's (-DORACLE_PORTABLE_LIBM) and
// by the definitions the compiled reference is linked against (oracle/ref/portable_libm.cpp): one implementation on every side.
//
// Conventions (the callers branch on them):
//   sinf / cosf     exact reduction for |x| <= 1e5 (pi/2 in three 33-bit parts), reduced with growing error up to 2^40 and
//                   sin = 0, cos = 1 beyond; sinf(-0) = -0; NaN or infinite -> NaN.
//   acosf           |x| > 1 -> NaN; acosf(1) = +0; acosf(-1) = float(pi).
//   atan2f          IEEE: all quadrants, signed zeros (atan2f(+-0, x >= +0) = +-0, atan2f(+-0, x <= -0) = +-float(pi)), infinities; NaN -> NaN.
//   powf            powf(x, 0) = 1 and powf(1, y) = 1 for every other argument; powf(+-0, y > 0) = 0 (-0 for -0 and an odd integer y),
//                   powf(+-0, y < 0) = inf; powf(x < 0, y) = NaN unless y is an integer; infinities as IEEE; NaN -> NaN.
//   expf            overflow -> inf, underflow -> denormals and then 0 through the one rounding; expf(-inf) = 0; NaN -> NaN.
#ifndef RT_LIBM_PORTABLE_H
#define RT_LIBM_PORTABLE_H

#ifndef PLM_FN
#define PLM_FN static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

typedef unsigned long long plm_u64;

PLM_FN plm_u64 plm_bits(double d) { plm_u64 u; __builtin_memcpy(&u, &d, 8); return u; }
PLM_FN double plm_from_bits(plm_u64 u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
PLM_FN float plm_float_from_bits(unsigned u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
PLM_FN bool plm_signbit(double d) { return (plm_bits(d) >> 63) != 0; }
PLM_FN double plm_abs(double d) { return plm_from_bits(plm_bits(d) & 0x7fffffffffffffffULL); }
PLM_FN bool plm_isinf(double d) { return (plm_bits(d) & 0x7fffffffffffffffULL) == 0x7ff0000000000000ULL; }
PLM_FN float plm_nan() { return plm_float_from_bits(0x7fc00000u); }
PLM_FN float plm_inf(bool neg) { return plm_float_from_bits(neg ? 0xff800000u : 0x7f800000u); }
PLM_FN double plm_pow2(long long k) { return plm_from_bits((plm_u64)(k + 1023) << 52); }      // -1022 <= k <= 1023

// the one rounding.  What lies at or above FLT_MAX + half an ulp (2^128 - 2^103) is infinite, said here and not left to the conversion.
PLM_FN float plm_round(double v) {
    if (v != v) return plm_nan();
    if (v >= 3.4028235677973366e+38) return plm_inf(false);
    if (v <= -3.4028235677973366e+38) return plm_inf(true);
    return (float)v;
}

// 1 / d for a normal d > 0: the mantissa h in [0.5, 1) starts at 48/17 - 32/17 h (error 1/17) and five Newton steps square it away
PLM_FN double plm_recip(double d) {
    const plm_u64 u = plm_bits(d);
    long long e = (long long)((u >> 52) & 0x7ff);
    if (e < 1) e = 1;
    if (e > 2044) e = 2044;
    const double h = plm_from_bits((u & 0x000fffffffffffffULL) | 0x3fe0000000000000ULL);
    double r = 2.823529411764706 - 1.8823529411764706 * h;
    for (int i = 0; i < 5; ++i) r = r + r * (1.0 - h * r);
    return r * plm_from_bits((plm_u64)(2045 - e) << 52);
}

// sqrt(a) for a >= 0: the reciprocal root from the halved exponent (3.4 % off), five Newton steps, and one step on the root itself
PLM_FN double plm_sqrt(double a) {
    if (!(a > 0.0)) return 0.0;
    double y = plm_from_bits(0x5fe6eb50c7b537a9ULL - (plm_bits(a) >> 1));
    for (int i = 0; i < 5; ++i) y = y * (1.5 - 0.5 * a * y * y);
    double s = a * y;
    s = s + 0.5 * y * (a - s * s);
    return s;
}

// sin and cos of a finite x: k = round(x 2/pi), r = x - k pi/2 with pi/2 = P1 + P2 + P3 (33 + 33 + 53 bits: k P1 and k P2 are exact for
// k < 2^20, i.e. |x| <= 1e6), Taylor polynomials to r^17 / r^16 on |r| <= pi/4 (remainder < 5e-17)
PLM_FN void plm_sincos_core(double x, double* s, double* c) {
    if (plm_abs(x) >= 1099511627776.0) { *s = 0.0; *c = 1.0; return; }
    const double t = x * 0.6366197723675814;
    const long long k = (long long)(t + (t < 0.0 ? -0.5 : 0.5));
    const double kd = (double)k;
    const double r = ((x - kd * 1.5707963267341256) - kd * 6.077100506303966e-11) - kd * 2.0222662487959506e-21;
    const double z = r * r;
    const double sp = r + r * z * (-0.16666666666666666 + z * (0.008333333333333333 + z * (-0.0001984126984126984 + z * (2.7557319223985893e-06 +
                      z * (-2.505210838544172e-08 + z * (1.6059043836821613e-10 + z * (-7.647163731819816e-13 + z * 2.8114572543455206e-15)))))));
    const double cp = 1.0 + z * (-0.5 + z * (0.041666666666666664 + z * (-0.001388888888888889 + z * (2.48015873015873e-05 +
                      z * (-2.755731922398589e-07 + z * (2.08767569878681e-09 + z * (-1.1470745597729725e-11 + z * 4.779477332387385e-14)))))));
    switch ((int)(k & 3)) {
        case 0: *s = sp; *c = cp; break;
        case 1: *s = cp; *c = -sp; break;
        case 2: *s = -sp; *c = -cp; break;
        default: *s = -cp; *c = sp; break;
    }
}

// atan(a / b) for 0 <= a <= b, 0 < b: atan(q) = atan(c) + atan((a - c b) / (b + c a)) with c the nearest of 0, 1/4, .. 1, so the
// remaining argument is at most 1/8 and the series to t^21 leaves less than 2^-63
PLM_FN double plm_atan_ratio(double a, double b) {
    double c, ac;
    const double a8 = 8.0 * a;
    if (a8 < b) { c = 0.0; ac = 0.0; }
    else if (a8 < 3.0 * b) { c = 0.25; ac = 0.24497866312686414; }
    else if (a8 < 5.0 * b) { c = 0.5; ac = 0.4636476090008061; }
    else if (a8 < 7.0 * b) { c = 0.75; ac = 0.6435011087932844; }
    else { c = 1.0; ac = 0.7853981633974483; }
    const double t = (a - c * b) * plm_recip(b + c * a);
    const double z = t * t;
    const double p = t + t * z * (-0.3333333333333333 + z * (0.2 + z * (-0.14285714285714285 + z * (0.1111111111111111 + z * (-0.09090909090909091 +
                     z * (0.07692307692307693 + z * (-0.06666666666666667 + z * (0.058823529411764705 + z * (-0.05263157894736842 + z * 0.047619047619047616)))))))));
    return ac + p;
}

// atan2 of two numbers that are not NaN
PLM_FN double plm_atan2_core(double y, double x) {
    const double PI = 3.141592653589793, PIO2 = 1.5707963267948966;
    const double ay = plm_abs(y), ax = plm_abs(x);
    const bool xneg = plm_signbit(x);
    double r;
    if (ay == 0.0) r = xneg ? PI : 0.0;
    else if (ax == 0.0) r = PIO2;
    else if (plm_isinf(ax)) r = plm_isinf(ay) ? (xneg ? 2.356194490192345 : 0.7853981633974483) : (xneg ? PI : 0.0);
    else if (plm_isinf(ay)) r = PIO2;
    else {
        r = ay <= ax ? plm_atan_ratio(ay, ax) : PIO2 - plm_atan_ratio(ax, ay);
        if (xneg) r = PI - r;
    }
    return plm_signbit(y) ? -r : r;
}

// exp(z), z clamped to +-200 (far beyond float's range either way): k = round(z / ln 2), r = z - k ln2 in two parts, Taylor to r^14
PLM_FN double plm_exp_core(double z) {
    if (z > 200.0) z = 200.0;
    if (z < -200.0) z = -200.0;
    const double t = z * 1.4426950408889634;
    const long long k = (long long)(t + (t < 0.0 ? -0.5 : 0.5));
    const double kd = (double)k;
    const double r = (z - kd * 0.6931471804855391) - kd * 7.440617110012397e-11;
    const double p = 1.0 + r * (1.0 + r * (0.5 + r * (0.16666666666666666 + r * (0.041666666666666664 + r * (0.008333333333333333 + r * (0.001388888888888889 +
                     r * (0.0001984126984126984 + r * (2.48015873015873e-05 + r * (2.7557319223985893e-06 + r * (2.755731922398589e-07 + r * (2.505210838544172e-08 +
                     r * (2.08767569878681e-09 + r * (1.6059043836821613e-10 + r * 1.1470745597729725e-11)))))))))))));
    return p * plm_pow2(k);
}

// log(x) for a normal x > 0: x = m 2^e with m in (sqrt(1/2), sqrt(2)], s = (m - 1) / (m + 1), log m = 2 atanh s to s^25 (|s| <= 0.172)
PLM_FN double plm_log_core(double x) {
    const plm_u64 u = plm_bits(x);
    long long e = (long long)((u >> 52) & 0x7ff) - 1023;
    double m = plm_from_bits((u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL);
    if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }
    const double f = m - 1.0;
    const double s = f * plm_recip(2.0 + f);
    const double z = s * s;
    const double p = 2.0 * s * (1.0 + z * (0.3333333333333333 + z * (0.2 + z * (0.14285714285714285 + z * (0.1111111111111111 + z * (0.09090909090909091 +
                     z * (0.07692307692307693 + z * (0.06666666666666667 + z * (0.058823529411764705 + z * (0.05263157894736842 + z * (0.047619047619047616 +
                     z * (0.043478260869565216 + z * 0.04))))))))))));
    const double ed = (double)e;
    return ed * 0.6931471804855391 + (p + ed * 7.440617110012397e-11);
}

PLM_FN void plm_sincosf(float x, float* s, float* c) {
    const double d = (double)x;
    if (d != d || plm_isinf(d)) { *s = plm_nan(); *c = plm_nan(); return; }
    if (d == 0.0) { *s = x; *c = 1.f; return; }                     // sinf(-0) = -0: the polynomial's r + r z (...) would give +0
    double sd, cd;
    plm_sincos_core(d, &sd, &cd);
    *s = plm_round(sd); *c = plm_round(cd);
}

PLM_FN float plm_sinf(float x) { float s, c; plm_sincosf(x, &s, &c); return s; }
PLM_FN float plm_cosf(float x) { float s, c; plm_sincosf(x, &s, &c); return c; }

PLM_FN float plm_atan2f(float y, float x) {
    if (x != x || y != y) return plm_nan();
    return plm_round(plm_atan2_core((double)y, (double)x));
}

// acos x = atan2(sqrt((1 - x)(1 + x)), x): both factors are exact in double for a float x
PLM_FN float plm_acosf(float x) {
    const double d = (double)x;
    if (d != d || d > 1.0 || d < -1.0) return plm_nan();
    return plm_round(plm_atan2_core(plm_sqrt((1.0 - d) * (1.0 + d)), d));
}

PLM_FN float plm_expf(float x) {
    if (x != x) return plm_nan();
    return plm_round(plm_exp_core((double)x));
}

PLM_FN float plm_powf(float xf, float yf) {
    const double x = (double)xf, y = (double)yf;
    if (y == 0.0 || x == 1.0) return 1.f;
    if (x != x || y != y) return plm_nan();
    const double ax = plm_abs(x), ay = plm_abs(y);
    if (plm_isinf(ay)) {
        if (ax == 1.0) return 1.f;
        return ((ax > 1.0) == (y > 0.0)) ? plm_inf(false) : 0.f;
    }
    bool yint, yodd;
    if (ay >= 16777216.0) { yint = true; yodd = false; }
    else { const long long yi = (long long)y; yint = (double)yi == y; yodd = yint && (yi & 1); }
    const bool neg = plm_signbit(x) && yodd;
    if (ax == 0.0 || plm_isinf(ax)) {
        const bool big = plm_isinf(ax) == (y > 0.0);
        return big ? plm_inf(neg) : (neg ? -0.f : 0.f);
    }
    if (x < 0.0 && !yint) return plm_nan();
    const double r = plm_exp_core(y * plm_log_core(ax));
    return plm_round(neg ? -r : r);
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
#endif
