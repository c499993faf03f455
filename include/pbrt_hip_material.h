/* pbrt_hip_material.h -- what rt_scene_create derives from an RtMaterial of type RT_MAT_SHINYMETAL / RT_MAT_TRANSLUCENT before
 * the device sees it: everything that depends on the parameters alone, computed once in the reference's float order.
 * One definition for the device library (rt_scene.hip) and the host front end (ParsedScene.materials()), so that the
 * two cannot drift apart.  Compile without floating-point contraction. */
#ifndef PBRT_HIP_MATERIAL_H
#define PBRT_HIP_MATERIAL_H
#include <math.h>
#include "pbrt_hip.h"
#if defined(__HIPCC__)
#define RT_MAT_FN __host__ __device__ static inline    /* the EXT kernels derive the same values per hit for a textured material */
#else
#define RT_MAT_FN static inline
#endif

typedef struct RtMaterialLobes {
    float eta_ks[3], eta_kr[3];                 /* shinymetal: FresnelApproxEta(Ks), FresnelApproxEta(Kr) (shinymetal.cpp:57-58) */
    float r_kd[3], t_kd[3], r_ks[3], t_ks[3];   /* translucent: reflect*Kd, transmit*Kd, reflect*Ks, transmit*Ks (translucent.cpp:59-77) */
    int32_t has_dr, has_dt, has_gr, has_gt;     /* lobes present: diffuse R, diffuse T, glossy R, glossy T (shinymetal: glossy R and, in has_gt, specular R) */
} RtMaterialLobes;

/* FresnelApproxEta core/reflection.cpp:52-56: Clamp(0, .999), (1 + sqrt) / (1 - sqrt) */
RT_MAT_FN float rt_fresnel_approx_eta(float fr) {
    const float reflectance = fr < 0.f ? 0.f : (fr > .999f ? .999f : fr);
    return (1.f + sqrtf(reflectance)) / (1.f - sqrtf(reflectance));
}
RT_MAT_FN int rt_color_black(const float *c) { return c[0] == 0.f && c[1] == 0.f && c[2] == 0.f; }   /* Spectrum::Black color.h */

RT_MAT_FN void rt_material_lobes(const RtMaterial *m, RtMaterialLobes *o) {
    int c;
    for (c = 0; c < 3; ++c) { o->eta_ks[c] = o->eta_kr[c] = 0.f; o->r_kd[c] = o->t_kd[c] = o->r_ks[c] = o->t_ks[c] = 0.f; }
    o->has_dr = o->has_dt = o->has_gr = o->has_gt = 0;
    if (m->type == RT_MAT_SHINYMETAL) {
        for (c = 0; c < 3; ++c) { o->eta_ks[c] = rt_fresnel_approx_eta(m->ks[c]); o->eta_kr[c] = rt_fresnel_approx_eta(m->kr[c]); }
        o->has_gr = o->has_gt = 1;
    } else if (m->type == RT_MAT_TRANSLUCENT) {
        const int r = !rt_color_black(m->kr), t = !rt_color_black(m->kt);                 /* translucent.cpp:53-56 */
        const int d = (r || t) && !rt_color_black(m->kd), g = (r || t) && !rt_color_black(m->ks);
        for (c = 0; c < 3; ++c) {
            o->r_kd[c] = m->kr[c] * m->kd[c]; o->t_kd[c] = m->kt[c] * m->kd[c];
            o->r_ks[c] = m->kr[c] * m->ks[c]; o->t_ks[c] = m->kt[c] * m->ks[c];
        }
        o->has_dr = d && r; o->has_dt = d && t; o->has_gr = g && r; o->has_gt = g && t;
    }
}
#endif
