/* pbrt_hip_texture.h -- textured material parameters: the texture node table handed over with rt_scene_set_textures, its
 * evaluation at a hit (p, u, v) and the resolve of a material from its evaluated parameters.  One definition for the device
 * (the EXT kernels evaluate and resolve per hit, rt_texture.h), for rt_scene_create (materials without a textured slot are
 * resolved once on the host, as before) and for the host front end (ParsedScene.eval_texture(), makeMaterial).  Everything is
 * float32 in the reference's order of operations: compile without floating-point contraction.
 *
 * Texture classes (textures/{constant,scale,mix,bilerp,uv,checkerboard}.cpp) whose value depends on the hit alone; the four
 * 2-D mappings of core/texture.cpp:63-149.  No texture differentials exist here: a checkerboard is the point-sampled form
 * (aamode "none", checkerboard.cpp:119-122). */
#ifndef PBRT_HIP_TEXTURE_H
#define PBRT_HIP_TEXTURE_H
#include <math.h>
#include "pbrt_hip.h"
#include "pbrt_hip_material.h"

#if defined(__HIPCC__)
#define RT_TEX_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define RT_TEX_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_TEX_MEM __attribute__((address_space(1)))    /* the node table is read with global loads on the device */
#else
#define RT_TEX_MEM
#endif

/* limits of rt_scene_set_textures (beyond them: RT_EINVAL, never a truncated graph) */
#define RT_TEX_MAX_NODES 65536   /* nodes in the table                                                               */
#define RT_TEX_MAX_PROGRAM 32    /* nodes of one parameter's graph, counted as a tree (a shared node counts per use) */
#define RT_TEX_MAX_STACK 4       /* values alive at once while the post-order program of one parameter is evaluated  */

/* what rt_scene_create derives from an RtMaterial: the record the kernels read (DevMaterial, rt_device.h) */
typedef struct RtMaterialResolved {
    int32_t type;
    float r[3];        /* Kd / Kr                                                                                       */
    float t[3];        /* Kt                                                                                            */
    float on_a, on_b;  /* Oren-Nayar A, B (reflection.h:268-277); on_b < 0 => Lambertian                                */
    float ior;
    int32_t has_r, has_t;  /* glass.cpp:56-61: a lobe exists only if its colour is not black                            */
    float ks[3];       /* plastic: Microfacet reflectance                                                               */
    float exponent;    /* Blinn exponent = 1/roughness, capped at 1000 (reflection.h:313)                               */
    float kr[3];       /* uber: SpecularReflection reflectance (Fresnel 1.5 / 1)                                        */
    int32_t has_g, has_kr; /* glossy / specular-reflection lobes present (non-black, uber.cpp:71-86)                    */
    /* shinymetal: ks = FresnelApproxEta(Ks), kr = FresnelApproxEta(Kr), exponent.  translucent: r = reflect*Kd, t = transmit*Kd,
     * ks = reflect*Ks, kr = transmit*Ks; lobes present has_r (diffuse R), has_t (diffuse T), has_g (glossy R), has_kr (glossy T) */
} RtMaterialResolved;

/* the raw parameters of a material, as GetSpectrumTexture / GetFloatTexture deliver them (nothing clamped or multiplied yet).
 * Slots by material:     c[0]   c[1]  c[2]     c[3]      f
 *   matte                Kd                              sigma
 *   mirror               Kr
 *   glass                Kr     Kt                       index
 *   plastic              Kd     Ks                       roughness
 *   uber                 Kd     Ks    Kr       opacity   roughness
 *   shinymetal                  Ks    Kr                 roughness
 *   translucent          Kd     Ks    reflect  transmit  roughness                                                    */
enum { RT_MATSLOT_C0 = 0, RT_MATSLOT_C1 = 1, RT_MATSLOT_C2 = 2, RT_MATSLOT_C3 = 3, RT_MATSLOT_F = 4, RT_MATSLOT_COUNT = 5 };
typedef struct RtMaterialParams {
    int32_t type;      /* RT_MAT_* */
    float c[4][3];
    float f;
} RtMaterialParams;
/* per material: the raw parameters (literals / defaults / folded constant textures) and, per slot, the texture node that
 * replaces it at every hit, or -1 */
typedef struct RtMaterialTextures {
    RtMaterialParams raw;
    int32_t tex[RT_MATSLOT_COUNT];
} RtMaterialTextures;

enum { RT_TEX_CONSTANT = 0, RT_TEX_SCALE = 1, RT_TEX_MIX = 2, RT_TEX_BILERP = 3, RT_TEX_UV = 4, RT_TEX_CHECKERBOARD = 5, RT_TEX_KIND_COUNT = 6 };
enum { RT_TEXMAP_UV = 0, RT_TEXMAP_SPHERICAL = 1, RT_TEXMAP_CYLINDRICAL = 2, RT_TEXMAP_PLANAR = 3, RT_TEXMAP_COUNT = 4 };
typedef struct RtTexture {
    int32_t kind;          /* RT_TEX_*                                                                                   */
    int32_t is_color;      /* 0: Texture<float>, 1: Texture<Spectrum>.  A float value travels as (f, f, f)               */
    int32_t mapping;       /* RT_TEXMAP_* (bilerp, uv, checkerboard)                                                     */
    int32_t child[3];      /* tex1, tex2 (scale, mix, checkerboard), amount (mix): indices BELOW this node's, or -1      */
    float value[12];       /* constant: value (a float in all three);  bilerp: v00, v01, v10, v11                        */
    float map[8];          /* uv: su, sv, du, dv;  planar: vs.xyz, vt.xyz, ds, dt                                        */
    float world_to_texture[16]; /* spherical / cylindrical: the inverse of the CTM at the Texture statement, row-major   */
} RtTexture;

/* ---- materials: parameters -> RtMaterial (what the material's GetBSDF does first) -> RtMaterialResolved ---- */
RT_TEX_FN float rt_tex_clamp0(float v) { return v < 0.f ? 0.f : v; }                             /* Spectrum::Clamp() color.h */
/* matte.cpp:46-64, mirror.cpp:42-55, glass.cpp:46-63, plastic.cpp:47-69, uber.cpp:52-89, shinymetal.cpp:43-73, translucent.cpp:45-94 */
RT_TEX_FN void rt_material_from_params(const RtMaterialParams *p, RtMaterial *m) {
    int c;
    const int type = p->type;
    m->type = type; m->sigma = 0.f; m->ior = 1.f; m->roughness = 0.f;
    for (c = 0; c < 3; ++c) { m->kd[c] = m->kt[c] = m->ks[c] = m->kr[c] = 0.f; }
    if (type == RT_MAT_MATTE) {
        const float sig = p->f;
        for (c = 0; c < 3; ++c) m->kd[c] = rt_tex_clamp0(p->c[0][c]);
        m->sigma = sig < 0.f ? 0.f : (sig > 90.f ? 90.f : sig);                                   /* Clamp(sigma, 0, 90) */
    } else if (type == RT_MAT_MIRROR) {
        for (c = 0; c < 3; ++c) m->kd[c] = rt_tex_clamp0(p->c[0][c]);
    } else if (type == RT_MAT_GLASS) {
        for (c = 0; c < 3; ++c) { m->kd[c] = rt_tex_clamp0(p->c[0][c]); m->kt[c] = rt_tex_clamp0(p->c[1][c]); }
        m->ior = p->f;
    } else if (type == RT_MAT_PLASTIC) {
        for (c = 0; c < 3; ++c) { m->kd[c] = rt_tex_clamp0(p->c[0][c]); m->ks[c] = rt_tex_clamp0(p->c[1][c]); }
        m->roughness = p->f;
    } else if (type == RT_MAT_UBER) {                                                             /* uber.cpp:62-87 */
        for (c = 0; c < 3; ++c) {
            const float kd = rt_tex_clamp0(p->c[0][c]), ks = rt_tex_clamp0(p->c[1][c]), kr = rt_tex_clamp0(p->c[2][c]), op = rt_tex_clamp0(p->c[3][c]);
            m->kt[c] = -op + 1.f;                                                                 /* SpecularTransmission(-op + Spectrum(1.), 1., 1.) */
            m->kd[c] = op * kd; m->ks[c] = op * ks; m->kr[c] = op * kr;
        }
        m->roughness = p->f;
    } else if (type == RT_MAT_SHINYMETAL) {
        for (c = 0; c < 3; ++c) { m->ks[c] = rt_tex_clamp0(p->c[1][c]); m->kr[c] = rt_tex_clamp0(p->c[2][c]); }
        m->roughness = p->f;
    } else {                                                                                      /* translucent: kr = reflect, kt = transmit */
        for (c = 0; c < 3; ++c) {
            m->kd[c] = rt_tex_clamp0(p->c[0][c]); m->ks[c] = rt_tex_clamp0(p->c[1][c]);
            m->kr[c] = rt_tex_clamp0(p->c[2][c]); m->kt[c] = rt_tex_clamp0(p->c[3][c]);
        }
        m->roughness = p->f;
    }
}
RT_TEX_FN float rt_blinn_exponent(float roughness) {                                              /* 1.f / rough; Blinn ctor reflection.h:313 */
    float e = 1.f / roughness;
    if (e > 1000.f || e != e) e = 1000.f;
    return e;
}
RT_TEX_FN void rt_material_resolve(const RtMaterial *m, RtMaterialResolved *o) {
    int c;
    o->type = m->type; o->ior = m->ior; o->on_a = 1.f; o->on_b = -1.f;
    for (c = 0; c < 3; ++c) { o->r[c] = m->kd[c]; o->t[c] = m->kt[c]; o->ks[c] = m->ks[c]; o->kr[c] = m->kr[c]; }
    o->has_r = !rt_color_black(m->kd); o->has_t = !rt_color_black(m->kt);
    o->has_g = !rt_color_black(m->ks); o->has_kr = !rt_color_black(m->kr);
    o->exponent = 0.f;
    if (m->type == RT_MAT_PLASTIC || m->type == RT_MAT_UBER) o->exponent = rt_blinn_exponent(m->roughness);
    if (m->type == RT_MAT_SHINYMETAL || m->type == RT_MAT_TRANSLUCENT) {
        RtMaterialLobes lb;
        const int shiny = m->type == RT_MAT_SHINYMETAL;
        rt_material_lobes(m, &lb);
        for (c = 0; c < 3; ++c) {
            o->r[c] = lb.r_kd[c]; o->t[c] = lb.t_kd[c];
            o->ks[c] = shiny ? lb.eta_ks[c] : lb.r_ks[c]; o->kr[c] = shiny ? lb.eta_kr[c] : lb.t_ks[c];
        }
        o->has_r = lb.has_dr; o->has_t = lb.has_dt; o->has_g = lb.has_gr; o->has_kr = lb.has_gt;
        o->exponent = rt_blinn_exponent(m->roughness);
    }
    if (m->type == RT_MAT_MATTE && m->sigma != 0.f) {                                             /* OrenNayar ctor reflection.h:268-277 */
        const float sigma = (3.14159265358979323846f / 180.f) * m->sigma;
        const float sigma2 = sigma * sigma;
        o->on_a = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
        o->on_b = 0.45f * sigma2 / (sigma2 + 0.09f);
    }
}

/* ---- texture evaluation ---- */
typedef struct RtTexHit { float p[3]; float u, v; } RtTexHit;      /* dg.p (world), dg.u, dg.v */

RT_TEX_FN int rt_tex_floor2int(float v) { return (int)floorf(v); } /* Floor2Int without FAST_INT: (int)floor(double(v)), the same integer */

/* TextureMapping2D::Map, s and t only (core/texture.cpp:68-72, :97-105, :125-131, :139-144) */
RT_TEX_FN void rt_texture_map(const RtTexture RT_TEX_MEM *n, const RtTexHit *h, float *s, float *t) {
    const int mapping = n->mapping;
    if (mapping == RT_TEXMAP_UV) {
        *s = n->map[0] * h->u + n->map[2];
        *t = n->map[1] * h->v + n->map[3];
    } else if (mapping == RT_TEXMAP_PLANAR) {
        *s = n->map[6] + (h->p[0] * n->map[0] + h->p[1] * n->map[1] + h->p[2] * n->map[2]);
        *t = n->map[7] + (h->p[0] * n->map[3] + h->p[1] * n->map[4] + h->p[2] * n->map[5]);
    } else {
        /* Normalize(WorldToTexture(p) - Point(0,0,0)): Transform::operator()(Point) divides by w unless it is 1 (transform.h:69-80) */
        const float RT_TEX_MEM *m = n->world_to_texture;
        float x = m[0] * h->p[0] + m[1] * h->p[1] + m[2] * h->p[2] + m[3];
        float y = m[4] * h->p[0] + m[5] * h->p[1] + m[6] * h->p[2] + m[7];
        float z = m[8] * h->p[0] + m[9] * h->p[1] + m[10] * h->p[2] + m[11];
        const float w = m[12] * h->p[0] + m[13] * h->p[1] + m[14] * h->p[2] + m[15];
        float inv;
        if (w != 1.f) { const float iw = 1.f / w; x = x * iw; y = y * iw; z = z * iw; }
        inv = 1.f / sqrtf(x * x + y * y + z * z);                                                 /* Vector::operator/ multiplies by 1.f / length */
        x = x * inv; y = y * inv; z = z * inv;
        if (mapping == RT_TEXMAP_SPHERICAL) {
            const float theta = acosf(z < -1.f ? -1.f : (z > 1.f ? 1.f : z));                     /* SphericalTheta geometry.h:403-405 */
            const float p = atan2f(y, x);                                                         /* SphericalPhi :406-409: 2.f*M_PI is a double */
            const float phi = (p < 0.f) ? (float)((double)p + 2.f * 3.14159265358979323846) : p;
            *s = theta * 0.31830988618379067154f;                                                 /* INV_PI, INV_TWOPI: floats */
            *t = phi * 0.15915494309189533577f;
        } else {
            *s = (float)((3.14159265358979323846 + (double)atan2f(y, x)) / (2.f * 3.14159265358979323846));   /* M_PI is a double */
            *t = z;
        }
    }
}

/* Every class computes a colour channel from the same channel of its children (a float value is the same in all three, so mix's amount is too):
 * values are evaluated one channel at a time, which keeps the evaluation's state to a handful of scalars.
 * One node, channel ch, whose children's values are known: a = tex1, b = tex2, c = amount */
RT_TEX_FN float rt_texture_node(const RtTexture RT_TEX_MEM *n, const RtTexHit *h, int ch, float a, float b, float c) {
    const int kind = n->kind;
    if (kind == RT_TEX_CONSTANT) return n->value[ch];
    if (kind == RT_TEX_SCALE) return a * b;                                                       /* scale.cpp: tex1 * tex2 */
    if (kind == RT_TEX_MIX) return (1.f - c) * a + c * b;                                         /* mix.cpp */
    {
        float s, t;
        rt_texture_map(n, h, &s, &t);
        if (kind == RT_TEX_BILERP)                                                                /* bilerp.cpp: four terms, summed left to right */
            return ((((1 - s) * (1 - t)) * n->value[ch] + ((1 - s) * t) * n->value[3 + ch]) + (s * (1 - t)) * n->value[6 + ch]) + (s * t) * n->value[9 + ch];
        if (kind == RT_TEX_UV)                                                                    /* uv.cpp: (s - floor s, t - floor t, 0) */
            return ch == 0 ? s - (float)rt_tex_floor2int(s) : (ch == 1 ? t - (float)rt_tex_floor2int(t) : 0.f);
        return ((rt_tex_floor2int(s) + rt_tex_floor2int(t)) % 2 == 0) ? a : b;                    /* checkerboard.cpp:119-122 */
    }
}

/* Evaluate channel ch of a parameter's post-order program (node indices, children before parents; rt_scene_set_textures makes them and
 * guarantees that the stack of RT_TEX_MAX_STACK values suffices).  The stack is four named values that shift: nothing is indexed at run time. */
RT_TEX_FN float rt_texture_eval_program(const RtTexture RT_TEX_MEM *nodes, const int32_t RT_TEX_MEM *prog, int len, const RtTexHit *h, int ch) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i;
    for (i = 0; i < len; ++i) {
        const RtTexture RT_TEX_MEM *n = nodes + prog[i];
        const int kind = n->kind;
        if (kind == RT_TEX_MIX) {                                   /* stack: tex1 = s2, tex2 = s1, amount = s0 */
            s0 = rt_texture_node(n, h, ch, s2, s1, s0); s1 = s3;
        } else if (kind == RT_TEX_SCALE || kind == RT_TEX_CHECKERBOARD) {   /* tex1 = s1, tex2 = s0 */
            s0 = rt_texture_node(n, h, ch, s1, s0, 0.f); s1 = s2; s2 = s3;
        } else {                                                    /* a leaf: push */
            const float r = rt_texture_node(n, h, ch, 0.f, 0.f, 0.f);
            s3 = s2; s2 = s1; s1 = s0; s0 = r;
        }
    }
    return s0;
}
#endif
