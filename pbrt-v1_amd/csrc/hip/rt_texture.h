// rt_texture.h -- textured material parameters on the device (EXT kernels only): the (u, v) of a hit, the evaluation of a
// parameter's texture program and the per-hit resolve of the material.  The arithmetic is include/pbrt_hip_texture.h's -- the
// definition the host uses -- compiled for the device.
//
// A resolved material is a VALUE, but the BSDF functions keep taking a MatRef: the value is written once, where the vertex is
// made, into the room `materials` has behind the scene's own records -- one record per thread (or pipeline slot) and recursion
// level, DevFrame::mat_pool_base -- and Vertex::mat becomes its index.  The index travels wherever the vertex's material index
// travelled before (recursion frames, the bidirectional paths, the pipeline's slot state), RT_MAT(sc, v.mat) reads either kind, and
// no kernel keeps 21 more registers alive between two rays.  The record of level L is rewritten only by the next vertex made at
// level L, which is never alive together with this one (a child vertex lives one level up).
#pragma once
#include "rt_shade.h"

namespace rt {

// dg.p, dg.u, dg.v of the hit: ray(t) and Triangle::Intersect's (u, v) (trianglemesh.cpp:269-274) with the mesh's uvs or GetUVs' defaults (:321-326),
// which GetShadingGeometry hands on unchanged (:130-132); a quadric's ObjectToWorld(phit) and its own parameterisation (sphere.cpp:146-148,
// disk.cpp:86-88, cylinder.cpp:106-107, cone.cpp:99-100, paraboloid.cpp:101-102, hyperboloid.cpp:107,:130).  The point is make_vertex's, expression
// for expression.
RT_DEV void hit_point_uv(const DevScene &sc, const Trav &tv, unsigned bits, RtTexHit &h) {
    const unsigned prim = unsigned(tv.hit_prim);
    if (bits & RT_PRIM_QUADRIC) {
        const DevQuadric RT_G &q = RT_GPTR(const DevQuadric, sc.quadrics)[__float_as_uint(RT_GPTR(const DevTri, sc.tris)[prim].q0.x)];
        const V3 o = xform_point(q.w2o, tv.o), d = xform_vector(q.w2o, tv.d);
        const V3 phit = o + d * tv.maxt;                                         // as quadric_frame re-derives it
        const V3 pw = xform_point(q.o2w, phit);
        h.p[0] = pw.x; h.p[1] = pw.y; h.p[2] = pw.z;
        h.u = quadric_phi(q, phit) / q.phi_max;
        if (q.type == RT_QUADRIC_DISK) h.v = 1.f - ((sqrtf(phit.x * phit.x + phit.y * phit.y) - q.zmax) / (q.radius - q.zmax));
        else if (q.type == RT_QUADRIC_CONE) h.v = phit.z / q.zmax;
        else if (q.type == RT_QUADRIC_HYPERBOLOID) h.v = (phit.z - q.p1[2]) / (q.p2[2] - q.p1[2]);
        else if (q.type == RT_QUADRIC_SPHERE) h.v = (rt_acosf(clampf(phit.z / q.radius, -1.f, 1.f)) - q.theta_min) / (q.theta_max - q.theta_min);
        else h.v = (phit.z - q.zmin) / (q.zmax - q.zmin);                        // cylinder, paraboloid
        return;
    }
    const V3 pw = tv.o + tv.d * tv.maxt;                                         // ray(t), geometry.h:210
    h.p[0] = pw.x; h.p[1] = pw.y; h.p[2] = pw.z;
    float u0 = 0.f, v0 = 0.f, u1 = 1.f, v1 = 0.f, u2 = 1.f, v2 = 1.f;
    const int RT_G *idx = RT_GPTR(const int, sc.tex_uv_idx);
    if (idx) {
        const int k = idx[prim];
        if (k >= 0) {
            const float RT_G *r = RT_GPTR(const float, sc.tex_uv) + size_t(6) * unsigned(k);
            u0 = r[0]; v0 = r[1]; u1 = r[2]; v1 = r[3]; u2 = r[4]; v2 = r[5];
        }
    }
    const float b0 = 1 - tv.b1 - tv.b2;
    h.u = b0 * u0 + tv.b1 * u1 + tv.b2 * u2;
    h.v = b0 * v0 + tv.b1 * v1 + tv.b2 * v2;
}

// The evaluation and the resolve, out of line: a function of its own with its own register budget, called only for a hit on a primitive whose
// material has a textured parameter.  Everything goes in by value (the ray and the hit are the caller's registers; a reference would put them in memory).
// Inlined, this code cost every EXT kernel 1 - 8 VGPRs at its peak, spills in the two that sit at the 168-register step and a wave per SIMD in four
// others -- paid by every untextured EXT frame.  Returns the index of the record the resolved material was written to.
__device__ __attribute__((noinline)) int resolve_textured_hit(const DevScene *scp, const DevFrame *frp, unsigned bits, int prim, float ox, float oy, float oz,
                                                              float dx, float dy, float dz, float maxt, float b1, float b2, int level, unsigned gtid) {
    const DevScene &sc = *scp;
    const DevFrame &fr = *frp;
    Trav tv;
    tv.hit_prim = prim; tv.o = mk3(ox, oy, oz); tv.d = mk3(dx, dy, dz); tv.maxt = maxt; tv.b1 = b1; tv.b2 = b2;
    const DevMatTex RT_G &mt = RT_GPTR(const DevMatTex, sc.mat_tex)[bits & 0xffffu];
    RtTexHit h;
    hit_point_uv(sc, tv, bits, h);
    RtMaterialParams P;
    P.type = mt.raw.type; P.f = mt.raw.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) { P.c[s][0] = mt.raw.c[s][0]; P.c[s][1] = mt.raw.c[s][1]; P.c[s][2] = mt.raw.c[s][2]; }
#pragma unroll
    for (int s = 0; s < RT_MATSLOT_COUNT; ++s) {                                  // (unrolled: the slot is a compile-time index, P stays in registers)
        const int len = mt.prog_len[s];
        if (len == 0) continue;
        const RtTexture RT_G *nodes = RT_GPTR(const RtTexture, sc.tex_nodes);
        const int32_t RT_G *prog = RT_GPTR(const int32_t, sc.tex_prog) + mt.prog_off[s];
        if (s == RT_MATSLOT_F) P.f = rt_texture_eval_program(nodes, prog, len, &h, 0);
        else {
#pragma unroll 1
            for (int ch = 0; ch < 3; ++ch) {                                      // one channel at a time (include/pbrt_hip_texture.h)
                const float val = rt_texture_eval_program(nodes, prog, len, &h, ch);
                if (ch == 0) P.c[s][0] = val; else if (ch == 1) P.c[s][1] = val; else P.c[s][2] = val;
            }
        }
    }
    RtMaterial m;
    rt_material_from_params(&P, &m);
    RtMaterialResolved r;
    rt_material_resolve(&m, &r);
    const unsigned handle = fr.mat_pool_base + unsigned(level) * fr.n_threads + gtid;
    RT_GPTR(DevMaterial, sc.materials)[handle] = r;
    return int(handle);
}

// BEFORE make_vertex: when the material of the primitive hit has a textured parameter, evaluate those parameters at the hit, resolve the material into
// the record of (level, thread) and return the record's index -- what Vertex::mat becomes --, else -1.  `level`: the recursion level (path vertex, for
// the bidirectional integrator) the vertex will live at.  The test costs a scene without textures nothing: the word is the one make_vertex reads anyway.
RT_DEV int resolve_hit_material(const DevScene &sc, const DevFrame &fr, const Trav &tv, int level, unsigned gtid) {
    const unsigned bits = __float_as_uint(RT_GPTR(const float4, sc.tri_shade)[size_t(2) * unsigned(tv.hit_prim)].w);
    if (!(bits & RT_PRIM_TEXTURED)) return -1;
    return resolve_textured_hit(&sc, &fr, bits, tv.hit_prim, tv.o.x, tv.o.y, tv.o.z, tv.d.x, tv.d.y, tv.d.z, tv.maxt, tv.b1, tv.b2, level, gtid);
}

}  // namespace rt
