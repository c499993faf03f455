// rt_bidir.h -- BidirIntegrator::Li (integrators/bidirectional.cpp:80-210) as a persistent kernel of its own: rt::bidir_kernel, instantiated in rt_mega_b.hip.
//
// The integrator builds an eye sub-path and a light sub-path of at most four vertices each and then connects every pair of prefixes, so one camera
// sample casts up to 8 closest-hit rays, 8 EstimateDirect rays and 16 connection rays, in an order no ray result changes.  The kernel runs it in LOCK STEP:
// a wave takes 64 camera samples from the work counter, one per lane, and walks the reference's loops with wave-uniform trip counts -- every "cast a
// ray" of the reference is one shared traversal (rt_traverse.h trace_round, the LDS stacks of the megakernel) of whichever lanes have a ray there.  Lanes
// whose path is shorter idle through the rest of the batch; the per-lane order of operations, sample values and RandomFloat() draws is the reference's.
// The eight vertices do not fit registers: they live in a per-thread HBM record (DevFrame::frames, [field][thread] like the recursion frames, so one
// field of a wave's 64 lanes is one contiguous 256-byte run).
//
// Kept as the reference has them: the light's emitted spectrum is replaced by the grey value nLights / pdf (:107-110), BSDF::f of a
// specular vertex is black so nothing is carried through a mirror, no emitted radiance is added at eye vertices or on escaped rays, the connection's
// bsdf->f takes the unnormalised vector between the vertices, UniformSampleOneLight gets the geometric normal, dAWeight is never read (not computed).
#pragma once
#include "rt_render_kernel.h"

namespace rt {

#define RT_BD_WORDS 21                    // floats of one stored vertex: p, nn, sn, ng, wi, wo, material, bsdfWeight, rrWeight
#define RT_BD_FRAME_WORDS (2 * RT_BD_MAX_VERTS * RT_BD_WORDS)
// (RT_BD_MAX_VERTS and the BidirTable the host packs the integrator's sample requests into: rt_frame_plan.h)

struct BidirVertex { Vertex v; V3 wnext; float bsdfWeight, rrWeight; };      // v.wo is the reference's `wi` (towards the previous vertex), wnext its `wo`

RT_DEV float RT_G *bd_vertex_ptr(const DevFrame &fr, int side, int k, unsigned gtid) {
    return RT_GPTR(float, fr.frames) + size_t((side * RT_BD_MAX_VERTS + k) * RT_BD_WORDS) * fr.n_threads + gtid;
}
RT_DEV void bd_store(const DevFrame &fr, int side, int k, unsigned gtid, const BidirVertex &b) {
    float RT_G *q = bd_vertex_ptr(fr, side, k, gtid); const size_t st = fr.n_threads;
    q[0 * st] = b.v.p.x; q[1 * st] = b.v.p.y; q[2 * st] = b.v.p.z;
    q[3 * st] = b.v.nn.x; q[4 * st] = b.v.nn.y; q[5 * st] = b.v.nn.z;
    q[6 * st] = b.v.sn.x; q[7 * st] = b.v.sn.y; q[8 * st] = b.v.sn.z;
    q[9 * st] = b.v.ng.x; q[10 * st] = b.v.ng.y; q[11 * st] = b.v.ng.z;
    q[12 * st] = b.v.wo.x; q[13 * st] = b.v.wo.y; q[14 * st] = b.v.wo.z;
    q[15 * st] = b.wnext.x; q[16 * st] = b.wnext.y; q[17 * st] = b.wnext.z;
    q[18 * st] = __int_as_float(b.v.mat); q[19 * st] = b.bsdfWeight; q[20 * st] = b.rrWeight;
}
RT_DEV void bd_load(const DevFrame &fr, int side, int k, unsigned gtid, BidirVertex &b) {
    const float RT_G *q = bd_vertex_ptr(fr, side, k, gtid); const size_t st = fr.n_threads;
    b.v.p = mk3(q[0 * st], q[1 * st], q[2 * st]);
    b.v.nn = mk3(q[3 * st], q[4 * st], q[5 * st]);
    b.v.sn = mk3(q[6 * st], q[7 * st], q[8 * st]);
    b.v.tn = cross3(b.v.nn, b.v.sn);                                          // as make_vertex / frame_pop rebuild the BSDF frame
    b.v.ng = mk3(q[9 * st], q[10 * st], q[11 * st]);
    b.v.wo = mk3(q[12 * st], q[13 * st], q[14 * st]);
    b.wnext = mk3(q[15 * st], q[16 * st], q[17 * st]);
    b.v.mat = __float_as_int(q[18 * st]); b.v.light = -1;
    b.bsdfWeight = q[19 * st]; b.rrWeight = q[20 * st];
}
// eye[k].bsdf->f(wi, wo) * AbsDot(wo, ng) / weight   (bidirectional.cpp:123-125 with weight = bsdfWeight, :183-185 and :192-194 with bsdfWeight * rrWeight)
RT_DEV V3 bd_step_factor(const DevScene &sc, const BidirVertex &b, float weight) {
    return div_s(bsdf_f<true>(RT_MAT(sc, b.v.mat), b.v, b.v.wo, b.wnext) * absdot3(b.wnext, b.v.ng), weight);
}

// every lane with a ray traces it to the end (the megakernel's shared traversal loop without its early exit: nothing else could run meanwhile)
template <bool COUNT, int ACCEL>
RT_DEV void bd_trace(const DevScene &sc, const DevFrame &fr, Lane &ln, uint2 RT_L *lds_stack, unsigned gtid, TravCounters &tc) {
    for (;;) {
        if (!__ballot(ln.has_ray && ln.tv.active)) break;
        trace_round<COUNT, ACCEL, true, RT_STACK_LDS, false>(ln.tv, ln.has_ray, sc, lds_stack, (float RT_L *)nullptr, RT_GPTR(uint2, fr.spill), fr.n_threads, gtid, tc, fr.leaf_min);
    }
    ln.has_ray = false;
}

// generatePath (bidirectional.cpp:132-173) for the lanes in `alive`; side 0: the eye path, 1: the light path.  Returns the lane's vertex count.
template <bool COUNT, int ACCEL>
RT_DEV int bd_generate_path(const DevScene &sc, const DevFrame &fr, const BidirTable RT_G *tab, Lane &ln, bool alive, Ray ray, int side,
                            uint2 RT_L *lds_stack, unsigned gtid, TravCounters &tc, unsigned &c_closest) {
    int nVerts = 0;
#pragma unroll 1
    for (int k = 0; k < RT_BD_MAX_VERTS; ++k) {
        if (!__any(alive)) break;
        if (alive) { accel_begin<ACCEL>(ln.tv, sc, ray, false); ln.has_ray = true; }        // RayDifferential(o, d): mint = RAY_EPSILON, maxt = infinity
        bd_trace<COUNT, ACCEL>(sc, fr, ln, lds_stack, gtid, tc);
        if (alive) {
            if (COUNT) ++c_closest;
            if (ln.tv.hit_prim < 0) alive = false;
            else {
                BidirVertex b;
                const int resolved = resolve_hit_material(sc, fr, ln.tv, side * RT_BD_MAX_VERTS + k, gtid);   // a textured material: one resolved record per path vertex (rt_texture.h)
                make_vertex<true>(sc, ln.tv, b.v);                              // v.p, v.ng = dg.nn, the BSDF's shading frame, v.wi = -ray.d
                if (resolved >= 0) b.v.mat = resolved;
                b.wnext = mk3(0.f); b.bsdfWeight = 0.f; b.rrWeight = 1.f;
                ++nVerts;
                if (nVerts > 2) {                                               // :151-156
                    const float rrProb = .2f;
                    if (ln.rng.next_float() > rrProb) alive = false;
                    else b.rrWeight = 1.f / rrProb;
                }
                if (alive) {                                                    // :158-165
                    const DimReq r2 = tab->two_d[4 * k + side], r1 = tab->one_d[4 * k + side];
                    const float u1 = dim_value(fr, ln, r2, 0, 0), u2 = dim_value(fr, ln, r2, 0, 1), u3 = dim_value(fr, ln, r1, 0, 0);
                    int flags;
                    const V3 f = bsdf_sample_f<true>(RT_MAT(sc, b.v.mat), b.v, b.v.wo, b.wnext, u1, u2, u3, b.bsdfWeight, BX_ALL, flags);
                    if (is_black(f) && b.bsdfWeight == 0.f) alive = false;
                    else { ray.o = b.v.p; ray.d = b.wnext; }
                }
                bd_store(fr, side, k, gtid, b);
            }
        }
    }
    return nVerts;
}

template <bool COUNT, int ACCEL>
__global__ __launch_bounds__(RT_BLOCK, 1) void bidir_kernel(const DevScene *__restrict__ scp, const DevFrame *__restrict__ frp) {
    __shared__ uint2 lds_stack_own[RT_STACK_LDS * RT_BLOCK];
    uint2 RT_L *lds_stack = (uint2 RT_L *)lds_stack_own;
    const DevScene &sc = *scp;
    const DevFrame &fr = *frp;
    const BidirTable RT_G *tab = RT_GPTR(const BidirTable, fr.light_dims);
    const unsigned gtid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int nLights = int(sc.n_lights);
    const V3 wc = mk3(tab->wc[0], tab->wc[1], tab->wc[2]); const float wr = tab->wr;
    Lane ln;
    ln.has_ray = false; ln.tv.active = false; ln.tv.hit_prim = -1; ln.fsp = 0; ln.depth = 0; ln.stage = ST_FETCH;
    TravCounters tc; tc.nodes = tc.leaf_refs = tc.tris = tc.spills = 0;
    RT_PFT(tc.c_desc = tc.c_leaf = tc.n_chunks = tc.n_pooled = tc.n_iter = 0;)
    unsigned c_cam = 0, c_closest = 0, c_any = 0, c_bad = 0;
#pragma unroll 1
    for (;;) {
        // ---- the wave's next 64 camera samples (one visit to the work counter per RT_MEGA_CHUNK, as in the megakernel; a batch needs all of them fresh)
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(fr.work_counter, (unsigned long long)RT_MEGA_CHUNK);
        base = uniform64(__shfl(base, 0));
        if (base >= fr.total_work) break;
#pragma unroll 1
        for (unsigned sub = 0; sub < RT_MEGA_CHUNK; sub += 64) {
            const unsigned long long w = base + sub + unsigned(lane);
            bool on = w < fr.total_work;
            Ray ray; ray.o = mk3(0.f); ray.d = mk3(0.f, 0.f, 1.f); ray.mint = RT_RAY_EPSILON; ray.maxt = RT_INF;
            if (on) {
                unsigned long long pixel = 0; int s = 0;
                if (fr.mega_tile > 0) { unsigned px; tile_order_to_sample(fr, unsigned(w), px, s); pixel = px; }
                else on = work_to_sample(fr, w, pixel, s);
                if (on) {
                    Ray cam;
                    setup_sample(sc, fr, ln, pixel, s, cam);
                    ln.work = fr.mega_tile > 0 ? uint32_t(pixel * unsigned(fr.spp) + unsigned(s)) : uint32_t(w);
                    ray.o = cam.o; ray.d = cam.d;                               // generatePath: RayDifferential ray(r.o, r.d), the camera's mint / maxt are dropped (:137)
                    if (COUNT) ++c_cam;
                }
            }
            // ---- eye path (:86-92)
            const int nEye = bd_generate_path<COUNT, ACCEL>(sc, fr, tab, ln, on, ray, 0, lds_stack, gtid, tc, c_closest);
            bool live = on && nEye > 0;                                         // nEye == 0: alpha 0, L = 0, nothing further is drawn
            const float alpha = live ? 1.f : 0.f;
            V3 L = mk3(0.f);
            // ---- the light and its emission ray (:93-110)
            float Le = 0.f;
            if (live) {
                const DimReq rn = tab->one_d[4 * RT_BD_MAX_VERTS], rp = tab->two_d[4 * RT_BD_MAX_VERTS], rdir = tab->two_d[4 * RT_BD_MAX_VERTS + 1];
                const int lightNum = min(int(floorf(dim_value(fr, ln, rn, 0, 0) * nLights)), nLights - 1);
                const float u0 = dim_value(fr, ln, rp, 0, 0), u1 = dim_value(fr, ln, rp, 0, 1), u2 = dim_value(fr, ln, rdir, 0, 0), u3 = dim_value(fr, ln, rdir, 0, 1);
                float lightPdf;
                light_sample_emission<true>(sc, RT_LIGHT(sc, lightNum), wc, wr, u0, u1, u2, u3, ln.rng, ray.o, ray.d, lightPdf);
                if (lightPdf == 0.f) live = false;                              // return 0.f (alpha stays 1)
                else Le = float(nLights) / lightPdf;                            // Le = lightWeight / lightPdf: the light's spectrum is overwritten
            }
            // ---- light path (:111-112)
            const int nLight = bd_generate_path<COUNT, ACCEL>(sc, fr, tab, ln, live, ray, 1, lds_stack, gtid, tc, c_closest);
            // light[k]'s factor of evalPath's last loop (:191-194), k = 0 .. 2; used only where vertex k + 1 exists
            V3 lf0 = mk3(0.f), lf1 = mk3(0.f), lf2 = mk3(0.f);
#pragma unroll 1
            for (int k = 0; k < RT_BD_MAX_VERTS - 1; ++k) {
                if (!__any(live && k < nLight - 1)) break;
                if (live && k < nLight - 1) {
                    BidirVertex b; bd_load(fr, 1, k, gtid, b);
                    const V3 f = bd_step_factor(sc, b, b.bsdfWeight * b.rrWeight);
                    if (k == 0) lf0 = f; else if (k == 1) lf1 = f; else lf2 = f;
                }
            }
            // ---- connections (:113-130)
            V3 directWt = mk3(1.f), eyePre = mk3(1.f);                         // eyePre: evalPath's product over eye[0 .. i-2] (:181-185), carried across i
#pragma unroll 1
            for (int i = 1; i <= RT_BD_MAX_VERTS; ++i) {
                const bool act = live && i <= nEye;
                if (!__any(act)) break;
                BidirVertex e;
                if (act) {
                    bd_load(fr, 0, i - 1, gtid, e);
                    ln.v = e.v;
                    directWt = div_s(directWt, e.rrWeight);
                    // UniformSampleOneLight(p, ng, wi, bsdf, sample, directLight, directLightNum, directBSDF, directBSDFComp) transport.cpp:51-70
                    const DimReq rl = tab->two_d[4 * (i - 1) + 2], rb = tab->two_d[4 * (i - 1) + 3], rn = tab->one_d[4 * (i - 1) + 2], rc = tab->one_d[4 * (i - 1) + 3];
                    const int lightNum = min(int(floorf(dim_value(fr, ln, rn, 0, 0) * nLights)), nLights - 1);
                    const float ls1 = dim_value(fr, ln, rl, 0, 0), ls2 = dim_value(fr, ln, rl, 0, 1);
                    ln.bs1 = dim_value(fr, ln, rb, 0, 0); ln.bs2 = dim_value(fr, ln, rb, 0, 1); ln.bcs = dim_value(fr, ln, rc, 0, 0);
                    estimate_direct_begin<true, false, true>(sc, ln, lightNum, ls1, ls2);          // -> shadow ray (ST_SHADOW_DONE) or ST_ED_BSDF
                }
                bd_trace<COUNT, ACCEL>(sc, fr, ln, lds_stack, gtid, tc);
                if (act && ln.stage == ST_SHADOW_DONE) stage_body<COUNT, RT_INTEGRATOR_PATH, false, true, ST_SHADOW_DONE>(sc, fr, ln, gtid, &c_closest, &c_any, &c_bad);
                if (act && ln.stage == ST_ED_BSDF) estimate_direct_bsdf<true, false, true>(sc, ln);     // -> MIS ray (ST_MIS_DONE) or ST_ED_DONE
                bd_trace<COUNT, ACCEL>(sc, fr, ln, lds_stack, gtid, tc);
                if (act && ln.stage == ST_MIS_DONE) stage_body<COUNT, RT_INTEGRATOR_PATH, false, true, ST_MIS_DONE>(sc, fr, ln, gtid, &c_closest, &c_any, &c_bad);
                if (act) {
                    L = L + div_s(directWt * (ln.Ld * float(nLights)), float(i));                    // / weightPath(eye, i, light, 0)
                    if (i < nEye) directWt = directWt * bd_step_factor(sc, e, e.bsdfWeight);          // (the last vertex's wo is never read: skipped)
                }
#pragma unroll 1
                for (int j = 1; j <= RT_BD_MAX_VERTS; ++j) {
                    const bool cj = act && j <= nLight;
                    if (!__any(cj)) break;
                    if (cj) {                                                   // evalPath(eye, i, light, j) :179-200
                        BidirVertex l; bd_load(fr, 1, j - 1, gtid, l);
                        const V3 w = l.v.p - e.v.p;
                        const V3 wn = normalize3(l.v.p - e.v.p);                // G(eye[i-1], light[j-1]) :201-205
                        const float G = absdot3(e.v.ng, wn) * absdot3(l.v.ng, -wn) / dist_sq(e.v.p, l.v.p);
                        const V3 fe = bsdf_f<true>(RT_MAT(sc, e.v.mat), e.v, e.v.wo, w), fl = bsdf_f<true>(RT_MAT(sc, l.v.mat), l.v, -w, l.v.wo);
                        V3 Lp = eyePre * div_s((fe * G) * fl, e.rrWeight * l.rrWeight);
                        if (j >= 4) Lp = Lp * lf2;
                        if (j >= 3) Lp = Lp * lf1;
                        if (j >= 2) Lp = Lp * lf0;
                        if (!is_black(Lp)) {                                    // visible(): Ray(P0, P1 - P0, RAY_EPSILON, 1 - RAY_EPSILON), IntersectP :206-210
                            ln.pend = Lp;
                            launch_ray(ln, sc, e.v.p, w, RT_RAY_EPSILON, 1.f - RT_RAY_EPSILON, true, ST_SHADOW_DONE);
                        }
                    }
                    const bool cast = cj && ln.has_ray;
                    bd_trace<COUNT, ACCEL>(sc, fr, ln, lds_stack, gtid, tc);
                    if (cast) {
                        if (COUNT) ++c_any;
                        if (ln.tv.hit_prim < 0) L = L + div_s(mk3(Le) * ln.pend, float(i + j));     // L += Le * evalPath / weightPath
                    }
                }
                if (act && i < nEye) eyePre = eyePre * bd_step_factor(sc, e, e.bsdfWeight * e.rrWeight);
            }
            if (on) sample_write(fr, ln, L, alpha, c_bad);
        }
    }
    if (COUNT) {
        unsigned long long v[8] = {c_cam, c_closest, c_any, tc.nodes, tc.leaf_refs, tc.tris, c_bad, tc.spills};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            unsigned long long x = v[k];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
            if (lane == 0 && x) atomicAdd(fr.counters + k, x);
        }
    }
}

}  // namespace rt
