// rt_bsdf.hip -- rt_bsdf_device (include/pbrt_hip.h): what an integrator asks of a hit -- Intersection::GetBSDF followed by BSDF::f, BSDF::Pdf,
// BSDF::Sample_f and BSDF::NumComponents, and Intersection::Le -- at caller-supplied (ray, RtHit) pairs in DEVICE memory, on the scene's stream,
// without a host round trip.  It traces nothing and it is no frame.
//
// Kernel
//   bsdf_query_kernel    one lane per query: the traversal's hit state rebuilt from (ray, RtHit) (rt_hit_state.h, shared with hit_geometry_kernel),
//                        the material resolved at the hit where it has textured parameters (resolve_hit_material, rt_texture.h), the shading frame
//                        of make_vertex<true>, then rt_shade.h's own functions -- the code the frames run -- for the outputs the caller asked for.
//                        The grid is hit_geometry_kernel's, capped at the scene's resident threads: a lane beyond the cap takes its next query a
//                        grid further, so the resolved-material record a lane owns (one per lane, the frames' pool) is sized by the cap, not by n.
#include "rt_hit_state.h"

namespace rt {

// Which outputs are wanted is a property of the launch (the pointers are kernel arguments): every branch on it is wave-uniform.
__global__ __launch_bounds__(RT_RAYS_BLOCK) void bsdf_query_kernel(const DevScene *__restrict__ scp, const DevFrame *__restrict__ frp, const float4 *__restrict__ rays,
                                                                   const float4 *__restrict__ hits, unsigned n, RtBsdfQuery q) {
    const DevScene &sc = *scp;
    const unsigned slot = blockIdx.x * RT_RAYS_BLOCK + threadIdx.x, stride = gridDim.x * RT_RAYS_BLOCK;    // (n <= 2^30 and stride <= 2^30: i + stride fits)
    const bool want_sample = q.s_wi || q.s_f || q.s_pdf || q.s_type;
    for (unsigned i = slot; i < n; i += stride) {
        RT_HIT_STATE(tv, hit, sc, rays, hits, i);
        const int flags = q.flags ? RT_GPTR(const int, q.flags)[i] : int(BX_ALL);
        V3 f = mk3(0.f), s_wi = mk3(0.f), s_f = mk3(0.f), le = mk3(0.f);
        float pdf = 0.f, s_pdf = 0.f;
        int s_type = 0, nc = 0;
        if (hit) {
            Vertex v;
            const int resolved = resolve_hit_material(sc, *frp, tv, 0, slot);     // a textured material: resolved at this hit into this lane's record
            make_vertex<true>(sc, tv, v);                                         // the BSDF's frame, dg.nn (v.ng) and wo = -d
            if (resolved >= 0) v.mat = resolved;
            MatRef m = RT_MAT(sc, v.mat);
            if (q.n_components) nc = bsdf_num_components<true>(m, flags);
            if (q.f || q.pdf) {
                const float RT_G *w = RT_GPTR(const float, q.wi) + size_t(3) * i;
                const V3 wi = mk3(w[0], w[1], w[2]);
                if (q.f) f = bsdf_f_flags<true>(m, v, v.wo, wi, flags);
                if (q.pdf) pdf = bsdf_pdf_flags<true>(m, v, v.wo, wi, flags);
            }
            if (want_sample) {
                const float RT_G *u = RT_GPTR(const float, q.u) + size_t(3) * i;
                V3 wi = mk3(0.f);
                const V3 sf = bsdf_sample_f<true>(m, v, v.wo, wi, u[0], u[1], u[2], s_pdf, flags, s_type);
                if (s_pdf == 0.f) s_type = 0;                                      // reflection.cpp:428-431: no sample
                else { s_wi = wi; s_f = sf; }
            }
            if (q.le && v.light >= 0) le = area_L(RT_LIGHT(sc, v.light), v.ng, v.wo);   // Intersection::Le primitive.cpp:142-145: area->L(dg.p, dg.nn, wo), the geometric normal
        }
        const size_t i3 = size_t(3) * i;
        if (q.f) { float RT_G *w = RT_GPTR(float, q.f) + i3; w[0] = f.x; w[1] = f.y; w[2] = f.z; }
        if (q.pdf) RT_GPTR(float, q.pdf)[i] = pdf;
        if (q.s_wi) { float RT_G *w = RT_GPTR(float, q.s_wi) + i3; w[0] = s_wi.x; w[1] = s_wi.y; w[2] = s_wi.z; }
        if (q.s_f) { float RT_G *w = RT_GPTR(float, q.s_f) + i3; w[0] = s_f.x; w[1] = s_f.y; w[2] = s_f.z; }
        if (q.s_pdf) RT_GPTR(float, q.s_pdf)[i] = s_pdf;
        if (q.s_type) RT_GPTR(int, q.s_type)[i] = s_type;
        if (q.n_components) RT_GPTR(int, q.n_components)[i] = nc;
        if (q.le) { float RT_G *w = RT_GPTR(float, q.le) + i3; w[0] = le.x; w[1] = le.y; w[2] = le.z; }
    }
}

}  // namespace rt

// ------------------------------------------------------------------------------------------ host side
extern "C" {

int rt_bsdf_device(RtScene *s, const RtRay *dev_rays, const RtHit *dev_hits, uint32_t n, const RtBsdfQuery *q) {
    static const std::string fn = "rt_bsdf_device";
    if (int rc = refuse_null(fn, s, "scene")) return rc;
    if (n > RT_RAYS_MAX_N) return fail(RT_EINVAL, fn + ": n = " + std::to_string(n) + " is above 2^30");
    if (n == 0) return RT_OK;
    if (int rc = check_rays(fn, s, dev_rays, n)) return rc;
    if (int rc = check_hits(fn, dev_hits)) return rc;
    if (int rc = refuse_null(fn, q, "RtBsdfQuery")) return rc;
    const bool want_sample = q->s_wi || q->s_f || q->s_pdf || q->s_type;
    if (!q->f && !q->pdf && !want_sample && !q->n_components && !q->le)
        return fail(RT_EINVAL, fn + ": every output of the RtBsdfQuery is null (nothing is wanted)");
    if ((q->f || q->pdf) && !q->wi) return fail(RT_EINVAL, fn + ": f or pdf is wanted and wi is null");
    if (want_sample && !q->u) return fail(RT_EINVAL, fn + ": s_wi, s_f, s_pdf or s_type is wanted and u is null");
    HIPCHK(hipSetDevice(s->device));
    // A scene with textured materials resolves them per hit into one record per lane: the frames' pool behind the scene's own materials, level 0, one
    // record per resident thread -- sized by the scene, not by n, and grown (once: the stream is waited for) only when no frame or query has made it
    // yet.  Work on one stream runs in order, so a frame and a query never hold records at the same time.
    DevFrame fr{};
    const unsigned lanes = std::max(s->n_threads, unsigned(RT_RAYS_BLOCK));
    if (int rc = ensure_material_pool(s, fr, 1, lanes)) return rc;
    fr.n_threads = lanes;
    if (!s->bsdf_frame.p || s->bsdf_pool_base != fr.mat_pool_base) {      // the descriptor resolve_hit_material reads: the pool's place, uploaded when it changes
        HIPCHK(hipStreamSynchronize(s->stream));
        if (int rc = s->bsdf_frame.grow(1)) return rc;
        HIPCHK(hipMemcpy(s->bsdf_frame, &fr, sizeof(DevFrame), hipMemcpyHostToDevice));
        s->bsdf_pool_base = fr.mat_pool_base;
    }
    if (int rc = pending_error()) return rc;
    const unsigned grid = std::min(blocks_for(n), lanes / RT_RAYS_BLOCK);
    hipLaunchKernelGGL(bsdf_query_kernel, dim3(grid), dim3(RT_RAYS_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, (const DevFrame *)s->bsdf_frame,
                       reinterpret_cast<const float4 *>(dev_rays), reinterpret_cast<const float4 *>(dev_hits), n, *q);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

}  // extern "C"
