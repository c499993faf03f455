// rt_rays.hip -- caller-supplied rays in DEVICE memory: rt_trace_closest_device / rt_trace_any_device / rt_hit_geometry_device (include/pbrt_hip.h).
// Scene::Intersect / IntersectP and the Intersection's DifferentialGeometry for rays that are already on the GPU (a torch tensor of origins and
// directions: a G-buffer, a custom camera, a collision query), on the scene's stream, without a host round trip.
//
// Kernels
//   rays_layout_kernel   RtRay[n] -> the two float4 planes {o, mint} {d, maxt} rt::pipe_trace_kernel reads (rt_pipeline.h TraceJob), with the guard of
//                        rt_ray_guard.h applied, and the queue counters of the launch (the host path, rt_kernels.hip trace_common, uploads both from the host).
//   (rt_pipeline.h)      pipe_trace_kernel itself, the entry flavour::Trace names: the caller's RtHit array is its hit plane.
//   occlusion_kernel     the hit plane of an any-hit launch -> one byte per ray.
//   hit_geometry_kernel  one lane per ray: the traversal's hit state rebuilt from (ray, RtHit) (rt_hit_state.h), then make_vertex<true> / hit_point_uv -- the code the render
//                        kernels and the debug integrator run (rt_shade.h, rt_texture.h) -- for the fields the caller asked for.
#include "rt_hit_state.h"
#include "rt_ray_guard.h"

namespace rt {

__global__ __launch_bounds__(RT_RAYS_BLOCK) void rays_layout_kernel(const float4 *__restrict__ rays, unsigned n, float4 *__restrict__ q_o, float4 *__restrict__ q_d,
                                                                    unsigned *__restrict__ qc, int any) {
    const unsigned i = blockIdx.x * RT_RAYS_BLOCK + threadIdx.x;
    if (i == 0) {                                                        // this launch's queue: n rays of one kind, the consumer head at its start
        RT_GPTR(unsigned, qc)[0] = any ? 0u : n; RT_GPTR(unsigned, qc)[RT_QC_HEAD] = 0u; RT_GPTR(unsigned, qc)[RT_QC_ANY] = any ? n : 0u;
    }
    if (i >= n) return;
    const float4 a = RT_GPTR(const float4, rays)[size_t(2) * i], b = RT_GPTR(const float4, rays)[size_t(2) * i + 1];      // o.xyz d.x | d.yz mint maxt
    float4 ro = make_float4(a.x, a.y, a.z, b.z), rd = make_float4(a.w, b.x, b.y, b.w);
    if (!ray_usable(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w)) {
        ro = make_float4(RT_EMPTY_RAY_O, RT_EMPTY_RAY_MINT); rd = make_float4(RT_EMPTY_RAY_D, RT_EMPTY_RAY_MAXT);
    }
    RT_GPTR(float4, q_o)[i] = ro; RT_GPTR(float4, q_d)[i] = rd;
}

__global__ __launch_bounds__(RT_RAYS_BLOCK) void occlusion_kernel(const float4 *__restrict__ hits, unsigned n, uint8_t *__restrict__ occ) {
    const unsigned i = blockIdx.x * RT_RAYS_BLOCK + threadIdx.x;
    if (i >= n) return;
    RT_GPTR(uint8_t, occ)[i] = __float_as_int(RT_GPTR(const float4, hits)[i].x) >= 0 ? 1 : 0;
}

// Which fields are wanted is a property of the launch (the pointers are kernel arguments): every branch on it is wave-uniform.
__global__ __launch_bounds__(RT_RAYS_BLOCK) void hit_geometry_kernel(const DevScene *__restrict__ scp, const float4 *__restrict__ rays, const float4 *__restrict__ hits,
                                                                     unsigned n, RtHitGeometry out) {
    const DevScene &sc = *scp;
    const unsigned i = blockIdx.x * RT_RAYS_BLOCK + threadIdx.x;
    if (i >= n) return;
    RT_HIT_STATE(tv, hit, sc, rays, hits, i);                           // (rt_hit_state.h: a record that names no primitive of this scene counts as a miss)
    V3 p = mk3(0.f), ng = mk3(0.f), ns = mk3(0.f);
    float u = 0.f, v = 0.f;
    int mat = -1, light = -1;
    if (hit) {
        const float4 RT_G *q = RT_GPTR(const float4, sc.tri_shade) + size_t(2) * unsigned(tv.hit_prim);
        const unsigned bits = __float_as_uint(q[0].w);
        mat = int(bits & 0xffffu); light = __float_as_int(q[1].w);
        if (out.p || out.ng || out.ns) {
            Vertex vx;
            make_vertex<true>(sc, tv, vx);                              // dg.p, dg.nn (vx.ng) and bsdf->dgShading.nn (vx.nn)
            p = vx.p; ng = vx.ng; ns = vx.nn;
        }
        if (out.uv) { RtTexHit th; hit_point_uv(sc, tv, bits, th); u = th.u; v = th.v; }
    }
    const size_t i3 = size_t(3) * i;
    if (out.p) { float RT_G *w = RT_GPTR(float, out.p) + i3; w[0] = p.x; w[1] = p.y; w[2] = p.z; }
    if (out.ng) { float RT_G *w = RT_GPTR(float, out.ng) + i3; w[0] = ng.x; w[1] = ng.y; w[2] = ng.z; }
    if (out.ns) { float RT_G *w = RT_GPTR(float, out.ns) + i3; w[0] = ns.x; w[1] = ns.y; w[2] = ns.z; }
    if (out.uv) { float RT_G *w = RT_GPTR(float, out.uv) + size_t(2) * i; w[0] = u; w[1] = v; }
    if (out.material) RT_GPTR(int, out.material)[i] = mat;
    if (out.light) RT_GPTR(int, out.light)[i] = light;
}

}  // namespace rt

// ------------------------------------------------------------------------------------------ host side
// Lay the rays out, write the queue counters, run the trace kernel over them.  `hit_plane`: the caller's RtHit array or s->any_hits.
static int trace_device(RtScene *s, const RtRay *dev_rays, uint32_t n, int any, float4 *hit_plane) {
    if (int rc = ensure(s, s->ray_planes, size_t(n) * 2)) return rc;
    float4 *q_o = s->ray_planes, *q_d = q_o + n;
    hipLaunchKernelGGL(rays_layout_kernel, dim3(blocks_for(n)), dim3(RT_RAYS_BLOCK), 0, s->stream, reinterpret_cast<const float4 *>(dev_rays), n, q_o, q_d,
                       (unsigned *)s->trace_qc, any);
    TraceJob job{};
    job.q_o = q_o; job.q_d = q_d; job.q_slot = nullptr; job.q_count = s->trace_qc; job.hit = hit_plane;
    job.n_slots = 0; job.spill = s->spill; job.n_threads = s->n_threads; job.counters = s->counters;
    // rt_set_counting is honoured: the counting twin or the timed kernel (the hits are the same, rt_flavour.h)
    const int k = flavour::Trace::index(plan::request(nullptr, s->facts, nullptr));
    hipLaunchKernelGGL(g_pipe_trace[k], dim3(s->grids.trace[k]), dim3(RT_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, job);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

extern "C" {

int rt_trace_closest_device(RtScene *s, const RtRay *dev_rays, uint32_t n, RtHit *dev_hits) {
    static const std::string fn = "rt_trace_closest_device";
    if (int rc = check_rays(fn, s, dev_rays, n)) return rc;
    if (int rc = check_hits(fn, dev_hits)) return rc;
    if (n == 0) return RT_OK;
    HIPCHK(hipSetDevice(s->device));
    return trace_device(s, dev_rays, n, 0, reinterpret_cast<float4 *>(dev_hits));
}

int rt_trace_any_device(RtScene *s, const RtRay *dev_rays, uint32_t n, uint8_t *dev_occluded) {
    static const std::string fn = "rt_trace_any_device";
    if (int rc = check_rays(fn, s, dev_rays, n)) return rc;
    if (int rc = refuse_null(fn, dev_occluded, "output pointer")) return rc;
    if (n == 0) return RT_OK;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = ensure(s, s->any_hits, size_t(n))) return rc;
    if (int rc = trace_device(s, dev_rays, n, 1, s->any_hits)) return rc;
    hipLaunchKernelGGL(occlusion_kernel, dim3(blocks_for(n)), dim3(RT_RAYS_BLOCK), 0, s->stream, (const float4 *)s->any_hits, n, dev_occluded);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

int rt_hit_geometry_device(RtScene *s, const RtRay *dev_rays, const RtHit *dev_hits, uint32_t n, const RtHitGeometry *out) {
    static const std::string fn = "rt_hit_geometry_device";
    if (int rc = check_rays(fn, s, dev_rays, n)) return rc;
    if (int rc = check_hits(fn, dev_hits)) return rc;
    if (int rc = refuse_null(fn, out, "RtHitGeometry")) return rc;
    if (!out->p && !out->ng && !out->ns && !out->uv && !out->material && !out->light)
        return fail(RT_EINVAL, fn + ": every field of the RtHitGeometry is null (nothing is wanted)");
    if (n == 0) return RT_OK;
    HIPCHK(hipSetDevice(s->device));
    // dg.u / dg.v of a mesh with "uv" read the mesh's uvs: on the device from the first call that wants them (once per scene; rt_scene.hip)
    if (out->uv) { if (int rc = upload_tex_uv(s)) return rc; }
    hipLaunchKernelGGL(hit_geometry_kernel, dim3(blocks_for(n)), dim3(RT_RAYS_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene,
                       reinterpret_cast<const float4 *>(dev_rays), reinterpret_cast<const float4 *>(dev_hits), n, *out);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

}  // extern "C"
