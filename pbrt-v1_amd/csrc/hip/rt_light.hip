// rt_light.hip -- rt_light_device (include/pbrt_hip.h): what EstimateDirect asks of a light -- Light::Sample_L with and without a normal, Light::Pdf,
// Light::Le and Light::IsDeltaLight -- at caller-supplied points in DEVICE memory, on the scene's stream, without a host round trip.  It traces
// nothing and it is no frame: the shadow ray it returns goes to rt_trace_any_device.
//
// Kernel
//   light_query_kernel   one lane per query: the light's record by index, then rt_shade.h's own functions -- the code the frames run, in their generic
//                        forms (no scene twin, no small-emitter form) -- for the outputs the caller asked for.  The light's type is a per-lane value: a
//                        wave whose queries name lights of several types runs each type's code in turn, so callers do best to group queries by light.
//                        No workspace: the grid is capped at the scene's resident threads and a lane beyond the cap takes its next query a grid further.
#include "rt_hit_state.h"

namespace rt {

// Which outputs are wanted is a property of the launch (the pointers are kernel arguments): every branch on it is wave-uniform.
__global__ __launch_bounds__(RT_RAYS_BLOCK) void light_query_kernel(const DevScene *__restrict__ scp, unsigned n, RtLightQuery q) {
    const DevScene &sc = *scp;
    const unsigned slot = blockIdx.x * RT_RAYS_BLOCK + threadIdx.x, stride = gridDim.x * RT_RAYS_BLOCK;    // (n <= 2^30 and stride <= 2^30: i + stride fits)
    const bool want_sample = q.s_wi || q.s_L || q.s_pdf || q.s_ray || q.s_draws;
    for (unsigned i = slot; i < n; i += stride) {
        const size_t i3 = size_t(3) * i;
        const float RT_G *pp = RT_GPTR(const float, q.p) + i3;
        const V3 p = mk3(pp[0], pp[1], pp[2]);
        const int li = RT_GPTR(const int, q.light)[i];
        V3 nrm = mk3(0.f);
        if (q.nrm) { const float RT_G *w = RT_GPTR(const float, q.nrm) + i3; nrm = mk3(w[0], w[1], w[2]); }
        V3 s_wi = mk3(0.f), s_L = mk3(0.f), sd = mk3(0.f), so = mk3(0.f), le = mk3(0.f);
        float s_pdf = 0.f, smin = 0.f, smax = 0.f, pdf = 0.f;
        int draws = 0, delta = 0;
        if (unsigned(li) < sc.n_lights) {
            LightRef Lt = RT_LIGHT(sc, li);
            delta = light_is_delta<true>(Lt) ? 1 : 0;
            if (want_sample) {
                const float RT_G *u = RT_GPTR(const float, q.u) + size_t(2) * i;
                const float u1 = u[0], u2 = u[1];
                Rng rng;                                                            // the keyed stream of camera sample `key` (rt_integrate.h), at the caller's counter
                uint32_t key = i, ctr = 0u;
                if (q.rng) { const uint32_t RT_G *r = RT_GPTR(const uint32_t, q.rng) + size_t(2) * i; key = r[0]; ctr = r[1]; }
                rng.base = rng_base(key, q.seed); rng.ctr = ctr;
                if (delta) {                                                        // light.h:58-62 -> point.cpp:61-66, spot.cpp:79-83, distant.cpp:66-70: pdf = 1
                    s_L = delta_light_sample(Lt, p, s_wi, sd, smax);
                    s_pdf = 1.f;
                } else if (light_is_infinite<true>(Lt)) {                           // infinite.cpp:96-116 with a normal, :121-128 without; SetRay(p, wi)
                    s_wi = q.nrm ? infinite_sample_cosine(nrm, u1, u2, rng, s_pdf) : infinite_sample_sphere(u1, u2, s_pdf);
                    s_L = mat_color(Lt.color);
                    sd = s_wi; smax = RT_INF;
                } else {                                                            // area.cpp:58-68 and :73-82: one body, the normal is not read
                    V3 ns;
                    const V3 ps = area_sample_point<true>(sc, Lt, p, u1, u2, rng, ns);
                    s_wi = normalize3(ps - p);
                    s_pdf = area_light_pdf<true>(sc, Lt, p, s_wi);
                    s_L = area_L(Lt, ns, -s_wi);
                    sd = ps - p; smax = 1.f - RT_RAY_EPSILON;                       // SetSegment(p, ps) light.h:78-80
                }
                so = p; smin = RT_RAY_EPSILON;
                draws = int(rng.ctr - ctr);
            }
            if (q.pdf || q.le) {
                const float RT_G *w = RT_GPTR(const float, q.wi) + i3;
                const V3 wi = mk3(w[0], w[1], w[2]);
                if (q.pdf && !delta) {                                              // point.cpp:67-69, spot.cpp:84-86, distant.cpp:71-73 Pdf: 0
                    if (light_is_infinite<true>(Lt)) pdf = q.nrm ? infinite_pdf_cosine(nrm, wi) : infinite_pdf_sphere();    // infinite.cpp:117-120, :129-131
                    else pdf = area_light_pdf<true>(sc, Lt, p, wi);                 // area.cpp:69-72, :93-95
                }
                if (q.le && light_is_infinite<true>(Lt)) le = mat_color(Lt.color);  // infinite.cpp:83-95 (no map); every other light: Light::Le light.cpp, black
            }
        }
        if (q.s_wi) { float RT_G *w = RT_GPTR(float, q.s_wi) + i3; w[0] = s_wi.x; w[1] = s_wi.y; w[2] = s_wi.z; }
        if (q.s_L) { float RT_G *w = RT_GPTR(float, q.s_L) + i3; w[0] = s_L.x; w[1] = s_L.y; w[2] = s_L.z; }
        if (q.s_pdf) RT_GPTR(float, q.s_pdf)[i] = s_pdf;
        if (q.s_ray) {                                                              // RtRay: o.xyz d.x | d.yz mint maxt -- two 16-byte stores
            float4 RT_G *w = RT_GPTR(float4, q.s_ray) + size_t(2) * i;
            w[0] = make_float4(so.x, so.y, so.z, sd.x); w[1] = make_float4(sd.y, sd.z, smin, smax);
        }
        if (q.s_draws) RT_GPTR(int, q.s_draws)[i] = draws;
        if (q.pdf) RT_GPTR(float, q.pdf)[i] = pdf;
        if (q.le) { float RT_G *w = RT_GPTR(float, q.le) + i3; w[0] = le.x; w[1] = le.y; w[2] = le.z; }
        if (q.is_delta) RT_GPTR(int, q.is_delta)[i] = delta;
    }
}

}  // namespace rt

// ------------------------------------------------------------------------------------------ host side
extern "C" {

int rt_light_device(RtScene *s, uint32_t n, const RtLightQuery *q) {
    static const std::string fn = "rt_light_device";
    if (int rc = refuse_null(fn, s, "scene")) return rc;
    if (n > RT_RAYS_MAX_N) return fail(RT_EINVAL, fn + ": n = " + std::to_string(n) + " is above 2^30");
    if (n == 0) return RT_OK;
    if (int rc = refuse_null(fn, q, "RtLightQuery")) return rc;
    if (int rc = refuse_null(fn, q->p, "p")) return rc;
    if (int rc = refuse_null(fn, q->light, "light")) return rc;
    const bool want_sample = q->s_wi || q->s_L || q->s_pdf || q->s_ray || q->s_draws;
    if (!want_sample && !q->pdf && !q->le && !q->is_delta)
        return fail(RT_EINVAL, fn + ": every output of the RtLightQuery is null (nothing is wanted)");
    if (want_sample && !q->u) return fail(RT_EINVAL, fn + ": s_wi, s_L, s_pdf, s_ray or s_draws is wanted and u is null");
    if ((q->pdf || q->le) && !q->wi) return fail(RT_EINVAL, fn + ": pdf or le is wanted and wi is null");
    if (q->s_ray) { if (int rc = refuse_unaligned16(fn, q->s_ray, "s_ray")) return rc; }
    HIPCHK(hipSetDevice(s->device));
    if (int rc = pending_error()) return rc;
    const unsigned lanes = std::max(s->n_threads, unsigned(RT_RAYS_BLOCK));
    const unsigned grid = std::min(blocks_for(n), lanes / RT_RAYS_BLOCK);
    hipLaunchKernelGGL(light_query_kernel, dim3(grid), dim3(RT_RAYS_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, n, *q);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

}  // extern "C"
