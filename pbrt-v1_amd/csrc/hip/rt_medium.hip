// rt_medium.hip -- rt_medium_device and rt_volume_samples_device (include/pbrt_hip.h): what an integrator asks of scene->volumeRegion and of the
// volume integrator -- sigma_a / sigma_s / sigma_t / Lve / p at points, IntersectP / Tau / Transmittance / EmissionIntegrator::Li along rays -- at
// caller-supplied points and rays in DEVICE memory, on the scene's stream, without a host round trip; and the two sampler values and the stream
// position a frame's volume integrator starts from.  Neither is a frame.
//
// Kernels
//   medium_query_kernel    one lane per query.  The region is asked through the frames' own functions (rt_integrate.h: vol_intersect, vol_inside,
//                          vol_transmittance, density_at, density_tau_capped, exp_neg); the emission march (emission.cpp:60-95) is written out here in a
//                          straight line with the operations of march_begin / march_steps in their order.  Every loop carries a cap the host
//                          computed (rt_march_guard.h), and a march that could not advance is not started.  No workspace: the grid is capped at the
//                          scene's resident threads and a lane beyond the cap takes its next query a grid further.
//   volume_samples_kernel  setup_sample (rt_integrate.h) for camera sample first + i, then the frame's tau and scatter requests through dim_value.
#include "rt_hit_state.h"
#include "rt_march_guard.h"

namespace rt {

// PhaseHG(w, wp, g), volume.cpp:44-48 -- the expression of march_steps
RT_DEV float phase_hg(V3 w, V3 wp, float g) {
    const float costheta = dot3(w, wp);
    return 1.f / (4.f * RT_PI) * (1.f - g * g) / rt_powf(1.f + g * g - 2.f * g * costheta, 1.5f);
}

// EmissionIntegrator::Li (emission.cpp:60-95) with a sample, over the clipped interval [t0, t1] in N steps: the scatter offset, then per step one
// RandomFloat() for the step's Tau (at .5f * stepSize), the roulette draw when Tr.y() < 1e-3, and Lv += Tr * Lve(p).  N is bounded by the caller.
RT_DEV V3 emission_march(const DevScene &sc, bool dens, V3 o, V3 d, float t0, float t1, int N, float step_size, float u_scatter, Rng &rng, int tau_cap) {
    const RtVolume &vol = sc.vol;
    const float step = (t1 - t0) / N;
    V3 Tr = mk3(1.f), p = o + d * t0, Lv = mk3(0.f);
    t0 += u_scatter * step;
#pragma unroll 1
    for (int i = 0; i < N; ++i, t0 += step) {
        const V3 pPrev = p; p = o + d * t0;
        const float u = rng.next_float();                                       // Tau's offset argument
        const V3 stepT = dens ? exp_neg(density_tau_capped(sc, [tau_cap] { return tau_cap; }, pPrev, p - pPrev, 0.f, 1.f, .5f * step_size, u))
                              : vol_transmittance(vol, pPrev, p - pPrev, 0.f, 1.f);
        Tr = Tr * stepT;
        if (lum_y(Tr) < 1e-3) {
            if (rng.next_float() > .5f) break;
            Tr = div_s(Tr, .5f);
        }
        const float D = dens ? density_at(sc, xform_point(vol.world_to_volume, p)) : 0.f;
        const bool in = dens || vol_inside(vol, p);
        Lv = Lv + Tr * (dens ? D * mat_color(vol.le) : (in ? mat_color(vol.le) : mk3(0.f)));
    }
    return Lv * step;
}

RT_DEV void store3(void *base, size_t i3, V3 v) { float RT_G *w = RT_GPTR(float, base) + i3; w[0] = v.x; w[1] = v.y; w[2] = v.z; }

// Which outputs are wanted is a property of the launch (the pointers are kernel arguments), and so is the medium's kind: every branch on them is wave-uniform.
__global__ __launch_bounds__(RT_RAYS_BLOCK) void medium_query_kernel(const DevScene *__restrict__ scp, unsigned n, RtMediumQuery q, int step_cap, int tau_cap) {
    const DevScene &sc = *scp;
    const RtVolume &vol = sc.vol;
    const unsigned slot = blockIdx.x * RT_RAYS_BLOCK + threadIdx.x, stride = gridDim.x * RT_RAYS_BLOCK;    // (n <= 2^30 and stride <= 2^30: i + stride fits)
    const bool present = vol.present != 0, dens = sc.dens_kind != RT_DENSITY_NONE;
    const bool want_point = q.sigma_a || q.sigma_s || q.sigma_t || q.lve || q.phase;
    const bool want_ray = q.hit || q.t01 || q.tau || q.tr || q.lv || q.draws || q.status;
    const bool want_march = q.tau || q.tr || q.lv;
    const bool tr_draws = q.tr && !q.u;                                         // Scene::Transmittance(ray): sample == NULL, one RandomFloat()
    // the smallest step a Tau march of this query is called with: .5f * stepSize per emission step, stepSize with a sample, 4.f * stepSize without
    const float min_step = q.lv ? .5f * q.step_size : ((q.tau || !tr_draws) ? q.step_size : 4.f * q.step_size);
    for (unsigned i = slot; i < n; i += stride) {
        const size_t i3 = size_t(3) * i;
        if (want_point) {
            V3 sa = mk3(0.f), ss = mk3(0.f), st = mk3(0.f), le = mk3(0.f); float ph = 0.f;
            if (present) {
                const float RT_G *pp = RT_GPTR(const float, q.p) + i3;
                const V3 p = mk3(pp[0], pp[1], pp[2]);
                if (dens) {                                                     // DensityRegion, volume.h:72-90: Density(WorldToVolume(p)) times the constant
                    const float D = density_at(sc, xform_point(vol.world_to_volume, p));
                    sa = D * mat_color(vol.sigma_a); ss = D * mat_color(vol.sigma_s); le = D * mat_color(vol.le);
                    st = D * (mat_color(vol.sigma_a) + mat_color(vol.sigma_s));
                } else if (vol_inside(vol, p)) {                                // homogeneous.cpp:47-62
                    sa = mat_color(vol.sigma_a); ss = mat_color(vol.sigma_s); le = mat_color(vol.le);
                    st = mat_color(vol.sigma_a) + mat_color(vol.sigma_s);
                }
                if (q.phase && (dens || vol_inside(vol, p))) {                  // a density region's p() has no inside test (volume.h:84-86)
                    const float RT_G *a = RT_GPTR(const float, q.w) + i3, *b = RT_GPTR(const float, q.wp) + i3;
                    ph = phase_hg(mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), vol.g);
                }
            }
            if (q.sigma_a) store3(q.sigma_a, i3, sa);
            if (q.sigma_s) store3(q.sigma_s, i3, ss);
            if (q.sigma_t) store3(q.sigma_t, i3, st);
            if (q.lve) store3(q.lve, i3, le);
            if (q.phase) RT_GPTR(float, q.phase)[i] = ph;
        }
        if (!want_ray) continue;
        int hit = 0, draws = tr_draws ? 1 : 0, status = 0;
        float t0 = 0.f, t1 = 0.f;
        V3 tau = mk3(0.f), tr = mk3(1.f), lv = mk3(0.f);
        if (present) {
            const float4 a = RT_GPTR(const float4, q.rays)[size_t(2) * i], b = RT_GPTR(const float4, q.rays)[size_t(2) * i + 1];
            const V3 o = mk3(a.x, a.y, a.z), d = mk3(a.w, b.x, b.y); const float mint = b.z, maxt = b.w;
            uint32_t key = i, ctr = 0u;
            if (q.rng) { const uint32_t RT_G *r = RT_GPTR(const uint32_t, q.rng) + size_t(2) * i; key = r[0]; ctr = r[1]; }
            bool ok = false, bad = !ray_usable(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
            if (!bad) {
                ok = vol_intersect(vol, o, d, mint, maxt, t0, t1);              // VolumeRegion::IntersectP(ray, &t0, &t1)
                if (ok && !(ray_finite(t0) && ray_finite(t1))) { bad = true; ok = false; }
                if (!bad && want_march && dens) {                               // the interval DensityRegion::Tau marches: the ray normalised, then clipped
                    const float length = len3(d);
                    if (length != 0.f) {
                        const float inv = 1.f / length;
                        float n0, n1;
                        if (vol_intersect(vol, o, mk3(d.x * inv, d.y * inv, d.z * inv), mint * length, maxt * length, n0, n1) && !march_advances(n0, n1, min_step)) bad = true;
                    }
                }
            }
            hit = ok ? 1 : 0;                                                   // (an unusable ray or a non-finite interval: no hit; a march that cannot advance keeps its interval)
            if (!ok) t0 = t1 = 0.f;
            if (bad) { status = RT_MEDIUM_NO_ADVANCE; tr = mk3(0.f); }
            else {
                if (q.tau || (q.tr && q.u)) {                                   // Tau(ray, stepSize, u): homogeneous.cpp:63-67 ignores both, volume.cpp:137-153
                    if (dens) tau = density_tau_capped(sc, [tau_cap] { return tau_cap; }, o, d, mint, maxt, q.step_size, RT_GPTR(const float, q.u)[i]);
                    else if (ok) tau = (mat_color(vol.sigma_a) + mat_color(vol.sigma_s)) * len3((o + d * t0) - (o + d * t1));
                }
                if (q.tr) {
                    if (q.u) tr = dens ? exp_neg(tau) : vol_transmittance(vol, o, d, mint, maxt);     // Transmittance with a sample: no draw
                    else {                                                      // Scene::Transmittance(ray): the draw is made for a homogeneous region too
                        Rng rng; rng.base = rng_base(key, q.seed); rng.ctr = ctr;
                        const float u = rng.next_float();
                        tr = dens ? exp_neg(density_tau_capped(sc, [tau_cap] { return tau_cap; }, o, d, mint, maxt, 4.f * q.step_size, u)) : vol_transmittance(vol, o, d, mint, maxt);
                    }
                }
                if (q.lv && ok && (t1 - t0) != 0.f) {
                    const float Nf = ceilf((t1 - t0) / q.step_size);
                    if (!(Nf <= float(step_cap))) status = RT_MEDIUM_TOO_LONG;
                    else {
                        Rng rng; rng.base = rng_base(key, q.seed); rng.ctr = ctr;
                        lv = emission_march(sc, dens, o, d, t0, t1, int(Nf), q.step_size, RT_GPTR(const float, q.u_scatter)[i], rng, tau_cap);
                        const int moved = int(rng.ctr - ctr);
                        draws = moved > draws ? moved : draws;
                    }
                }
            }
        }
        if (q.hit) RT_GPTR(int, q.hit)[i] = hit;
        if (q.t01) { float RT_G *w = RT_GPTR(float, q.t01) + size_t(2) * i; w[0] = t0; w[1] = t1; }
        if (q.tau) store3(q.tau, i3, tau);
        if (q.tr) store3(q.tr, i3, tr);
        if (q.lv) store3(q.lv, i3, lv);
        if (q.draws) RT_GPTR(int, q.draws)[i] = draws;
        if (q.status) RT_GPTR(int, q.status)[i] = status;
    }
}

__global__ __launch_bounds__(RT_RAYS_BLOCK) void volume_samples_kernel(DevScene sc, DevFrame fr, unsigned long long first, unsigned count, uint4 *__restrict__ out) {
    const unsigned i = blockIdx.x * RT_RAYS_BLOCK + threadIdx.x;
    if (i >= count) return;
    const unsigned long long n = first + i;
    Lane ln; Ray r;
    ln.work = uint32_t(n);                                                      // one shard: the scanline index pixel * spp + s (dim_value's sample-in-pixel)
    setup_sample(sc, fr, ln, n / fr.spp, int(n % fr.spp), r);
    const float u_tau = dim_value(fr, ln, fr.one_d[fr.n1d - 2], 0, 0), u_scatter = dim_value(fr, ln, fr.one_d[fr.n1d - 1], 0, 0);
    RT_GPTR(uint4, out)[i] = make_uint4(__float_as_uint(u_tau), __float_as_uint(u_scatter), ln.sample_index, ln.rng.ctr);
}

}  // namespace rt

// ------------------------------------------------------------------------------------------ host side
int volume_samples_launch(RtScene *s, const rt::DevFrame &fr, unsigned long long first, unsigned count, uint32_t *dev_out) {
    if (int rc = pending_error()) return rc;
    hipLaunchKernelGGL(rt::volume_samples_kernel, dim3(blocks_for(count)), dim3(RT_RAYS_BLOCK), 0, s->stream, s->dev, fr, first, count, reinterpret_cast<uint4 *>(dev_out));
    HIPCHK(hipGetLastError());
    return RT_OK;
}

extern "C" {

int rt_medium_device(RtScene *s, uint32_t n, const RtMediumQuery *q) {
    static const std::string fn = "rt_medium_device";
    if (int rc = refuse_null(fn, s, "scene")) return rc;
    if (n > RT_RAYS_MAX_N) return fail(RT_EINVAL, fn + ": n = " + std::to_string(n) + " is above 2^30");
    if (n == 0) return RT_OK;
    if (int rc = refuse_null(fn, q, "RtMediumQuery")) return rc;
    const bool want_point = q->sigma_a || q->sigma_s || q->sigma_t || q->lve || q->phase;
    const bool want_ray = q->hit || q->t01 || q->tau || q->tr || q->lv || q->draws || q->status;
    if (!want_point && !want_ray) return fail(RT_EINVAL, fn + ": every output of the RtMediumQuery is null (nothing is wanted)");
    if (want_point && !q->p) return fail(RT_EINVAL, fn + ": sigma_a, sigma_s, sigma_t, lve or phase is wanted and p is null");
    if (q->phase && (!q->w || !q->wp)) return fail(RT_EINVAL, fn + ": phase is wanted and w or wp is null");
    if (want_ray && !q->rays) return fail(RT_EINVAL, fn + ": hit, t01, tau, tr, lv, draws or status is wanted and rays is null");
    if (want_ray) { if (int rc = refuse_unaligned16(fn, q->rays, "rays")) return rc; }
    if (q->tau && !q->u) return fail(RT_EINVAL, fn + ": tau is wanted and u is null");
    if (q->lv && !q->u_scatter) return fail(RT_EINVAL, fn + ": lv is wanted and u_scatter is null");
    if (q->lv && q->volume_integrator == RT_VOLUME_SINGLE)
        return fail(RT_EINVAL, fn + ": lv with volume_integrator = RT_VOLUME_SINGLE (SingleScattering::Li traces shadow rays: a frame's job, rt_radiance_device)");
    // Every march must end: the limits of plan_march (rt_frame_plan.h) over the volume's diagonal, handed to the kernel as loop caps
    MarchCaps caps;
    if (!s->facts.medium) { if (!march_step_ok(q->step_size)) return fail(RT_EINVAL, fn + ": step_size must be positive and finite"); }
    else {
        const plan::SceneFacts &sf = s->facts;
        const float ex = sf.vol_p1[0] - sf.vol_p0[0], ey = sf.vol_p1[1] - sf.vol_p0[1], ez = sf.vol_p1[2] - sf.vol_p0[2];
        const double *wb = sf.vol_world;
        const double wx = wb[3] - wb[0], wy = wb[4] - wb[1], wz = wb[5] - wb[2];
        switch (march_caps(q->step_size, std::sqrt(double(ex) * ex + double(ey) * ey + double(ez) * ez), std::sqrt(wx * wx + wy * wy + wz * wz),
                           sf.density_kind != RT_DENSITY_NONE, caps)) {
            case MARCH_BAD_STEP: return fail(RT_EINVAL, fn + ": step_size must be positive and finite");
            case MARCH_TOO_MANY_TAUS: return fail(RT_EINVAL, fn + ": step_size too small for the density region (an optical-depth march would take more than 2^20 samples)");
            case MARCH_TOO_MANY_STEPS: return fail(RT_EINVAL, fn + ": step_size too small for the medium (more than 65536 march steps)");
            default: break;
        }
    }
    HIPCHK(hipSetDevice(s->device));
    if (int rc = pending_error()) return rc;
    const unsigned lanes = std::max(s->n_threads, unsigned(RT_RAYS_BLOCK));
    const unsigned grid = std::min(blocks_for(n), lanes / RT_RAYS_BLOCK);
    // a caller's ray may cross a scaled homogeneous box in more steps than the box's own diagonal has: the emission march is capped at plan_march's limit itself
    hipLaunchKernelGGL(medium_query_kernel, dim3(grid), dim3(RT_RAYS_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, n, *q, int(RT_MARCH_MAX_STEPS), caps.taus);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

}  // extern "C"
