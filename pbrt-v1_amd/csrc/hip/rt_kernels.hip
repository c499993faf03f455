// rt_kernels.hip -- the render path of libpbrt_hip.so's C ABI (include/pbrt_hip.h): make_frame (the binder of what rt_frame_plan.h plans), launch_persistent (the one launch of the kernel plan_launch chose), the queue pipeline, rt_render, rt_trace_*.
// (Scene create: rt_scene.hip.  Film kernels and rt_film_*: rt_film.hip.  Shared host declarations: rt_host.h.  Which kernel instantiation: rt_flavour.h.)
//
// Kernels
//   render_kernel   persistent-thread wavefront renderer: Scene::Render's sample loop (scene.cpp:42-84).
//                   Every lane runs the state machine of rt_integrate.h; all lanes of a wave share ONE
//                   kd-tree traversal loop (rt_traverse.h) whatever kind of ray they carry (camera,
//                   bounce, MIS closest-hit, shadow any-hit); finished lanes refill from a global work
//                   counter with one wave-aggregated atomic.  No MFMA: the work is pointer chasing and
//                   3-vector arithmetic, bounded by HBM/L2 latency and bandwidth, not by dense math.
//   (rt_pipeline.h) pipe_shade_kernel / pipe_trace_kernel: the queue pipeline used for large scenes; rt_trace_closest / rt_trace_any
//                   (unit parity entry points) run caller-supplied rays through the same pipe_trace_kernel.
//   camera_kernel   Sampler + Camera::GenerateRay only.
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (parity with the reference's non-FMA build).
#include "rt_host.h"
#include "rt_weighted.h"

namespace rt {
__global__ void camera_kernel(DevScene sc, DevFrame fr, unsigned long long first, unsigned count, RtRay *out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const unsigned long long n = first + i;
    Lane ln; Ray r;
    setup_sample(sc, fr, ln, n / fr.spp, int(n % fr.spp), r);
    out[i].o[0] = r.o.x; out[i].o[1] = r.o.y; out[i].o[2] = r.o.z;
    out[i].d[0] = r.d.x; out[i].d[1] = r.d.y; out[i].d[2] = r.d.z;
    out[i].mint = r.mint; out[i].maxt = r.maxt;
}

}  // namespace rt

// ------------------------------------------------------------------------------------------ host side
namespace rt {
const char *knob(const char *name) {
#ifdef RT_NO_TUNABLES
    (void)name; return nullptr;
#else
    static const bool on = std::getenv("PBRT_HIP_TUNE") != nullptr;
    return on ? std::getenv(name) : nullptr;
#endif
}
static thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }
const char *last_error() { return g_err.c_str(); }
void hip_warn(hipError_t e, const char *what) {
    if (e != hipSuccess) std::fprintf(stderr, "libpbrt_hip: %s failed: %s\n", what, hipGetErrorString(e));
}
// what the owners of rt_devbuf.h / rt_host.h allocate and release through
int dev_alloc(void **p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return RT_OK;
    *p = nullptr;
    return fail(RT_EDEVICE, "hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
}
void dev_free(void *p) { HIPWARN(hipFree(p)); }
void host_free(void *p) { HIPWARN(hipHostFree(p)); }
void event_free(void *e) { HIPWARN(hipEventDestroy(static_cast<hipEvent_t>(e))); }
void stream_free(void *st) { HIPWARN(hipStreamDestroy(static_cast<hipStream_t>(st))); }
}  // namespace rt

// The scratch of the state machine per thread (megakernel) or slot (pipeline), in words: recursion frames (whitted / directlighting; the bidirectional
// integrator: its path vertices), the medium's [vol_levels x 8 rays | 13 state | the single-scattering march samples], and the levels of materials
// resolved per hit (rt_texture.h).  fr.vol_nmax is what rt_render's validation found.
struct ScratchWords { size_t frame = 0, vol_levels = 0, vol = 0, mat_levels = 0; };
static ScratchWords scratch_words(const RtScene *s, const RtRenderDesc *rd, const DevFrame &fr) {
    // (the debug integrator recurses no more than the path integrator does: no frames, one level of the medium's rays)
    const bool bidir = rd->integrator == RT_INTEGRATOR_BIDIRECTIONAL, path = rd->integrator == RT_INTEGRATOR_PATH || rd->integrator == RT_INTEGRATOR_DEBUG;
    ScratchWords w;
    w.frame = bidir ? size_t(RT_BD_FRAME_WORDS) : path ? 0 : size_t(rd->max_depth + 2) * RT_FRAME_WORDS;
    w.mat_levels = bidir ? size_t(2 * RT_BD_MAX_VERTS) : path ? 1 : size_t(rd->max_depth + 2);
    if (s->volume.present) {
        w.vol_levels = path ? 1 : size_t(rd->max_depth + 2);
        w.vol = w.vol_levels * 8 + 13 + (rd->volume_integrator == RT_VOLUME_SINGLE ? size_t(3) * fr.vol_nmax : 0);
    }
    return w;
}
// ... grown for n threads / slots and bound to the frame
static int bind_scratch(RtScene *s, const RtRenderDesc *rd, DevFrame &fr, size_t n) {
    const ScratchWords w = scratch_words(s, rd, fr);
    int rc;
    if ((rc = ensure(s, s->frames, w.frame * n))) return rc;
    if ((rc = ensure(s, s->vol_buf, w.vol * n))) return rc;
    fr.frames = s->frames; fr.n_threads = unsigned(n);
    if (w.vol) { fr.vol_rays = s->vol_buf; fr.vol_state = fr.vol_rays + w.vol_levels * 8 * n; fr.vol_samp = fr.vol_state + size_t(13) * n; }
    return ensure_material_pool(s, fr, w.mat_levels, n);
}

// The kernel and resident grid of a planned launch (rt_host.h persistent_kernel); a variant the scene has no grid for is refused
static int resident_kernel(const RtScene *s, const plan::Launch &ln, PersistentKernel &pk) {
    pk = persistent_kernel(s->grids, ln);
    return pk.grid ? RT_OK : fail(RT_ESTATE, "render kernel variant has no resident grid");
}
// One launch of a persistent kernel on the scene's stream: the descriptor to `dev_fr` (the frame's, or a query's own), the work counters zeroed, `staged`
// (where the caller times from there: ev0 of a megakernel frame) recorded, the kernel over its resident grid
static int launch_persistent(RtScene *s, const PersistentKernel &pk, const DevFrame &fr, DevFrame *dev_fr, hipEvent_t staged = nullptr) {
    HIPCHK(hipMemcpyAsync(dev_fr, &fr, sizeof(DevFrame), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemsetAsync(s->work_counter, 0, 64 * sizeof(unsigned long long), s->stream));
    if (staged) HIPCHK(hipEventRecord(staged, s->stream));
    hipLaunchKernelGGL(pk.fn, dim3(pk.grid), dim3(RT_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, (const DevFrame *)dev_fr);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// The queue pipeline: alternate a shade kernel (pipe_shade_kernel, or pipe_vertex_kernel for a path without a medium) and pipe_trace_kernel
// until a shade pass enqueues no ray.  The host learns the queue sizes RT_PIPE_BATCH iterations late (page-locked copy + fence event per
// batch), so the GPU never waits for it; the iterations launched after the last productive one find every slot in ST_EXIT and return at once.
static int render_pipeline(RtScene *s, const RtRenderDesc *rd, DevFrame &fr, const plan::Schedule &sc, const plan::FrameKnobs &kn, LastLaunch &ll) {
    const int integ = rd->integrator;
    const bool by_vertex = sc.by_vertex;          // PathIntegrator without a medium: one shade pass per path vertex (plan_schedule)
    // ---- pool size: 32 M slots with a medium, 8 M without, unless the frame is smaller or the per-slot scratch would not fit (a fine ray march: 3 floats per step)
    const ScratchWords w = scratch_words(s, rd, fr);
    size_t slot_bytes = (w.frame + w.vol) * 4 + (s->has_textures ? w.mat_levels * sizeof(DevMaterial) : 0);   // ... and the materials resolved per hit
    size_t held = s->frames.bytes() + s->vol_buf.bytes();                        // what this scene's pool already holds
    s->pool.each([&](auto &b, size_t per_slot) { slot_bytes += per_slot * sizeof(*b.p); held += b.bytes(); });
    // (C5, 64 spp with a march per ray: 8 M slots 329 ms, 16 M 311, 32 M 289, 48 M 312, 64 M 326 -- fewer, fuller iterations until the shade passes' state
    // traffic takes over; the by-vertex path frame on the 1 M tree: 8 M 70.6 ms, 16 M 72.1; profiles/r03_c5_knobs.txt)
    unsigned want = s->volume.present ? 1u << 25 : 1u << 23;
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        size_t budget = (free_b + held) / 2;                                      // leave half of what is free to the caller (film, other scenes)
        if (kn.pipe_mem_mb) budget = size_t(std::max(1, *kn.pipe_mem_mb)) << 20;      // tests: a small budget
        if (slot_bytes * want > budget) want = unsigned(std::max<size_t>(budget / slot_bytes, 2 * RT_BLOCK));
    }
    if (kn.pipe_slots) want = unsigned(std::max(256, *kn.pipe_slots));
    unsigned long long tw = fr.total_work ? fr.total_work : 1;
    unsigned n_slots = unsigned(std::min<unsigned long long>(want, tw));
    n_slots = (n_slots + RT_BLOCK - 1) / RT_BLOCK * RT_BLOCK;
    if (n_slots >= (1u << 30)) return fail(RT_EINVAL, "rt_render: more than 2^30 pipeline slots");
    int rc = RT_OK;
    s->pool.each([&](auto &b, size_t per_slot) { if (!rc) rc = ensure(s, b, per_slot * n_slots); });
    if (!rc) rc = ensure(s, s->wave_work, size_t(n_slots / 64 + 1) * 2);
    if (!rc) rc = s->q_count.grow(size_t(RT_PIPE_QN) * RT_QC_STRIDE);
    if (rc) return rc;
    PipePool pl{};                                                          // the kernels' view of the pool
    pl.n_slots = n_slots; pl.state = s->pool.state; pl.hit = s->pool.hit; pl.q_count = s->q_count; pl.wave_work = s->wave_work;
    pl.ray_o = s->pool.ray_o; pl.ray_d = pl.ray_o + n_slots; pl.q_o = s->pool.q_o; pl.q_d = pl.q_o + size_t(2) * n_slots;
    pl.q_slot = s->pool.q_slot; pl.q_march = pl.q_slot + size_t(2) * n_slots;
    if (by_vertex) pl.ray_d = pl.q_o;                                       // directions [3][n_slots] (the compacted ray copies are not used)
    if ((rc = bind_scratch(s, rd, fr, n_slots))) return rc;
    if (s->pipe_ev.empty()) {
        s->pipe_ev.resize(6 * RT_PIPE_TIMED); s->pipe_fence.resize(RT_PIPE_QN / RT_PIPE_BATCH);
        for (auto &e : s->pipe_ev) HIPCHK(hipEventCreate(&e.p));
        for (auto &e : s->pipe_fence) HIPCHK(hipEventCreateWithFlags(&e.p, hipEventDisableTiming));
    }
    const flavour::Request rq = plan::request(rd, s->facts, &sc);
    const PipeShadeFn shade = by_vertex ? g_pipe_vertex[flavour::Vertex::index(rq)] : (*g_pipe_shade[integ])[flavour::Shade::index(rq)];
    const int tk = flavour::Trace::index(rq);
    const PipeTraceFn trace = g_pipe_trace[tk];
    const unsigned trace_grid = s->grids.trace[tk];
    // frames with a medium: the march kernel (rt_pipe_march.h) runs the ray marches the shade pass parked
    const bool marches = s->volume.present;
    const int mk = flavour::March::index(rq);
    const unsigned march_grid = s->grids.march[mk];
    HIPCHK(hipMemcpyAsync(s->dev_frame, &fr, sizeof(DevFrame), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemcpyAsync(s->dev_pool, &pl, sizeof(PipePool), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemsetAsync(s->work_counter, 0, sizeof(unsigned long long), s->stream));
    HIPCHK(hipMemsetAsync(pl.state + n_slots, 0, size_t(n_slots) * sizeof(float4), s->stream));      // control words: every slot in ST_FETCH
    HIPCHK(hipMemsetAsync(pl.wave_work, 0, size_t(n_slots / 64 + 1) * 2 * sizeof(unsigned long long), s->stream));
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    int iter = 0, checked = 0, batch = 0;
    bool done = false;
    const int max_iters = 1 << 20;
    while (!done) {
        for (int k = 0; k < RT_PIPE_BATCH; ++k, ++iter) {
            const unsigned qi = unsigned(iter % RT_PIPE_QN);
            PipeLaunch pk{}; pk.qi = qi; pk.slot_base = 0; pk.q_base = 0;
            HIPCHK(hipMemsetAsync(pl.q_count + size_t(RT_QC_STRIDE) * qi, 0, RT_QC_STRIDE * sizeof(unsigned), s->stream));
            if (iter < RT_PIPE_TIMED) HIPCHK(hipEventRecord(s->pipe_ev[6 * iter + 2], s->stream));
            hipLaunchKernelGGL(shade, dim3(n_slots / RT_BLOCK), dim3(RT_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene,
                               (const DevFrame *)s->dev_frame, (const PipePool *)s->dev_pool, pk);
            if (iter < RT_PIPE_TIMED) HIPCHK(hipEventRecord(s->pipe_ev[6 * iter + 3], s->stream));
            TraceJob job{};
            job.q_o = pl.q_o; job.q_d = pl.q_d; job.q_slot = pl.q_slot; job.q_count = pl.q_count + size_t(RT_QC_STRIDE) * qi; job.hit = pl.hit;
            job.n_slots = n_slots; job.q_base = pk.q_base; job.spill = s->spill; job.n_threads = s->n_threads; job.counters = s->counters;
            if (by_vertex) { job.by_slot = 1; job.q_o = pl.ray_o; job.q_d = pl.ray_d; }
            if (iter < RT_PIPE_TIMED) HIPCHK(hipEventRecord(s->pipe_ev[6 * iter], s->stream));
            hipLaunchKernelGGL(trace, dim3(trace_grid), dim3(RT_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, job);
            if (iter < RT_PIPE_TIMED) HIPCHK(hipEventRecord(s->pipe_ev[6 * iter + 1], s->stream));
            if (marches) {
                MarchJob mj{};
                mj.q_march = pl.q_march; mj.q_count = pl.q_count + size_t(RT_QC_STRIDE) * qi;
                mj.spill = s->spill; mj.n_threads = s->n_threads; mj.counters = s->counters;
                if (iter < RT_PIPE_TIMED) HIPCHK(hipEventRecord(s->pipe_ev[6 * iter + 4], s->stream));
                hipLaunchKernelGGL(g_pipe_march[mk], dim3(march_grid), dim3(RT_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, (const DevFrame *)s->dev_frame,
                                   (const PipePool *)s->dev_pool, mj);
                if (iter < RT_PIPE_TIMED) HIPCHK(hipEventRecord(s->pipe_ev[6 * iter + 5], s->stream));
            }
            HIPCHK(hipMemcpyAsync(s->h_qcount + size_t(RT_QC_STRIDE) * qi, pl.q_count + size_t(RT_QC_STRIDE) * qi, (RT_QC_MARCH + 1) * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->pipe_fence[batch % (RT_PIPE_QN / RT_PIPE_BATCH)], s->stream));
        if (batch >= 1) {                                                   // look at the batch before the one just launched
            HIPCHK(hipEventSynchronize(s->pipe_fence[(batch - 1) % (RT_PIPE_QN / RT_PIPE_BATCH)]));
            for (int k = 0; k < RT_PIPE_BATCH; ++k, ++checked) {
                const unsigned *q = s->h_qcount + size_t(RT_QC_STRIDE) * (checked % RT_PIPE_QN);
                if (q[0] + q[RT_QC_ANY] + q[RT_QC_MARCH] == 0) { done = true; break; }
            }
        }
        ++batch;
        if (iter > max_iters) return fail(RT_ESTATE, "rt_render: the queue pipeline did not terminate");
    }
    ll.pipeline = true; ll.marches = marches;
    ll.slots = n_slots; ll.iterations = checked + 1; ll.timed_iterations = std::min(ll.iterations, RT_PIPE_TIMED);
    HIPCHK(hipEventRecord(s->ev1, s->stream));
    return RT_OK;
}

// One launch of the persistent kernel plan_launch chose: the megakernel rt::render_kernel of Whitted, DirectLighting "all" / "one", Path (generic, or a twin
// compiled for a fixed frame and scene) and the debug integrator, or the bidirectional integrator's rt::bidir_kernel (rt_bidir.h: the eight path vertices
// of every thread in s->frames)
static int render_mega(RtScene *s, const RtRenderDesc *rd, DevFrame &fr, const plan::Launch &ln) {
    int rc = bind_scratch(s, rd, fr, s->n_threads); if (rc) return rc;
    PersistentKernel pk; if ((rc = resident_kernel(s, ln, pk))) return rc;
#ifdef RT_TAIL_PROBE
    static unsigned long long *probe = nullptr;
    const size_t n_waves = size_t(pk.grid) * (RT_BLOCK / 64);
    if (!probe) HIPCHK(hipMalloc((void **)&probe, size_t(s->n_threads / 64 + 64) * 4 * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(probe, 0, n_waves * 4 * sizeof(unsigned long long), s->stream));
    fr.probe = probe;
#endif
    if ((rc = launch_persistent(s, pk, fr, s->dev_frame, s->ev0))) return rc;
    HIPCHK(hipEventRecord(s->ev1, s->stream));
#ifdef RT_TAIL_PROBE
    {   // the launch's timeline: when the waves started, when each found the work list empty, when each ended (10 ns ticks of s_memrealtime)
        std::vector<unsigned long long> h(n_waves * 4);
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipMemcpy(h.data(), probe, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t0max = 0, e0 = ~0ull, e1 = 0, x1 = 0, smin = ~0ull, smax = 0, stot = 0;
        std::vector<double> ends, drain;
        for (size_t w = 0; w < n_waves; ++w) {
            const unsigned long long *r = &h[4 * w];
            if (!r[2]) continue;
            t0 = std::min(t0, r[0]); t0max = std::max(t0max, r[0]); x1 = std::max(x1, r[2]);
            if (r[1]) { e0 = std::min(e0, r[1]); e1 = std::max(e1, r[1]); drain.push_back(double(r[2] - r[1]) * 1e-2); }
            smin = std::min(smin, r[3]); smax = std::max(smax, r[3]); stot += r[3];
            ends.push_back(double(r[2]));
        }
        std::sort(ends.begin(), ends.end()); std::sort(drain.begin(), drain.end());
        auto q = [&](const std::vector<double> &v, double f) { return v.empty() ? 0.0 : v[size_t(f * (v.size() - 1))]; };
        std::fprintf(stderr, "RT_TAIL_PROBE waves=%zu span=%.1f us | starts spread %.1f us | list first seen empty at %.1f us, last at %.1f us | wave ends (us after start): p1 %.1f p10 %.1f p50 %.1f p90 %.1f p99 %.1f max %.1f | "
                             "drain per wave (end - empty, us): p10 %.1f p50 %.1f p90 %.1f p99 %.1f max %.1f | samples per wave min %llu mean %.1f max %llu\n",
                     ends.size(), double(x1 - t0) * 1e-2, double(t0max - t0) * 1e-2, double(e0 - t0) * 1e-2, double(e1 - t0) * 1e-2,
                     (q(ends, .01) - double(t0)) * 1e-2, (q(ends, .1) - double(t0)) * 1e-2, (q(ends, .5) - double(t0)) * 1e-2, (q(ends, .9) - double(t0)) * 1e-2, (q(ends, .99) - double(t0)) * 1e-2, (q(ends, 1.) - double(t0)) * 1e-2,
                     q(drain, .1), q(drain, .5), q(drain, .9), q(drain, .99), q(drain, 1.), smin, double(stot) / double(std::max<size_t>(ends.size(), 1)), smax);
    }
#endif
    return RT_OK;
}

// DirectLighting "weighted" (rt_weighted.h): count -> scan -> survey -> recurrence -> the frame.  ev0 .. ev1 bracket all of it (kernel_ms of a weighted frame
// is the five together)
static int render_weighted(RtScene *s, const RtRenderDesc *rd, DevFrame &fr, const plan::Launch &ln, LastLaunch &ll) {
    int rc = bind_scratch(s, rd, fr, s->n_threads); if (rc) return rc;
    PersistentKernel pk; if ((rc = resident_kernel(s, ln, pk))) return rc;
    const int nL = int(s->dev.n_lights), R = 1 + 2 * nL;
    if (!s->wt_total) HIPCHK(hipHostMalloc((void **)&s->wt_total.p, sizeof(unsigned long long), hipHostMallocDefault));
    if ((rc = s->wt_sums.grow(RT_WSCAN_BLOCKS))) return rc;
    for (Event &e : s->wt_ev) if (!e) HIPCHK(hipEventCreate(&e.p));
    rc = ensure(s, s->wt_base, size_t(fr.total_work) + 1); if (rc) return rc;
    fr.wt_base = s->wt_base;
    auto pass = [&](int phase) -> int { fr.weighted_phase = phase; return launch_persistent(s, pk, fr, s->dev_frame); };
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    if ((rc = pass(1))) return rc;
    HIPCHK(hipEventRecord(s->wt_ev[0], s->stream));
    hipLaunchKernelGGL(weighted_scan_sums_kernel, dim3(RT_WSCAN_BLOCKS), dim3(RT_WSCAN_THREADS), 0, s->stream, (const unsigned *)s->wt_base, (unsigned long long)fr.total_work, s->wt_sums);
    hipLaunchKernelGGL(weighted_scan_top_kernel, dim3(1), dim3(RT_WSCAN_THREADS), 0, s->stream, s->wt_base, (unsigned long long)fr.total_work, s->wt_sums, s->wt_total);
    hipLaunchKernelGGL(weighted_scan_apply_kernel, dim3(RT_WSCAN_BLOCKS), dim3(RT_WSCAN_THREADS), 0, s->stream, s->wt_base, (unsigned long long)fr.total_work, (const unsigned long long *)s->wt_sums);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->wt_ev[1], s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    const unsigned long long n_points = *s->wt_total;
    // The one place where rt_render can fail AFTER it has launched work (the number of shading points is only known once the count pass has run;
    // pbrt_hip.h says so): the film and the sample buffer are untouched (the count pass writes neither), the scene is left without a last frame.
    auto late_fail = [&](int code, const char *msg) { s->last = LastLaunch{}; return fail(code, msg); };
    if (n_points >= 0xffffffffull) return late_fail(RT_EINVAL, "rt_render: strategy \"weighted\": more than 2^32 - 2 shading points in the frame");
    ll.weighted = true; ll.weighted_points = n_points;
    const bool mixed = s->facts.light_draws < 0;
    const int nD = int(s->n_drawing_lights);
    size_t rec_floats = size_t(n_points) * size_t(R);
    fr.wt_mixed = mixed ? 1 : 0; fr.wt_nd = unsigned(nD); fr.wt_recbase = nullptr;
    if (mixed) {
        // A sample with P shading points keeps P * A + nD * P * (P + 1) floats: quadratic in P, and sum P (P + 1) >= W * Pavg * (Pavg + 1) for W samples of
        // Pavg points on average (convexity) -- a frame that cannot fit even by that lower bound is refused here, before the size scan is launched
        {
            const double W = double(fr.total_work ? fr.total_work : 1), Pavg = double(n_points) / W;
            const double at_least = double(n_points) * double(1 + 2 * (nL - nD)) + double(nD) * W * Pavg * (Pavg + 1.0);
            if (at_least >= 4294967295.0) return late_fail(RT_EINVAL, "rt_render: strategy \"weighted\" with lights of mixed RNG use: the survey's records exceed 2^32 floats (quadratic in a sample's shading points)");
        }
        // where every sample's records start: per-sample sizes from the point counts (P * A + nD * P * (P + 1)), scanned like the counts were
        rc = ensure(s, s->wt_recbase, size_t(fr.total_work) + 1); if (rc) return late_fail(rc, rt::last_error());
        const unsigned long long nw = fr.total_work;
        if (nw) hipLaunchKernelGGL(weighted_sizes_kernel, dim3(unsigned((nw + 255) / 256)), dim3(256), 0, s->stream, (const unsigned *)s->wt_base, nw, unsigned(1 + 2 * (nL - nD)), unsigned(nD), s->wt_recbase);
        hipLaunchKernelGGL(weighted_scan_sums_kernel, dim3(RT_WSCAN_BLOCKS), dim3(RT_WSCAN_THREADS), 0, s->stream, (const unsigned *)s->wt_recbase, nw, s->wt_sums);
        hipLaunchKernelGGL(weighted_scan_top_kernel, dim3(1), dim3(RT_WSCAN_THREADS), 0, s->stream, s->wt_recbase, nw, s->wt_sums, s->wt_total);
        hipLaunchKernelGGL(weighted_scan_apply_kernel, dim3(RT_WSCAN_BLOCKS), dim3(RT_WSCAN_THREADS), 0, s->stream, s->wt_recbase, nw, (const unsigned long long *)s->wt_sums);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->stream));
        if (*s->wt_total >= 0xffffffffull) return late_fail(RT_EINVAL, "rt_render: strategy \"weighted\" with lights of mixed RNG use: the survey's records exceed 2^32 floats");
        rec_floats = size_t(*s->wt_total);
        fr.wt_recbase = s->wt_recbase;
    }
    rc = ensure(s, s->wt_rec, rec_floats + 1); if (rc) return late_fail(rc, rt::last_error());
    rc = ensure(s, s->wt_pick, size_t(n_points) + 1); if (rc) return late_fail(rc, rt::last_error());
    fr.wt_rec = s->wt_rec; fr.wt_pick = s->wt_pick;
    if (n_points > 0) {
        if ((rc = pass(2))) return rc;
        HIPCHK(hipEventRecord(s->wt_ev[2], s->stream));
        // LDS of the recurrence kernel: [state | chunk records | chunk picks] within 64 KB
        const size_t state_f = nL <= 64 ? 0 : size_t((3 * nL + 2) & ~1);
        int chunk = int((size_t(64) * 1024 / 4 - state_f - 2) / size_t(R + 2));
        chunk = chunk > 1024 ? 1024 : chunk < 1 ? 1 : chunk;
        const size_t lds = (state_f + size_t((chunk * R + 1) & ~1) + size_t(chunk) * 2) * sizeof(float);
        if (mixed) {
            // LDS of the general form: [5 nL + 1 state | 2 x (group + 1) sample offsets | staged records | staged picks] within 64 KB
            const int group = 256;
            const size_t fixed = size_t(5 * nL + 2) + 2 * size_t(group + 1);
            const size_t room = size_t(64) * 1024 / 4 - fixed - 4;
            const int cap_points = int(room / 4 / 2), cap_floats = int(room - size_t(cap_points) * 2) & ~1;     // a quarter of the room for the picks (2 floats each)
            const size_t mlds = (fixed + size_t(cap_floats) + 2 + size_t(cap_points) * 2) * sizeof(float);
            hipLaunchKernelGGL(weighted_recurrence_mixed_kernel, dim3(1), dim3(64), mlds, s->stream, (const float *)s->wt_rec, s->wt_pick, (const unsigned *)s->wt_base,
                               (const unsigned *)s->wt_recbase, (unsigned long long)fr.total_work, nL, nD, s->light_draw_flags, group, cap_floats, cap_points);
        } else {
            auto rk = nL <= 64 ? weighted_recurrence_lanes_kernel : weighted_recurrence_lds_kernel;      // light i in lane i | tables in LDS, one lane
            hipLaunchKernelGGL(rk, dim3(1), dim3(64), lds, s->stream, (const float *)s->wt_rec, s->wt_pick, n_points, nL, chunk);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->wt_ev[3], s->stream));
    } else { HIPCHK(hipEventRecord(s->wt_ev[2], s->stream)); HIPCHK(hipEventRecord(s->wt_ev[3], s->stream)); }
    if ((rc = pass(3))) return rc;
    HIPCHK(hipEventRecord(s->ev1, s->stream));
    return RT_OK;
}

extern "C" {


const char *rt_last_error(void) { return rt::last_error(); }

int rt_device_count(int *count) {
    if (!count) return fail(RT_EINVAL, "rt_device_count: null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(RT_EDEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *count = n; return RT_OK;
}
// The PBRT_HIP_* knobs of the render path as values (rt_frame_plan.h FrameKnobs), read through knob(), so that PBRT_HIP_TUNE gates them: the one
// place in this file that names them
static plan::FrameKnobs frame_knobs() {
    auto num = [](const char *name) -> std::optional<int> { const char *e = knob(name); return e ? std::optional<int>(std::atoi(e)) : std::nullopt; };
    plan::FrameKnobs k;
    k.high_occ = num("PBRT_HIP_HIGH_OCC"); k.leaf_min = num("PBRT_HIP_LEAF_MIN"); k.trav_mode = num("PBRT_HIP_TRAV_MODE");
    k.xcd_bands = num("PBRT_HIP_XCD_BANDS"); k.exit_thresh = num("PBRT_HIP_EXIT_THRESH"); k.phase_sync = num("PBRT_HIP_PHASE_SYNC");
    k.pipeline = num("PBRT_HIP_PIPELINE"); k.mega_tile = num("PBRT_HIP_MEGA_TILE"); k.fixed_frame = num("PBRT_HIP_FIXED_FRAME");
    k.pipe_vertex = num("PBRT_HIP_PIPE_VERTEX"); k.pipe_mem_mb = num("PBRT_HIP_PIPE_MEM_MB"); k.pipe_slots = num("PBRT_HIP_PIPE_SLOTS");
    k.debug_nofilm = num("PBRT_HIP_DEBUG_NOFILM");
    if (const char *e = knob("PBRT_HIP_DEBUG_PIXEL")) std::sscanf(e, "%d,%d", &k.dbg_x, &k.dbg_y);
    return k;
}

// The descriptor's sampler, film window and work extent, with the divisors of the work fetch (rt_fastdiv.h; they are these frame constants only, and
// nothing in make_frame or rt_render changes one of them afterwards): all a camera ray needs (camera_frame), and where make_frame starts
static void bind_extent(const RtRenderDesc *rd, const plan::Extent &e, int mega_tile, DevFrame &fr) {
    std::memset(&fr, 0, sizeof fr);
    fr.integrator = rd->integrator; fr.max_depth = rd->max_depth; fr.strategy = rd->strategy;
    fr.volume_integrator = rd->volume_integrator; fr.step_size = rd->step_size;
    fr.sampler = rd->sampler; fr.xs = rd->x_samples; fr.ys = rd->y_samples; fr.jitter = rd->jitter;
    fr.spp = e.spp;
    fr.seed = rd->seed;
    fr.x_pixel_start = rd->x_pixel_start; fr.y_pixel_start = rd->y_pixel_start;
    fr.x_pixel_count = rd->x_pixel_count; fr.y_pixel_count = rd->y_pixel_count;
    fr.x_start = rd->x_start; fr.x_end = rd->x_end; fr.y_start = rd->y_start; fr.y_end = rd->y_end;
    fr.fxw = rd->filter_x_width; fr.fyw = rd->filter_y_width;
    fr.inv_fxw = 1.f / fr.fxw; fr.inv_fyw = 1.f / fr.fyw;
    fr.shard_index = e.shard_index; fr.shard_count = e.shard_count; fr.tile_pixels = e.tile_pixels;
    fr.tile_w = e.tile_w; fr.tile_h = e.tile_h; fr.tiles_x = e.tiles_x;
    fr.total_pixels = e.total_pixels; fr.total_work = e.total_work;
    fr.mega_tile = mega_tile;
    fr.div = framediv_make(unsigned(fr.spp), unsigned(fr.xs), unsigned(fr.x_end - fr.x_start), unsigned(fr.y_end - fr.y_start), unsigned(fr.mega_tile),
                           (unsigned long long)fr.tile_pixels * fr.spp, unsigned(fr.tile_w), unsigned(fr.tiles_x));
}

// The frame of rt_camera_rays / rt_camera_rays_device: a camera ray depends on the sampler, the film and the camera, not on the integrator's sample
// requests (setup_sample, rt_integrate.h), so no request table is planned, and nothing is copied or waited for
static int camera_frame(const RtRenderDesc *rd, DevFrame &fr) {
    plan::Extent ext;
    if (plan::Refusal r = plan::plan_extent(*rd, ext)) return fail(r.code, r.msg);
    bind_extent(rd, ext, 0, fr);
    return RT_OK;
}

// Build the per-frame device descriptor: what rt_frame_plan.h plans for the frame (work extent, sample requests, schedule; `sc` keeps the host-side
// choices), bound to the scene's device memory.
static int make_frame(RtScene *s, const RtRenderDesc *rd, const plan::FrameKnobs &kn, DevFrame &fr, plan::Schedule &sc, bool need_film, const plan::QueryRange *query = nullptr) {
    plan::Extent ext; plan::Requests rq;
    if (plan::Refusal r = plan::plan_extent(*rd, ext)) return fail(r.code, r.msg);
    if (plan::Refusal r = plan::plan_requests(*rd, s->facts, ext.spp, rq)) return fail(r.code, r.msg);
    sc = plan::plan_schedule(*rd, s->facts, ext, rq, kn);
    if (query) { if (plan::Refusal r = plan::plan_query(*rd, *query, sc)) return fail(r.code, r.msg); }      // rt_radiance_device: the frame's sample set, the caller's rays as the work
    bind_extent(rd, sc.extent, sc.mega_tile, fr);
    fr.n1d = rq.n1d; fr.n2d = rq.n2d; fr.lhs_total = rq.lhs_total; fr.pixgen_draws = rq.pixgen_draws; fr.dims_max_n = rq.dims_max_n;
    std::memcpy(fr.one_d, rq.one_d, sizeof fr.one_d); std::memcpy(fr.two_d, rq.two_d, sizeof fr.two_d);
    fr.trav_mode = sc.trav_mode; fr.exit_thresh = sc.exit_thresh; fr.high_occupancy = sc.high_occupancy; fr.leaf_min = sc.leaf_min;
    fr.xcd_bands = sc.xcd_bands; fr.phase_sync = sc.phase_sync; fr.pipeline = sc.pipeline; fr.dbg_x = sc.dbg_x; fr.dbg_y = sc.dbg_y;
    if (!rq.table.empty()) {
        std::vector<DimReq> &up = s->light_dims_host;          // what the device holds: uploaded again only when a frame asks for other requests
        if (!s->light_dims || up.size() != rq.table.size() || std::memcmp(up.data(), rq.table.data(), rq.table.size() * sizeof(DimReq)) != 0) {
            int rc = ensure(s, s->light_dims, rq.table.size()); if (rc) return rc;
            up.swap(rq.table);
            // rt_render is asynchronous: a frame queued earlier may still be reading the table, and the source is pageable host memory that the next make_frame
            // may swap away -- wait for the stream, then copy synchronously (36 bytes per light; only when a frame asks for other requests than the last one)
            HIPCHK(hipStreamSynchronize(s->stream));
            HIPCHK(hipMemcpy(s->light_dims, up.data(), up.size() * sizeof(DimReq), hipMemcpyHostToDevice));
        }
        fr.light_dims = s->light_dims;
    }
    fr.filter_table = s->filter_dev; fr.accum = s->accum;
    fr.work_counter = s->work_counter; fr.counters = s->counters; fr.spill = s->spill; fr.n_threads = s->n_threads;
    fr.frames = s->frames;
    if (need_film && !s->accum) return fail(RT_ESTATE, "rt_render: no film bound (call rt_film_bind first)");
    if (need_film && (fr.x_pixel_count != s->film_w || fr.y_pixel_count != s->film_h))
        return fail(RT_EINVAL, "rt_render: film size does not match the bound film");
    return RT_OK;
}

int rt_camera_rays(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, RtRay *rays_out) {
    if (!s || !rd || !rays_out) return fail(RT_EINVAL, "null argument");
    HIPCHK(hipSetDevice(s->device));
    DevFrame fr; int rc = camera_frame(rd, fr); if (rc) return rc;
    DevBuf<RtRay> dev;
    if ((rc = dev.grow(count ? count : 1))) return rc;
    hipLaunchKernelGGL(camera_kernel, dim3((count + 255) / 256), dim3(256), 0, s->stream, s->dev, fr,
                       (unsigned long long)first, count, dev.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(rays_out, dev, size_t(count) * sizeof(RtRay), hipMemcpyDeviceToHost));
    return RT_OK;
}
// The same into the caller's DEVICE buffer, asynchronous on the scene's stream: no allocation, no copy, no wait (rt_rays.hip traces such rays).
int rt_camera_rays_device(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, RtRay *dev_rays) {
    static const std::string fn = "rt_camera_rays_device";
    int rc;
    if ((rc = refuse_null(fn, s, "scene")) || (rc = refuse_null(fn, rd, "render description")) || (rc = refuse_null(fn, dev_rays, "ray pointer")) ||
        (rc = refuse_unaligned16(fn, dev_rays, "dev_rays"))) return rc;
    if (count > (1u << 30)) return fail(RT_EINVAL, fn + ": count = " + std::to_string(count) + " is above 2^30");
    HIPCHK(hipSetDevice(s->device));
    DevFrame fr; if ((rc = camera_frame(rd, fr))) return rc;
    if (count == 0) return RT_OK;
    hipLaunchKernelGGL(camera_kernel, dim3((count + 255) / 256), dim3(256), 0, s->stream, s->dev, fr, (unsigned long long)first, count, dev_rays);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// Scene::Intersect / IntersectP for caller-supplied rays: the rays form one queue of the pipeline's trace kernel (counting
// twin with the quadric code), so the unit parity tests exercise the very kernel the large-scene renders spend their time in.
static int trace_common(RtScene *s, const RtRay *rays, uint32_t n, int any, RtHit *hits, uint8_t *occ) {
    if (!s || !rays || (!hits && !occ)) return fail(RT_EINVAL, "null argument");
    HIPCHK(hipSetDevice(s->device));
    if (n == 0) return RT_OK;
    if (int rc = ensure(s, s->trace_buf, size_t(n) * 3)) return rc;
    std::vector<float4> host(size_t(n) * 2);
    for (uint32_t i = 0; i < n; ++i) {
        host[i] = make_float4(rays[i].o[0], rays[i].o[1], rays[i].o[2], rays[i].mint);
        host[size_t(n) + i] = make_float4(rays[i].d[0], rays[i].d[1], rays[i].d[2], rays[i].maxt);
    }
    unsigned qc[RT_QC_STRIDE] = {0};
    qc[0] = any ? 0u : n; qc[RT_QC_ANY] = any ? n : 0u;
    HIPCHK(hipMemcpyAsync(s->trace_buf, host.data(), host.size() * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemcpyAsync(s->trace_qc, qc, sizeof qc, hipMemcpyHostToDevice, s->stream));
    TraceJob job{};
    job.q_o = s->trace_buf; job.q_d = s->trace_buf + n; job.q_slot = nullptr; job.q_count = s->trace_qc; job.hit = s->trace_buf + 2 * size_t(n);
    job.n_slots = 0; job.spill = s->spill; job.n_threads = s->n_threads; job.counters = s->counters;
    flavour::Request rq = plan::request(nullptr, s->facts, nullptr);
    rq.count = true;                                            // whatever rt_set_counting says
    const int k = flavour::Trace::index(rq);
    s->last = LastLaunch{};                                     // (the events are recorded anew)
    HIPWARN(hipEventRecord(s->ev0, s->stream));
    hipLaunchKernelGGL(g_pipe_trace[k], dim3(s->grids.trace[k]), dim3(RT_BLOCK), 0, s->stream, (const DevScene *)s->dev_scene, job);
    HIPWARN(hipEventRecord(s->ev1, s->stream)); HIPWARN(hipEventRecord(s->ev2, s->stream));
    HIPCHK(hipGetLastError());
    s->last.timed = true;                                       // one kernel between ev0 and ev1, nothing of a frame: every other field stays empty
    HIPCHK(hipMemcpyAsync(host.data(), s->trace_buf + 2 * size_t(n), size_t(n) * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (uint32_t i = 0; i < n; ++i) {
        int prim; std::memcpy(&prim, &host[i].x, 4);
        if (any) occ[i] = prim >= 0 ? 1 : 0;
        else { hits[i].prim = prim; hits[i].t = host[i].y; hits[i].b1 = host[i].z; hits[i].b2 = host[i].w; }
    }
    return RT_OK;
}
int rt_trace_closest(RtScene *s, const RtRay *rays, uint32_t n, RtHit *hits_out) { return trace_common(s, rays, n, 0, hits_out, nullptr); }
int rt_trace_any(RtScene *s, const RtRay *rays, uint32_t n, uint8_t *occluded_out) { return trace_common(s, rays, n, 1, nullptr, occluded_out); }
// Validate, bound the medium's marches, size the sample buffer, hand the frame to the launch function of the family plan_launch chose (render_pipeline,
// render_weighted, or render_mega for every single-launch family), then the film gather.  From the moment the frame is accepted the scene has no last
// launch (LastLaunch) until this one's events are all recorded: an error on the way leaves "no timed launch yet", never a mix of two frames.
int rt_render(RtScene *s, const RtRenderDesc *rd) {
    if (!s || !rd) return fail(RT_EINVAL, "null argument");
    HIPCHK(hipSetDevice(s->device));
    // ---- validation first: a failing call launches nothing and leaves the film and the sample buffer untouched
    const bool debug = rd->integrator == RT_INTEGRATOR_DEBUG;
    if ((rd->integrator < RT_INTEGRATOR_WHITTED || rd->integrator > RT_INTEGRATOR_BIDIRECTIONAL) && !debug) return fail(RT_EINVAL, "unknown integrator");
    const bool bidir = rd->integrator == RT_INTEGRATOR_BIDIRECTIONAL;
    if (rd->max_depth < 0 && !bidir && !debug) return fail(RT_EINVAL, "rt_render: negative maxdepth");
    if (debug) {                                              // DebugIntegrator (debug.cpp): strategy = red | green << 8 | blue << 16 (include/pbrt_hip.h)
        const unsigned codes = unsigned(rd->strategy);
        if ((codes >> 24) != 0u || (codes & 0xffu) > unsigned(RT_DEBUG_HIT) || ((codes >> 8) & 0xffu) > unsigned(RT_DEBUG_HIT) || ((codes >> 16) & 0xffu) > unsigned(RT_DEBUG_HIT))
            return fail(RT_EINVAL, "rt_render: unknown debug channel code (the debug integrator's strategy holds three RT_DEBUG_* codes, red | green << 8 | blue << 16)");
    }
    if (bidir) {                                              // BidirIntegrator (bidirectional.cpp): rt_bidir.h
        // the reference's connections ignore the medium's transmittance while EstimateDirect applies it: left for a later change
        if (s->volume.present) return fail(RT_EINVAL, "rt_render: the bidirectional integrator in a participating medium is not supported");
        if (s->dev.n_lights == 0) return fail(RT_EINVAL, "rt_render: the bidirectional integrator needs at least one light (the reference indexes lights[-1] in a scene with no lights)");
    }
    if (!rd->filter_table) return fail(RT_EINVAL, "rt_render: no filter table");
    const plan::FrameKnobs kn = frame_knobs();
    DevFrame fr; plan::Schedule sc; int rc = make_frame(s, rd, kn, fr, sc, true); if (rc) return rc;
    const bool weighted = rd->integrator == RT_INTEGRATOR_DIRECT && rd->strategy == RT_STRATEGY_WEIGHTED;
    if (rd->integrator == RT_INTEGRATOR_DIRECT && (rd->strategy < RT_STRATEGY_ALL || rd->strategy > RT_STRATEGY_WEIGHTED)) return fail(RT_EINVAL, "rt_render: unknown direct lighting strategy");
    if (weighted) {                                           // WeightedSampleOneLight: rt_weighted.h
        if (fr.shard_count != 1) return fail(RT_EINVAL, "rt_render: strategy \"weighted\" is a recurrence over the whole frame in the sampler's order (transport.cpp:71-122): one shard only");
        // (lights of mixed RNG use -- an emitter of several triangles draws its triangle, every other light draws nothing -- run the general form of the
        // survey and the recurrence: DevFrame::wt_mixed)
        // With a medium EstimateDirect draws one RandomFloat per UNOCCLUDED shadow / MIS ray (Scene::Transmittance), so the draws of an estimate depend on
        // the light AND on occlusion: the survey pass (every light, the counter left where the LAST light's estimate ends) and the frame pass (the chosen
        // light only) then reach the sample's next shading point with different counters, and a light that draws (ShapeSet::Sample's triangle pick) is fed
        // a different random number than the one its surveyed luminance came from.  Delta lights never draw: their Ld does not depend on it.
        if (s->volume.present && s->facts.light_draws != 0) return fail(RT_EINVAL, "rt_render: strategy \"weighted\" in a participating medium needs lights whose estimates draw no random numbers "
                                                                            "(point / spot / distant / single-triangle / quadric lights): an emitter of several triangles draws its triangle, and the medium makes "
                                                                            "the draw's position in the stream depend on occlusion");
        // An infinite light draws one RandomFloat() per estimate (infinite.cpp:104), whatever the light sample: the survey would have to keep one estimate of it
        // per position of that draw, as it does for emitters of several triangles (DevFrame::wt_mixed); that is not built.
        if (s->n_infinite != 0) return fail(RT_EINVAL, "rt_render: strategy \"weighted\" with an infinite light is not supported (the light draws a random number per estimate); "
                                                       "use strategy \"one\" or \"all\"");
        if (s->dev.n_lights > 2048u) return fail(RT_EINVAL, "rt_render: strategy \"weighted\" holds the per-light tables of its recurrence in LDS: at most 2048 lights");
        if (fr.total_work >= 0xffffffffull) return fail(RT_EINVAL, "rt_render: strategy \"weighted\": more than 2^32 - 2 camera samples in the frame");
    }
    const bool skip_film = kn.debug_nofilm.has_value();                // perf experiments only
    FilmGather fg; rc = film_gather_plan(s, fr, fg); if (rc) return rc;
    {   // the medium's march bounds (bind_scratch sizes the march samples from vol_nmax)
        plan::March m;
        if (plan::Refusal r = plan::plan_march(*rd, s->facts, m)) return fail(r.code, r.msg);
        fr.vol_nmax = m.vol_nmax; fr.dens_cap = m.dens_cap;
    }
    // ---- scratch
    {
        const size_t cap = s->samples.cap;
        const size_t local_pixels = size_t(fr.total_work / fr.spp);                     // sample_slot(): whole 64-pixel chunks
        const size_t need = ((local_pixels + 63) / 64 * 64 + 64) * size_t(fr.spp) * 2;
        rc = ensure(s, s->samples, need); if (rc) return rc;
        // A fresh buffer is zeroed once: the film gathers weigh the records of lanes without a column of their own (film_march_kernel: record 0)
        // and of dropped border items with +0, which is only a zero if the record is finite -- from here on sample_write keeps it so; a rank
        // that owns no tile at all writes nothing, ever.  For dropped items rt_samples_read returns zeros or what an earlier frame left there.
        if (cap != s->samples.cap) HIPCHK(hipMemsetAsync(s->samples, 0, s->samples.bytes(), s->stream));
    }
    fr.samples = s->samples; s->samples_last = fr.total_work; s->samples_spp = fr.spp;
    HIPCHK(hipMemcpyAsync(s->filter_dev, rd->filter_table, 256 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if (debug) { rc = upload_tex_uv(s); if (rc) return rc; }    // dg.u / dg.v of a mesh with "uv": on the device from the first debug frame on
    if ((rc = pending_error())) return rc;
    s->rendered = true;
    s->last = LastLaunch{};                                    // (the launch functions record the events anew)
    // ---- the frame, by the launch function of its family
    const plan::Launch ln = plan::plan_launch(*rd, s->facts, sc, false);
    LastLaunch ll;
    ll.fixed = ln.family == plan::Launch::Fixed || ln.family == plan::Launch::FixedScene; ll.fixed_scene = ln.scene_axes;
    if (ln.family == plan::Launch::Pipeline) rc = render_pipeline(s, rd, fr, sc, kn, ll);
    else if (ln.family == plan::Launch::Weighted) rc = render_weighted(s, rd, fr, ln, ll);
    else rc = render_mega(s, rd, fr, ln);
    if (rc) return rc;
    // ---- film gather and events
    if (!skip_film) { rc = film_gather_launch(s, fr, fg, (const DevFrame *)s->dev_frame, 0, fr.y_pixel_count); if (rc) return rc; }
    HIPCHK(hipEventRecord(s->ev2, s->stream));
    ll.timed = true; s->last = ll;
#ifdef RT_PROFILE
    {   // -DRT_PROFILE builds: per-wave cycle split of the render kernel
        unsigned long long v[24];
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipMemcpy(v, s->counters, sizeof v, hipMemcpyDeviceToHost));
        std::fprintf(stderr, "RT_PROFILE shade_cyc=%llu trav_cyc=%llu outer=%llu inner=%llu rounds=%llu act_lane_rounds=%llu rays_at_trav_start=%llu desc_cyc=%llu leaf_cyc=%llu chunks=%llu pooled_rounds=%llu leaf_iters=%llu\n",
                     v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15], v[16], v[17], v[18], v[19]);
#ifdef RT_PROFILE_STAGES
        {   // cycles (wave-level, summed over waves) and lane visits per stage of the state machine (rt_integrate.h advance_pass)
            unsigned long long st[32];
            HIPCHK(hipMemcpy(st, s->counters + 24, sizeof st, hipMemcpyDeviceToHost));
            static const char *names[16] = {"FETCH", "VERTEX", "DIRECT_NEXT", "SHADOW_DONE", "MIS_DONE", "ED_BSDF", "ED_DONE", "BOUNCE", "SPECULAR", "SPEC_TRANS", "RETURN", "VOL_BEGIN", "VOL_STEP", "POP", "FINISH", "EXIT"};
            for (int i = 0; i < 16; ++i) if (st[2 * i + 1])
                std::fprintf(stderr, "RT_PROFILE_STAGE %-12s cycles=%llu passes=%llu lane_visits=%llu\n", names[i], st[2 * i], st[2 * i + 1] >> 40, st[2 * i + 1] & ((1ull << 40) - 1));
            HIPCHK(hipMemsetAsync(s->counters + 24, 0, 32 * sizeof(unsigned long long), s->stream));
        }
#endif
        HIPCHK(hipMemsetAsync(s->counters + 8, 0, 16 * sizeof(unsigned long long), s->stream));
    }
#endif
    return RT_OK;
}
// Scene::Li for caller-supplied rays in device memory (include/pbrt_hip.h): the frame's plan with the n rays as its work (plan_query), bound like a
// frame, and one launch of the flavour::Rays entry -- the megakernel's radiance estimate with the caller's array as ray source and result sink.
// Nothing of the last rt_render is touched: no film, no sample buffer, no events, no LastLaunch; the descriptor is the query's own (query_frame).
int rt_radiance_device(RtScene *s, const RtRenderDesc *rd, const RtRay *dev_rays, uint64_t first, uint32_t n, float *dev_out) {
    static const std::string fn = "rt_radiance_device";
    int rc;
    if ((rc = refuse_null(fn, s, "scene")) || (rc = refuse_null(fn, rd, "render description"))) return rc;
    if (n > 0 && ((rc = refuse_null(fn, dev_rays, "ray pointer")) || (rc = refuse_null(fn, dev_out, "output pointer")) ||
                  (rc = refuse_unaligned16(fn, dev_rays, "dev_rays")) || (rc = refuse_unaligned16(fn, dev_out, "dev_out")))) return rc;
    HIPCHK(hipSetDevice(s->device));
    const plan::FrameKnobs kn = frame_knobs();
    const plan::QueryRange q{first, n};
    DevFrame fr; plan::Schedule sc;
    if ((rc = make_frame(s, rd, kn, fr, sc, false, &q))) return rc;
    {
        plan::March m;
        if (plan::Refusal r = plan::plan_march(*rd, s->facts, m)) return fail(r.code, r.msg);
        fr.vol_nmax = m.vol_nmax; fr.dens_cap = m.dens_cap;
    }
    if (n == 0) return RT_OK;
    fr.q_rays = reinterpret_cast<const float4 *>(dev_rays); fr.q_out = reinterpret_cast<float4 *>(dev_out); fr.q_first = unsigned(first);
    fr.samples = nullptr; fr.accum = nullptr; fr.filter_table = nullptr;          // (a query has no film)
    if ((rc = bind_scratch(s, rd, fr, s->n_threads))) return rc;
    PersistentKernel pk;
    if ((rc = resident_kernel(s, plan::plan_launch(*rd, s->facts, sc, true), pk)) || (rc = pending_error())) return rc;
    return launch_persistent(s, pk, fr, s->query_frame);
}
// Sample::imageX / imageY of camera samples first .. first + count - 1 into the caller's DEVICE buffer (include/pbrt_hip.h): the frame of
// rt_camera_rays_device, the sampler without the camera (rt_film_add.hip).
int rt_sample_positions_device(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, float *dev_xy) {
    static const std::string fn = "rt_sample_positions_device";
    int rc;
    if ((rc = refuse_null(fn, s, "scene")) || (rc = refuse_null(fn, rd, "render description")) || (count > 0 && (rc = refuse_null(fn, dev_xy, "output pointer")))) return rc;
    if (count > 0 && (reinterpret_cast<uintptr_t>(dev_xy) & 7u) != 0) return fail(RT_EINVAL, fn + ": dev_xy is not 8-byte aligned");
    HIPCHK(hipSetDevice(s->device));
    DevFrame fr; if ((rc = camera_frame(rd, fr))) return rc;
    if (fr.shard_count != 1) return fail(RT_EINVAL, fn + ": shard_count != 1 (the positions are addressed as the camera samples of the whole frame: one shard only)");
    const unsigned long long samples = fr.total_pixels * (unsigned long long)fr.spp;
    if (first > samples || count > samples - first) return fail(RT_EINVAL, fn + ": first + count is beyond the frame's camera samples");
    return sample_positions_launch(s, fr, first, count, dev_xy, nullptr);
}
// The volume integrator's two sampler values, the stream key and the counter of camera samples first .. first + count - 1 into the caller's DEVICE
// buffer (include/pbrt_hip.h): the frame of rt_sample_positions_device with the frame's sample requests bound (plan_requests; nothing is uploaded).
int rt_volume_samples_device(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, uint32_t *dev_out) {
    static const std::string fn = "rt_volume_samples_device";
    int rc;
    if ((rc = refuse_null(fn, s, "scene")) || (rc = refuse_null(fn, rd, "render description")) || (count > 0 && (rc = refuse_null(fn, dev_out, "output pointer")))) return rc;
    if (count > 0 && (rc = refuse_unaligned16(fn, dev_out, "dev_out"))) return rc;
    HIPCHK(hipSetDevice(s->device));
    DevFrame fr; if ((rc = camera_frame(rd, fr))) return rc;
    if (fr.shard_count != 1) return fail(RT_EINVAL, fn + ": shard_count != 1 (the samples are addressed as the camera samples of the whole frame: one shard only)");
    const unsigned long long samples = fr.total_pixels * (unsigned long long)fr.spp;
    if (first > samples || count > samples - first) return fail(RT_EINVAL, fn + ": first + count is beyond the frame's camera samples");
    plan::Requests rq;
    if (plan::Refusal r = plan::plan_requests(*rd, s->facts, fr.spp, rq)) return fail(r.code, r.msg);
    if (rq.n1d < 2) return fail(RT_EINVAL, fn + ": the frame plans no volume requests");
    fr.n1d = rq.n1d; fr.n2d = rq.n2d; fr.lhs_total = rq.lhs_total; fr.pixgen_draws = rq.pixgen_draws;
    std::memcpy(fr.one_d, rq.one_d, sizeof fr.one_d); std::memcpy(fr.two_d, rq.two_d, sizeof fr.two_d);
    if (count == 0) return RT_OK;
    return volume_samples_launch(s, fr, first, count, dev_out);
}
// Film::AddSample for radiances in device memory (include/pbrt_hip.h): binds what plan::plan_film_add plans -- the range's image positions into the
// call's own staging buffer (with the scene counting: the bad radiances counted on the way), then the gather over the film rows the range reaches.
// Nothing of the last rt_render but the film is touched: no sample buffer, no events, no LastLaunch.
int rt_film_add_device(RtScene *s, const RtRenderDesc *rd, const float *dev_L, uint64_t first, uint32_t n) {
    static const std::string fn = "rt_film_add_device";
    int rc;
    if ((rc = refuse_null(fn, s, "scene")) || (rc = refuse_null(fn, rd, "render description"))) return rc;
    if (n > 0 && ((rc = refuse_null(fn, dev_L, "radiance pointer")) || (rc = refuse_unaligned16(fn, dev_L, "dev_L")))) return rc;
    HIPCHK(hipSetDevice(s->device));
    plan::FilmAdd p;
    if (plan::Refusal r = plan::plan_film_add(*rd, plan::QueryRange{first, n}, s->accum ? s->film_w : 0, s->accum ? s->film_h : 0, p)) return fail(r.code, r.msg);
    if (n == 0) return RT_OK;
    bool packed; if ((rc = film_add_form(p, packed))) return rc;
    DevFrame fr; if ((rc = camera_frame(rd, fr))) return rc;
    if ((rc = ensure(s, s->add_xy, p.staging_floats)) || (rc = pending_error())) return rc;
    HIPCHK(hipMemcpyAsync(s->filter_dev, rd->filter_table, 256 * sizeof(float), hipMemcpyHostToDevice, s->stream));      // as rt_render uploads it
    if ((rc = sample_positions_launch(s, fr, first, n, s->add_xy, s->facts.counting ? dev_L : nullptr))) return rc;
    return film_add_launch(s, *rd, p, packed, first, n, dev_L, s->add_xy);
}
int rt_sync(RtScene *s) {
    if (!s) return fail(RT_EINVAL, "null scene");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    return RT_OK;
}

int rt_counters(RtScene *s, RtCounters *out) {
    if (!s || !out) return fail(RT_EINVAL, "null argument");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    unsigned long long v[8];
    HIPCHK(hipMemcpy(v, s->counters, sizeof v, hipMemcpyDeviceToHost));
    out->camera_rays = v[0]; out->closest_rays = v[1]; out->any_rays = v[2]; out->nodes_visited = v[3];
    out->leaf_refs = v[4]; out->tri_tests = v[5]; out->bad_samples = v[6]; out->stack_overflows = v[7];
    return RT_OK;
}
int rt_counters_reset(RtScene *s) {
    if (!s) return fail(RT_EINVAL, "null scene");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemsetAsync(s->counters, 0, 24 * sizeof(unsigned long long), s->stream));
    return RT_OK;
}
int rt_set_counting(RtScene *s, int enabled) {
    if (!s) return fail(RT_EINVAL, "null scene");
    s->facts.counting = enabled != 0;
    return RT_OK;
}
// Timing of the last timed launch by kernel, read from its events (rt_last_render_stats below keeps what this reads)
static int read_render_stats(RtScene *s, RtRenderStats *out) {
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipEventSynchronize(s->ev2));
    std::memset(out, 0, sizeof *out);
    HIPCHK(hipEventElapsedTime(&out->render_ms, s->ev0, s->ev1));
    HIPCHK(hipEventElapsedTime(&out->total_ms, s->ev0, s->ev2));
    out->gather_ms = out->total_ms - out->render_ms;
    const LastLaunch &l = s->last;
    out->pipeline = l.pipeline ? 1 : 0;
    if (l.pipeline) {
        out->iterations = l.iterations; out->timed_iterations = l.timed_iterations;
        float sum = 0.f;
        float sum2 = 0.f, sum3 = 0.f;
        for (int i = 0; i < l.timed_iterations; ++i) {
            float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, s->pipe_ev[6 * i], s->pipe_ev[6 * i + 1])); sum += ms;
            HIPCHK(hipEventElapsedTime(&ms, s->pipe_ev[6 * i + 2], s->pipe_ev[6 * i + 3])); sum2 += ms;
            if (l.marches) { HIPCHK(hipEventElapsedTime(&ms, s->pipe_ev[6 * i + 4], s->pipe_ev[6 * i + 5])); sum3 += ms; }
        }
        out->trace_ms = sum; out->shade_ms = sum2; out->march_ms = sum3;
        out->slots = l.slots;
    } else out->trace_ms = out->render_ms;
    out->bands = l.pipeline ? 0 : 1;
    out->fixed_frame = l.fixed ? 1 : 0;
    out->fixed_scene = l.fixed_scene;
    if (l.weighted) {
        out->weighted_points = l.weighted_points;
        hipEvent_t seq[6] = {s->ev0, s->wt_ev[0], s->wt_ev[1], s->wt_ev[2], s->wt_ev[3], s->ev1};
        for (int i = 0; i < 5; ++i) HIPCHK(hipEventElapsedTime(&out->weighted_ms[i], seq[i], seq[i + 1]));
    }
    return RT_OK;
}
// Timing of the last rt_render by kernel: {whole frame, render part (megakernel or shade+trace loop), trace kernel launches summed,
// film gather} in ms, the number of pipeline iterations (0: megakernel) and how many of them were timed.  The events are read once per timed launch:
// every later call returns the same bits (LastLaunch::stats), whatever was queued on the stream in between (rt_radiance_device records no event).
int rt_last_render_stats(RtScene *s, RtRenderStats *out) {
    if (!s || !out) return fail(RT_EINVAL, "null argument");
    if (!s->last.timed) return fail(RT_ESTATE, "no timed launch yet");
    if (!s->last.stats_read) {
        if (int rc = read_render_stats(s, &s->last.stats)) return rc;
        s->last.stats_read = true;
    }
    *out = s->last.stats;
    return RT_OK;
}
int rt_last_render_ms(RtScene *s, float *total_ms, float *kernel_ms) {
    if (!s || !s->last.timed) return fail(RT_ESTATE, "no timed launch yet");
    RtRenderStats st;
    if (int rc = rt_last_render_stats(s, &st)) return rc;
    if (total_ms) *total_ms = st.total_ms;        // render kernel(s) + film gather
    if (kernel_ms) *kernel_ms = st.render_ms;     // rt::render_kernel alone, or the whole shade / trace loop of the queue pipeline
    return RT_OK;
}

}  // extern "C"
