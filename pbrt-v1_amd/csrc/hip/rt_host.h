// rt_host.h -- what the host-side translation units of libpbrt_hip.so share: the scene object behind the opaque RtScene handle, error / knob helpers,
// the owners of its device memory, events and stream, the kernel tables with their resident grids (rt_flavour.h; persistent_kernel is the one place that
// turns a planned launch, rt_frame_plan.h plan::Launch, into a kernel and a grid), the record of the last timed launch (LastLaunch) and the refusals the device-pointer entry points share.  rt_scene.hip builds scenes (layouts, uploads, the accelerator ABI), rt_film.hip owns the film kernels and the rt_film_* ABI,
// rt_kernels.hip renders (make_frame binds what rt_frame_plan.h plans, launch_persistent launches what plan_launch chose, the queue pipeline, rt_render, rt_trace_*), rt_rays.hip traces caller-supplied rays in device
// memory (rt_trace_*_device, rt_hit_geometry_device), rt_bsdf.hip answers an integrator's questions of such hits (rt_bsdf_device), rt_film_add.hip adds caller-supplied radiances in device memory to the film (the kernels of rt_film_add_device /
// rt_sample_positions_device).  Round 6: split out of a 2 300-line rt_kernels.hip.
#pragma once
#include "rt_flavour.h"
#include "rt_render_kernel.h"
#include "rt_pipeline.h"
#include "rt_pipe_vertex.h"
#include "rt_pipe_march.h"
#include "rt_bidir.h"
#include "rt_internal.h"
#include "rt_devbuf.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <cmath>
#include <chrono>
#include <atomic>
#include <thread>
#include <type_traits>

namespace rt {
// Experiment / test knobs (PBRT_HIP_*: kernel flavour, pipeline form, film-gather kernel, layout switches, logs) are read only when
// PBRT_HIP_TUNE is set in the environment -- the tests and tools/ set it -- so a production process cannot change its behaviour through a stray
// variable; -DRT_NO_TUNABLES compiles them out.  (rt_kernels.hip)
const char *knob(const char *name);
// status code + message for rt_last_error() (thread-local; rt_kernels.hip)
int fail(int code, const std::string &msg);
const char *last_error();
void hip_warn(hipError_t e, const char *what);
}  // namespace rt
using namespace rt;
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return rt::fail(RT_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)
#define HIPWARN(expr) rt::hip_warn((expr), #expr)

// The kernel tables of the eight families, one per translation unit that instantiates kernels; rt_flavour.h has their sizes, the order of their
// entries and index(), the entry a frame takes.  The megakernel and the pipeline's shade kernel have a table per integrator (Whitted, DirectLighting, Path).
namespace rt {
extern const flavour::Table<RenderKernelFn, flavour::Mega> g_render_kernels_whitted, g_render_kernels_direct, g_render_kernels_path;
extern const flavour::Table<RenderKernelFn, flavour::Fixed> g_render_kernels_fixed;        // the fixed-frame twins of six Mega entries (rt_fixed_frame.h), all integrators in one table
extern const flavour::Table<RenderKernelFn, flavour::FixedScene> g_render_kernels_fixed_scene_direct, g_render_kernels_fixed_scene_path;   // their scene twins (rt_mega_fs{d,p}.hip)
extern const flavour::Table<RenderKernelFn, flavour::Rays> g_radiance_kernels_whitted, g_radiance_kernels_direct, g_radiance_kernels_path;   // rt_radiance_device (rt_mega_r{w,d,p}.hip)
extern const flavour::Table<RenderKernelFn, flavour::Weighted> g_render_kernels_weighted;
extern const flavour::Table<RenderKernelFn, flavour::Bidir> g_render_kernels_bidir;
extern const flavour::Table<RenderKernelFn, flavour::Debug> g_render_kernels_debug;
extern const flavour::Table<PipeShadeFn, flavour::Shade> g_pipe_shade_whitted, g_pipe_shade_direct, g_pipe_shade_path;
extern const flavour::Table<PipeShadeFn, flavour::Vertex> g_pipe_vertex;
extern const flavour::Table<PipeTraceFn, flavour::Trace> g_pipe_trace;
extern const flavour::Table<PipeMarchFn, flavour::March> g_pipe_march;
}  // namespace rt
// ... by RtRenderDesc::integrator
static const flavour::Table<RenderKernelFn, flavour::Mega> *const g_render_kernels[RT_INTEGRATOR_PATH + 1] = {&g_render_kernels_whitted, &g_render_kernels_direct, &g_render_kernels_path};
static const flavour::Table<RenderKernelFn, flavour::FixedScene> *const g_render_kernels_fixed_scene[RT_INTEGRATOR_PATH + 1] = {nullptr, &g_render_kernels_fixed_scene_direct, &g_render_kernels_fixed_scene_path};   // (flavour::FixedScene::has)
static const flavour::Table<RenderKernelFn, flavour::Rays> *const g_radiance_kernels[RT_INTEGRATOR_PATH + 1] = {&g_radiance_kernels_whitted, &g_radiance_kernels_direct, &g_radiance_kernels_path};
static const flavour::Table<PipeShadeFn, flavour::Shade> *const g_pipe_shade[RT_INTEGRATOR_PATH + 1] = {&g_pipe_shade_whitted, &g_pipe_shade_direct, &g_pipe_shade_path};
// The persistent families are launched with as many blocks as stay resident (scene_create): a grid per table entry
struct ResidentGrids {
    flavour::Table<unsigned, flavour::Mega> mega[RT_INTEGRATOR_PATH + 1];
    flavour::Table<unsigned, flavour::Fixed> fixed;
    flavour::Table<unsigned, flavour::FixedScene> fixed_scene[RT_INTEGRATOR_PATH + 1];
    flavour::Table<unsigned, flavour::Rays> rays[RT_INTEGRATOR_PATH + 1];
    flavour::Table<unsigned, flavour::Weighted> weighted;
    flavour::Table<unsigned, flavour::Bidir> bidir;
    flavour::Table<unsigned, flavour::Debug> debug;
    flavour::Table<unsigned, flavour::Trace> trace;
    flavour::Table<unsigned, flavour::March> march;
};
// The kernel and the grid of a planned launch (rt_frame_plan.h plan_launch): the one place that indexes the tables above for the persistent families.
// The queue pipeline is no one kernel: render_pipeline picks its entries
struct PersistentKernel { RenderKernelFn fn = nullptr; unsigned grid = 0; };
static inline PersistentKernel persistent_kernel(const ResidentGrids &g, const plan::Launch &l) {
    const int i = l.integ, k = l.k;
    switch (l.family) {
    case plan::Launch::Mega: return {(*g_render_kernels[i])[k], g.mega[i][k]};
    case plan::Launch::Fixed: return {g_render_kernels_fixed[k], g.fixed[k]};
    case plan::Launch::FixedScene: return {(*g_render_kernels_fixed_scene[i])[k], g.fixed_scene[i][k]};
    case plan::Launch::Debug: return {g_render_kernels_debug[k], g.debug[k]};
    case plan::Launch::Weighted: return {g_render_kernels_weighted[k], g.weighted[k]};
    case plan::Launch::Bidir: return {g_render_kernels_bidir[k], g.bidir[k]};
    case plan::Launch::Rays: return {(*g_radiance_kernels[i])[k], g.rays[i][k]};
    case plan::Launch::Pipeline: break;
    }
    return {};
}
// A device's resident grids: every entry gets as many blocks as its registers / LDS keep resident (x CUs; the trace kernel at most what
// PBRT_HIP_TRACE_BLOCKS_PER_CU says: occupancy experiments), then the rules that let every family share one scratch.  n_threads: the threads of the largest
// grid of all -- what the per-thread scratch and the spill area are sized by
static inline int size_resident_grids(int device, ResidentGrids &g, int &n_cus, unsigned &n_threads) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    n_cus = prop.multiProcessorCount;
    unsigned trace_per_cu = ~0u;
    if (const char *e = knob("PBRT_HIP_TRACE_BLOCKS_PER_CU")) trace_per_cu = unsigned(std::max(1, std::atoi(e)));
    auto resident = [&](const auto &kernels, auto &grids, unsigned at_most = ~0u) -> int {
        static_assert(sizeof kernels / sizeof kernels[0] == sizeof grids / sizeof grids[0], "a grid per table entry");
        for (size_t k = 0; k < kernels.size(); ++k) {
            int per_cu = 0;
            HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kernels[k], RT_BLOCK, 0));
            grids[k] = unsigned(prop.multiProcessorCount) * std::max(1u, std::min(unsigned(std::max(per_cu, 0)), at_most));
        }
        return RT_OK;
    };
    int rc;
    for (int i = 0; i <= RT_INTEGRATOR_PATH; ++i) {
        if ((rc = resident(*g_render_kernels[i], g.mega[i])) || (rc = resident(*g_radiance_kernels[i], g.rays[i]))) return rc;
        if (!flavour::FixedScene::has(i)) g.fixed_scene[i].fill(0u);
        else if ((rc = resident(*g_render_kernels_fixed_scene[i], g.fixed_scene[i]))) return rc;
    }
    if ((rc = resident(g_render_kernels_fixed, g.fixed)) || (rc = resident(g_render_kernels_weighted, g.weighted)) || (rc = resident(g_render_kernels_bidir, g.bidir)) ||
        (rc = resident(g_render_kernels_debug, g.debug)) || (rc = resident(g_pipe_trace, g.trace, trace_per_cu)) || (rc = resident(g_pipe_march, g.march))) return rc;
    auto largest = [](const auto &grids, unsigned of = 0) { for (unsigned n : grids) of = std::max(of, n); return of; };
    // a fixed-frame kernel never takes a larger grid than its generic twin's (it shares the twin's scratch), a scene twin never a larger one than its fixed-frame twin's
    for (int k = 0; k < flavour::Fixed::N; ++k) g.fixed[k] = std::min(g.fixed[k], g.mega[flavour::Fixed::integrator(k)][flavour::Fixed::generic(k)]);
    for (int i = 0; i <= RT_INTEGRATOR_PATH; ++i)
        for (int k = 0; flavour::FixedScene::has(i) && k < flavour::FixedScene::N; ++k) g.fixed_scene[i][k] = std::min(g.fixed_scene[i][k], g.fixed[flavour::FixedScene::fixed_twin(k, i)]);
    unsigned grid = largest(g.bidir, largest(g.weighted));                // the largest of the megakernel families
    for (const auto &mega : g.mega) grid = largest(mega, grid);
    // the debug and the radiance-query kernels (fewer registers than any of those; the code of Mega's EXT entries) never take a larger grid than the largest of the others
    for (unsigned &n : g.debug) n = std::min(n, grid);
    for (auto &rays : g.rays) for (unsigned &n : rays) n = std::min(n, grid);
    n_threads = largest(g.march, largest(g.trace, grid)) * RT_BLOCK;
    return RT_OK;
}

// ---- owners (rt_devbuf.h).  A device block is a DevBuf<T>; the same template with another release function owns page-locked memory, an event and the
// stream a scene created itself.  rt_kernels.hip defines the release functions, next to rt::dev_alloc / rt::dev_free.
namespace rt { void host_free(void *p); void event_free(void *e); void stream_free(void *st); }
template <class T> using Pinned = rt::DevBuf<T, rt::host_free>;
using Event = rt::DevBuf<std::remove_pointer_t<hipEvent_t>, rt::event_free>;
using OwnedStream = rt::DevBuf<std::remove_pointer_t<hipStream_t>, rt::stream_free>;

// The slot-indexed planes of the queue pipeline's pool (rt_pipeline.h PipePool is the kernels' view of them, filled once per frame).  each() is the
// ONE list of their elements per slot: the allocation sizes, the per-slot cost and what the pool holds (render_pipeline's memory budget) all walk it.
struct PipePlanes {
    DevBuf<float4> state, ray_o, hit, q_o; DevBuf<unsigned> q_slot;
    template <class F> void each(F &&f) { f(state, size_t(RT_PIPE_VEC)); f(ray_o, size_t(2)); f(hit, size_t(3)); f(q_o, size_t(4)); f(q_slot, size_t(3)); }   // hit: [kind][slot] in the by-vertex form
};

// The last timed launch (rt_render, rt_trace_closest / rt_trace_any): what rt_last_render_stats reports next to the events' times.  A launch builds one
// and assigns it to the scene whole once it is queued, so no field outlives its launch; a default one is "no timed launch yet".  The events are read once
// per launch and kept (stats): hipEventElapsedTime forms a time anew at every call and two reads of the same events differ in the last digits.
struct LastLaunch {
    bool timed = false;                                 // ev0 .. ev2 hold a launch
    bool pipeline = false, marches = false; int iterations = 0, timed_iterations = 0; unsigned slots = 0;     // the queue pipeline: iterations, those with events, slots
    bool weighted = false; unsigned long long weighted_points = 0;     // DirectLighting "weighted": the frame's shading points
    bool fixed = false; int fixed_scene = 0;            // a fixed-frame kernel (rt_fixed_frame.h); a scene twin of one: the axes it fixes (fixed::SCENE_*)
    bool stats_read = false; RtRenderStats stats{};
};

// Members are destroyed in reverse order of declaration: every buffer, then the events, then the stream (rt_scene_destroy has synchronised it).
struct RtScene {
    int device = 0;
    hipStream_t stream = nullptr;      // what every call uses: own_stream's, or the caller's (rt_scene_set_stream: not destroyed with the scene)
    OwnedStream own_stream;
    Event ev0, ev1, ev2;
    Event wt_ev[6];
    std::vector<Event> pipe_ev;                         // [6 * RT_PIPE_TIMED]: per iteration, around the trace, the shade and the march launch
    std::vector<Event> pipe_fence;
    KdTree tree;
    GridAccelData gridacc;
    plan::SceneFacts facts;             // what the frame planners read of the scene (rt_frame_plan.h): filled by scene_create and the setters that change a fact
    DevScene dev{};
    std::vector<DevBuf<char>> allocs;   // what was uploaded once and lives as long as the scene (scene_alloc)
    // film
    float *accum = nullptr; DevBuf<float> own_accum; int film_w = 0, film_h = 0;      // accum: own_accum's block, or the caller's (rt_film_bind)
    DevBuf<float> filter_dev;
    // per-launch scratch
    DevBuf<unsigned long long> work_counter, counters;
    DevBuf<uint2> spill;
    DevBuf<float> frames;
    unsigned n_threads = 0;
    ResidentGrids grids{};             // size_resident_grids; n_threads: the threads of the largest grid
    DevBuf<DimReq> light_dims;         // DirectLighting "all": the per-light sample requests (plan_requests, rt_frame_plan.h; make_frame uploads them); the bidirectional integrator: its BidirTable
    std::vector<DimReq> light_dims_host;
    const unsigned *light_draw_flags = nullptr; unsigned n_drawing_lights = 0;
    DevBuf<unsigned> wt_recbase;
    unsigned n_infinite = 0;           // RT_LIGHT_INFINITE lights (each estimate draws one RandomFloat(), infinite.cpp:104: refused with strategy "weighted")
    DevBuf<unsigned> wt_base; DevBuf<float> wt_rec; DevBuf<float2> wt_pick;
    DevBuf<unsigned long long> wt_sums;                        // per-block sums of the point-count scan
    Pinned<unsigned long long> wt_total;                       // page-locked: the frame's shading points (weighted_scan_top_kernel)
    DevBuf<DevScene> dev_scene; DevBuf<DevFrame> dev_frame;     // descriptors in HBM (read with scalar loads)
    DevBuf<float4> samples;                                    // per-shard sample buffer
    int samples_spp = 1;
    unsigned long long samples_last = 0;                       // camera samples the LAST rt_render wrote (rt_samples_read's range)
    DevBuf<float> resolve_buf;
    DevBuf<float> vol_buf;                                 // volume scratch: rays | state | samp
    RtVolume volume{};
    bool rendered = false;                                 // an rt_render has been accepted
    // textured materials (rt_scene_set_textures): the scene's own resolved records (host copy) and the device array that holds them followed by
    // the records for the materials resolved per hit (rt_texture.h); dev.materials points at it once the scene has textures
    std::vector<DevMaterial> materials_host;
    std::vector<DevLight> lights_host;
    std::vector<int> tex_uv_idx_host; std::vector<float> tex_uv_host;   // uvs of the triangles whose mesh has "uv" ([n_tris] index or -1, 6 floats each): host only until upload_tex_uv
    bool has_textures = false;
    DevBuf<DevMaterial> mat_buf;
    int spill_depth = 0;
    LastLaunch last;
    uint32_t n_tris = 0;
    // queue pipeline (rt_pipeline.h)
    PipePlanes pool; DevBuf<unsigned> q_count; DevBuf<unsigned long long> wave_work; DevBuf<PipePool> dev_pool;
    Pinned<unsigned> h_qcount;                          // page-locked mirror of q_count (termination test)
    DevBuf<float4> trace_buf;                            // rt_trace_*: rays (2 x float4) and hits, reused across calls
    int n_cus = 0;
    DevBuf<unsigned> trace_qc;
    // rt_trace_*_device (rt_rays.hip): the two ray planes the trace kernel reads, and the hit plane of an any-hit call (a closest-hit call
    // writes the caller's RtHit array); each grows only when a call brings more rays than any before it
    DevBuf<float4> ray_planes, any_hits;
    // rt_radiance_device (rt_kernels.hip): the query's own descriptor, so that the last frame's stays what rt_render left.  Everything else a query needs
    // is the scratch frames use (frames, vol_buf, the material pool: per resident thread, grown only when a query recurses deeper than anything before
    // it); nothing is sized by the number of rays
    DevBuf<DevFrame> query_frame;
    // rt_film_add_device (rt_kernels.hip): the image positions of the call's samples, two floats each -- the call's own staging, sized by the largest
    // range added so far; the sample buffer above stays the last frame's
    DevBuf<float> add_xy;
    // rt_bsdf_device (rt_bsdf.hip): the descriptor resolve_hit_material reads -- where the resolved-material records lie (mat_pool_base as of
    // bsdf_pool_base) and how many lanes own one; the records themselves are level 0 of the frames' pool, one per resident thread
    DevBuf<DevFrame> bsdf_frame; unsigned bsdf_pool_base = 0;
};
#define RT_PIPE_QN 4096          // ring of per-iteration queue counters
#define RT_PIPE_TIMED 256        // iterations whose trace launch is bracketed by events
#define RT_PIPE_BATCH 4          // iterations launched between two termination checks

// a device block that lives as long as the scene
static inline int scene_alloc(RtScene *s, size_t bytes, void **p) {
    DevBuf<char> b;
    if (int rc = b.grow(bytes)) return rc;
    *p = b.p; s->allocs.push_back(std::move(b));
    return RT_OK;
}
template <class T>
static inline int upload(RtScene *s, const T *host, size_t n, const T **dev) {
    void *p = nullptr;
    if (int rc = scene_alloc(s, (n ? n : 1) * sizeof(T), &p)) return rc;
    if (n) HIPCHK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<const T *>(p);
    return RT_OK;
}

// the uvs of the meshes that have them, to the device (hit_point_uv reads them): once, for a scene that gets textures or renders a debug frame; rt_scene.hip
int upload_tex_uv(RtScene *s);
// scenes with textures: room for `levels` resolved materials per thread / slot behind the scene's own (fr.mat_pool_base); rt_scene.hip
int ensure_material_pool(RtScene *s, rt::DevFrame &fr, size_t levels, size_t n_slots);

// (re)allocate a scratch buffer that work queued on the scene's stream may still be using: wait for the stream before the old block goes
template <class T>
static inline int ensure(RtScene *s, DevBuf<T> &b, size_t need) {
    if (need <= b.cap) return RT_OK;
    if (b.p) HIPCHK(hipStreamSynchronize(s->stream));
    return b.grow(need);
}

// No C++ exception crosses the C boundary: the host builders allocate gigabytes and start worker threads (every group of them is joined while the
// exception unwinds, rt_internal.h ThreadGroup), so bad_alloc / a failed thread start end in a status code, not in std::terminate.
template <class F> static inline int guarded(const char *what, F &&f) {
    try { return f(); }
    catch (const std::bad_alloc &) { return rt::fail(RT_ENOMEM, std::string(what) + ": out of host memory"); }
    catch (const std::exception &e) { return rt::fail(RT_ESTATE, std::string(what) + ": " + e.what()); }
}

// ---- the refusals the entry points that take device pointers share (rt_kernels.hip, rt_rays.hip), before anything is launched.  `what` names a pointer in
// the "null" text ("ray pointer"), `name` in the alignment text ("dev_rays")
static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int refuse_null(const std::string &fn, const void *p, const char *what) { return p ? RT_OK : fail(RT_EINVAL, fn + ": null " + what); }
static inline int refuse_unaligned16(const std::string &fn, const void *p, const char *name) {
    return aligned16(p) ? RT_OK : fail(RT_EINVAL, fn + ": " + name + " is not 16-byte aligned");
}
// an error some earlier asynchronous work left behind must not be taken for this launch's
static inline int pending_error() {
    const hipError_t pre = hipGetLastError();
    return pre == hipSuccess ? RT_OK : fail(RT_EDEVICE, std::string("pending HIP error before launch: ") + hipGetErrorString(pre));
}

// ---- the film gather (rt_film.hip): which of the three kernels a frame takes, and its launch over film rows [row0, row_end) on the scene's stream
struct FilmGather { int which = 0, grx = 0, gry = 0, cols = 0, rows = 0, slot_ncs = 0; size_t slot_lds = 0, col_bytes = 0; };
int film_gather_plan(RtScene *s, const rt::DevFrame &fr, FilmGather &g);
int film_gather_launch(RtScene *s, const rt::DevFrame &fr, const FilmGather &g, const rt::DevFrame *dfr, int row0, int row_end);

// ---- a film add (rt_film_add.hip): the image positions of camera samples [first, first + count) of the frame bound to `fr` (with dev_L: its bad
// radiances counted), and ImageFilm::AddSample for such a range over the film rows plan::plan_film_add found, both on the scene's stream
int sample_positions_launch(RtScene *s, const rt::DevFrame &fr, unsigned long long first, unsigned count, float *dev_xy, const float *dev_L);
// ---- rt_volume_samples_device (rt_medium.hip): per camera sample of [first, first + count) the frame's tau and scatter values, the stream's key and its counter
int volume_samples_launch(RtScene *s, const rt::DevFrame &fr, unsigned long long first, unsigned count, uint32_t *dev_out);
int film_add_form(const rt::plan::FilmAdd &p, bool &packed);       // which of the gather's two forms (PBRT_HIP_FILM_ADD forces one), before any launch
int film_add_launch(RtScene *s, const RtRenderDesc &rd, const rt::plan::FilmAdd &p, bool packed, unsigned long long first, unsigned n, const float *dev_L, const float *dev_xy);
