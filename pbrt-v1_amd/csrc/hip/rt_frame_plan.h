// rt_frame_plan.h -- what the host decides for a frame before anything touches the device: the work extent (plan_extent), the sample-request tables
// that are the keyed RNG's address map (plan_requests), the scheduling policy with its knobs (plan_schedule) and the bounds of the medium's marches
// (plan_march); what turns a frame's schedule into that of a radiance query over caller-supplied rays (plan_query); what a range of caller-supplied radiances needs of the film (plan_film_add); and which kernel of which family the frame or query launches (plan_launch).  Plain functions over plain structs: a render description, the SceneFacts an RtScene keeps of itself, the knobs as values.  No
// allocation beyond std::vector, no I/O, no getenv; a refusal comes back as a code and a message.  make_frame (rt_kernels.hip) binds the results
// to a DevFrame.  No HIP header: tests/frame_plan_host_test.cpp checks the rules with a host compiler.
#pragma once
#include "rt_fastdiv.h"
#include "rt_flavour.h"
#include "rt_fixed_frame.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <optional>
#include <vector>

// The -D knobs of rt_traverse.h and rt_render_kernel.h that the policy reads, with their defaults for a unit that includes neither
#ifndef RT_TRACE_LEAF_MIN
#define RT_TRACE_LEAF_MIN 24
#endif
#ifndef RT_MEGA_BYV
#define RT_MEGA_BYV 1
#endif

namespace rt {

#define RT_MAX_DIM_REQ 12         // requests the frame descriptor itself carries (PathIntegrator: 11 one-dimensional, 9 two-dimensional); DirectLighting "all"
                                  // has three per light, without bound (directlighting.cpp:39-66): DevFrame::light_dims
struct DimReq { unsigned f_base, u_base; unsigned short n; unsigned short dims; };

#define RT_BD_MAX_VERTS 4
// RequestSamples (bidirectional.cpp:65-79) in HBM, where DirectLighting "all" keeps its per-light requests (DevFrame::light_dims, idle for this integrator):
// for vertex i the 1-D requests eyeBSDFComp, lightBSDFComp, directLightNum, directBSDFComp at one_d[4 i ..] and the 2-D requests eyeBSDF, lightBSDF,
// directLight, directBSDF at two_d[4 i ..], then lightNum (one_d[16]), lightPos and lightDir (two_d[16], [17]); and the world's bounding sphere
struct BidirTable { DimReq one_d[4 * RT_BD_MAX_VERTS + 1], two_d[4 * RT_BD_MAX_VERTS + 2]; float wc[3], wr; };

namespace plan {

// RT_OK, or why the frame is refused (the text of rt_last_error())
struct Refusal {
    int code = RT_OK; const char *msg = "";
    explicit operator bool() const { return code != RT_OK; }
};
inline Refusal refuse(int code, const char *msg) { return Refusal{code, msg}; }

// What the planners need to know of a scene.  RtScene fills it at create and in the setters that change a fact (rt_scene.hip, rt_set_counting)
struct SceneFacts {
    int accel_kind = RT_ACCEL_KDTREE;
    size_t n_nodes = 0;                  // kd-tree nodes / grid voxels
    double per_leaf = 1.0;               // average primitives per non-empty kd leaf (1 for a grid or a tree without one)
    bool has_ext = false;                // plastic materials or quadrics present: use the kernels that carry that code (EXT)
    bool counting = true;                // rt_set_counting
    bool medium = false;                 // RtVolume::present
    unsigned n_lights = 0;
    bool specular_materials = false;     // some material is not matte (mirror, glass; the EXT materials set has_ext): fixed::SceneFacts::specular
    bool scene_twins = true;             // the scene's frames may take a kernel compiled for its light and materials; scene_create clears it for PBRT_HIP_FIXED_SCENE=0
    std::vector<int> light_samples;     // [n_lights] DevLight::n_samples, as uploaded (>= 1)
    int light_draws = 0;                 // RandomFloat()s one EstimateDirect draws: the same for every light (0 / 1), or -1 when the lights differ
    float lens_radius = 0.f; int camera_type = RT_CAMERA_PERSPECTIVE;
    float bounds[6] = {0, 0, 0, 0, 0, 0};            // the accelerator's bound (min, max)
    float vol_p0[3] = {0, 0, 0}, vol_p1[3] = {0, 0, 0};   // the medium's extent in its own space (RtVolume::p0, p1)
    double vol_world[6] = {0, 0, 0, 0, 0, 0};        // density region: the volume's world bound (WorldToVolume^-1 of its extent)
    double cam_pos[3] = {0, 0, 0};                   // CameraToWorld(0,0,0)
    int density_kind = RT_DENSITY_NONE;              // rt_scene_set_density
};

// The PBRT_HIP_* knobs of the render path as values: unset, or the integer the variable held (frame_knobs() in rt_kernels.hip reads them)
struct FrameKnobs {
    std::optional<int> high_occ, leaf_min, trav_mode, xcd_bands, exit_thresh, phase_sync, pipeline, mega_tile, fixed_frame, pipe_vertex, pipe_mem_mb,
        pipe_slots, debug_nofilm;
    int dbg_x = -1000000, dbg_y = -1000000;          // PBRT_HIP_DEBUG_PIXEL "x,y" (-DRT_DEBUG_PIXEL builds)
};

inline unsigned round_up_pow2(unsigned v) { v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v + 1; }   // pbrt.h:590-598

// ---------------------------------------------------------------------------------------------- 1. the work extent
// samples per pixel, the sample extent's pixels, the caller's tiles and this shard's share of them (the DevFrame fields of the same names)
struct Extent {
    int spp = 0;
    int shard_index = 0, shard_count = 1, tile_pixels = 1;
    int tile_w = 0, tile_h = 0, tiles_x = 0;
    unsigned long long total_pixels = 0, total_work = 0;
};
// ... as the caller describes it: plan_schedule resets it for a one-shard megakernel frame
inline Refusal plan_extent(const RtRenderDesc &rd, Extent &e) {
    if (rd.sampler < RT_SAMPLER_STRATIFIED || rd.sampler > RT_SAMPLER_RANDOM) return refuse(RT_EINVAL, "unknown sampler");
    if (rd.sampler == RT_SAMPLER_LOWDISCREPANCY) { if (rd.pixel_samples < 1) return refuse(RT_EINVAL, "bad pixelsamples"); }
    else if (rd.x_samples < 1 || rd.y_samples < 1) return refuse(RT_EINVAL, "bad xsamples/ysamples");
    e = Extent{};
    e.spp = rd.sampler == RT_SAMPLER_LOWDISCREPANCY ? int(round_up_pow2(unsigned(rd.pixel_samples))) : rd.x_samples * rd.y_samples;
    if (rd.x_end <= rd.x_start || rd.y_end <= rd.y_start) return refuse(RT_EINVAL, "empty sample extent");
    e.shard_index = rd.shard_index; e.shard_count = rd.shard_count < 1 ? 1 : rd.shard_count;
    e.tile_pixels = rd.tile_pixels < 1 ? 1 : rd.tile_pixels;
    if (e.shard_index < 0 || e.shard_index >= e.shard_count) return refuse(RT_EINVAL, "bad shard index");
    e.total_pixels = (unsigned long long)(rd.x_end - rd.x_start) * (unsigned long long)(rd.y_end - rd.y_start);
    if (e.total_pixels * e.spp > 0xFFFFFFFFull) return refuse(RT_EINVAL, "more than 2^32 camera samples per frame");
    unsigned long long n_tiles = 0;
    if (rd.tile_pixels < 0) {                               // 2-D tiles: width in the low 16 bits of -tile_pixels, height above (pbrt_hip.h)
        const int tw = (-rd.tile_pixels) & 0xffff, th = (-rd.tile_pixels) >> 16;
        if (tw < 1 || th < 1 || tw > 4096 || th > 4096) return refuse(RT_EINVAL, "bad 2-D tile size");
        e.tile_w = tw; e.tile_h = th; e.tile_pixels = tw * th;
        e.tiles_x = (rd.x_end - rd.x_start + tw - 1) / tw;
        n_tiles = (unsigned long long)e.tiles_x * (unsigned long long)((rd.y_end - rd.y_start + th - 1) / th);
        if (n_tiles * e.tile_pixels * e.spp > 0xFFFFFFFFull) return refuse(RT_EINVAL, "more than 2^32 camera samples per frame (2-D tiles, border tiles included)");
    } else n_tiles = (e.total_pixels + e.tile_pixels - 1) / e.tile_pixels;
    const unsigned long long my_tiles = n_tiles > (unsigned long long)e.shard_index
        ? (n_tiles - e.shard_index + e.shard_count - 1) / e.shard_count : 0;
    e.total_work = my_tiles * e.tile_pixels * e.spp;
    return Refusal{};
}

// ---------------------------------------------------------------------------------------------- 2. the sample-request tables
// The Sample layout the integrators request (Sample::Sample sampling.cpp:41-70; RequestSamples of directlighting.cpp:39-66, path.cpp:47-57,
// emission.cpp:42-46 / single.cpp:43-47; LatinHypercube draw counts sampling.cpp:98-113): what the descriptor carries, and the table in HBM
struct Requests {
    int n1d = 0, n2d = 0;
    DimReq one_d[RT_MAX_DIM_REQ] = {}, two_d[RT_MAX_DIM_REQ] = {};
    unsigned lhs_total = 0;              // draws consumed by LatinHypercube per sample
    unsigned pixgen_draws = 0;           // draws consumed when a new pixel's strata are generated
    int dims_max_n = 0;                  // the largest sample count of a 2-D request
    std::vector<DimReq> table;           // DevFrame::light_dims: DirectLighting "all": three records per light (+ one); bidirectional: a BidirTable; else empty
};
inline Refusal plan_requests(const RtRenderDesc &rd, const SceneFacts &sf, int spp, Requests &rq) {
    rq = Requests{};
    std::vector<int> n1, n2;
    const int nl = int(sf.n_lights);
    if (rd.integrator == RT_INTEGRATOR_DIRECT && rd.strategy == RT_STRATEGY_ALL) {
        for (int i = 0; i < nl; ++i) { int ns = sf.light_samples[size_t(i)]; if (rd.sampler == RT_SAMPLER_LOWDISCREPANCY) ns = int(round_up_pow2(unsigned(ns)));   // Sampler::RoundSize
            if (ns > 65535) return refuse(RT_EINVAL, "rt_render: more than 65535 samples per light (the sample table holds counts in 16 bits)");
            n2.push_back(ns); n2.push_back(ns); n1.push_back(ns); }
    } else if (rd.integrator == RT_INTEGRATOR_DIRECT) { n2 = {1, 1}; n1 = {1, 1}; }
    else if (rd.integrator == RT_INTEGRATOR_PATH) { n1.assign(9, 1); n2.assign(9, 1); }
    else if (rd.integrator == RT_INTEGRATOR_BIDIRECTIONAL) { n1.assign(4 * RT_BD_MAX_VERTS + 1, 1); n2.assign(4 * RT_BD_MAX_VERTS + 2, 1); }     // bidirectional.cpp:65-79
    else if (rd.integrator != RT_INTEGRATOR_WHITTED && rd.integrator != RT_INTEGRATOR_DEBUG) return refuse(RT_EINVAL, "unknown integrator");     // (neither requests samples)
    n1.push_back(1); n1.push_back(1);                   // the volume integrator's tau / scatter samples
    // The requests in the reference's order (every 1-D request, then every 2-D one: Sample::Sample sampling.cpp:41-70).  DirectLighting "all" asks for
    // 2 x 2-D and 1 x 1-D per light WITHOUT bound (directlighting.cpp:39-66): its per-light requests go to a table in HBM (DevFrame::light_dims, three
    // records per light, indexed by the lane's light cursor); the frame descriptor itself carries the bounded rest.
    const bool all_lights = rd.integrator == RT_INTEGRATOR_DIRECT && rd.strategy == RT_STRATEGY_ALL;
    std::vector<DimReq> d1(n1.size()), d2(n2.size());
    unsigned c = 0;
    const unsigned P = unsigned(spp);
    if (rd.sampler == RT_SAMPLER_STRATIFIED) {              // LatinHypercube: n*d floats then n*d shuffles per request
        for (size_t i = 0; i < n1.size(); ++i) { d1[i] = DimReq{c, c + unsigned(n1[i]), (unsigned short)n1[i], 1}; c += 2u * n1[i]; }
        for (size_t i = 0; i < n2.size(); ++i) { d2[i] = DimReq{c, c + 2u * n2[i], (unsigned short)n2[i], 2}; c += 4u * n2[i]; }
        rq.lhs_total = c;
        rq.pixgen_draws = rd.jitter ? 7u * P : 2u * P;      // stratified.cpp:99-117
    } else if (rd.sampler == RT_SAMPLER_RANDOM) {           // one float per value (random.cpp:107-112)
        for (size_t i = 0; i < n1.size(); ++i) { d1[i] = DimReq{c, 0, (unsigned short)n1[i], 1}; c += unsigned(n1[i]); }
        for (size_t i = 0; i < n2.size(); ++i) { d2[i] = DimReq{c, 0, (unsigned short)n2[i], 2}; c += 2u * n2[i]; }
        rq.lhs_total = c;
        rq.pixgen_draws = 5u * P;                           // random.cpp:88-92
    } else {                                                // per-pixel tables (lowdiscrepancy.cpp:93-104, sampling.h:152-174)
        c = (2 + 2 * P) + (2 + 2 * P) + (1 + 2 * P);        // image, lens, time blocks
        for (size_t i = 0; i < n1.size(); ++i) { d1[i] = DimReq{c, 0, (unsigned short)n1[i], 1}; c += 1u + unsigned(n1[i]) * P + P; }
        for (size_t i = 0; i < n2.size(); ++i) { d2[i] = DimReq{c, 0, (unsigned short)n2[i], 2}; c += 2u + unsigned(n2[i]) * P + P; }
        rq.lhs_total = 0;
        rq.pixgen_draws = c;
    }
    {   // the draws of one camera sample are addressed by a 32-bit counter: the tables above must fit well inside it
        unsigned long long draws = 0;
        for (int n : n1) draws += 2ull * unsigned(n) * (P + 1);
        for (int n : n2) draws += 4ull * unsigned(n) * (P + 1);
        if (draws > 0x3fffffffull) return refuse(RT_EINVAL, "rt_render: the lights' sample requests need more than 2^30 random numbers per camera sample");
    }
    for (const DimReq &r : d2) rq.dims_max_n = std::max(rq.dims_max_n, int(r.n));
    const bool bidir = rd.integrator == RT_INTEGRATOR_BIDIRECTIONAL;
    if (all_lights) {
        rq.table.assign(size_t(nl) * 3 + 1, DimReq{0, 0, 0, 0});
        for (int i = 0; i < nl; ++i) { rq.table[3 * size_t(i)] = d2[2 * size_t(i)]; rq.table[3 * size_t(i) + 1] = d2[2 * size_t(i) + 1]; rq.table[3 * size_t(i) + 2] = d1[size_t(i)]; }
    } else if (bidir) {
        // the bidirectional integrator: its 17 + 18 requests (more than the descriptor's arrays hold) and the world's bounding sphere, one BidirTable
        BidirTable bt; std::memset(&bt, 0, sizeof bt);
        for (int i = 0; i < 4 * RT_BD_MAX_VERTS + 1; ++i) bt.one_d[i] = d1[size_t(i)];
        for (int i = 0; i < 4 * RT_BD_MAX_VERTS + 2; ++i) bt.two_d[i] = d2[size_t(i)];
        // Scene::WorldBound() (scene.cpp:114-119; a medium is refused, so it is the accelerator's bound) -> BBox::BoundingSphere (geometry.cpp:47-50)
        const float *b = sf.bounds;
        const float cx = .5f * b[0] + .5f * b[3], cy = .5f * b[1] + .5f * b[4], cz = .5f * b[2] + .5f * b[5];
        const bool inside = cx >= b[0] && cx <= b[3] && cy >= b[1] && cy <= b[4] && cz >= b[2] && cz <= b[5];
        const float dx = cx - b[3], dy = cy - b[4], dz = cz - b[5];
        bt.wc[0] = cx; bt.wc[1] = cy; bt.wc[2] = cz; bt.wr = inside ? std::sqrt(dx * dx + dy * dy + dz * dz) : 0.f;
        rq.table.assign((sizeof bt + sizeof(DimReq) - 1) / sizeof(DimReq), DimReq{0, 0, 0, 0});
        std::memcpy(rq.table.data(), &bt, sizeof bt);
    }
    if (all_lights || bidir) {
        d1.erase(d1.begin(), d1.begin() + (all_lights ? nl : 4 * RT_BD_MAX_VERTS + 1));     // what stays in the descriptor: the volume integrator's two 1-D requests
        d2.clear();
    }
    if (d1.size() > RT_MAX_DIM_REQ || d2.size() > RT_MAX_DIM_REQ) return refuse(RT_ESTATE, "rt_render: sample table overflow");      // (cannot happen: 11 / 9 for the path integrator)
    rq.n1d = int(d1.size()); rq.n2d = int(d2.size());
    for (size_t i = 0; i < d1.size(); ++i) rq.one_d[i] = d1[i];
    for (size_t i = 0; i < d2.size(); ++i) rq.two_d[i] = d2[i];
    return Refusal{};
}

// ---------------------------------------------------------------------------------------------- 3. the scheduling policy
// Performance only: results and counters do not depend on it.  Every default, then its knob; the rules that hold whatever the knobs say run after
// all of them, and trav_mode is fixed up last.
struct Schedule {
    int trav_mode = 2, exit_thresh = 0, high_occupancy = 0, leaf_min = 0, xcd_bands = 0, phase_sync = 0, pipeline = 0, mega_tile = 0;   // the DevFrame fields
    int dbg_x = -1000000, dbg_y = -1000000;
    Extent extent;                       // the caller's, or reset to scanline order for a one-shard megakernel frame
    bool fixed_frame = false;            // plan_launch takes the twin compiled for a fixed frame (rt_fixed_frame.h)
    int fixed_scene = 0;                 // ... and, non-zero, that kernel's twin compiled for the scene too: the axes it fixes (fixed::SCENE_*)
    bool by_vertex = false;              // render_pipeline shades once per path vertex (rt_pipe_vertex.h)
};
inline Schedule plan_schedule(const RtRenderDesc &rd, const SceneFacts &sf, const Extent &ext, const Requests &rq, const FrameKnobs &kn) {
    Schedule sc;
    sc.extent = ext;
    const bool tiny = sf.n_nodes <= 4096 && sf.per_leaf >= 1.5;       // few fat leaves: triangle tests dominate -> lock-step rounds
    const bool tiny_path = tiny && rd.integrator == RT_INTEGRATOR_PATH;
    sc.trav_mode = (tiny && !tiny_path) ? 3 : 2;           // tiny trees, Whitted / DirectLighting: lock-step rounds with pooled leaf tests; else batched
                                                           // rounds (measured best on 100k-1M triangle soups and, since the spill-free round-3 build,
                                                           // for the path integrator on tiny trees too: profiles/r03_c2_knobs.txt)
    // long divergent rays: let finished lanes refill early.  Tiny scenes: only with phase gating (path integrator), where 8
    // measured +1.5 % (16: -13 %); Whitted / DirectLighting on Cornell lose 10 % with any early exit
    sc.exit_thresh = tiny ? (rd.integrator == RT_INTEGRATOR_PATH ? 8 : 0) : 32;
    // round 5, the path integrator by vertex (a lane comes back for shading once per vertex, not once per ray): 16 on tiny trees (C2's kernel 49.8 -> 48.5 ms;
    // 24: 48.7, 32: 50.1), 32-40 alike on the 1 M-triangle frames (profiles/r05_by_vertex_scan.txt)
    if (RT_MEGA_BYV && tiny && rd.integrator == RT_INTEGRATOR_PATH && !sf.medium && !sf.has_ext) sc.exit_thresh = 16;
    sc.high_occupancy = (tiny && !tiny_path) ? 0 : 1;      // C2 (round 3): 4-wave flavour + batched rounds + exit threshold 8 = 54.0 ms, natural allocation + pooled lock-step 56.5
    if (kn.high_occ) sc.high_occupancy = *kn.high_occ;
    sc.leaf_min = tiny ? 8 : RT_TRACE_LEAF_MIN;          // C2: 50.8 ms at 8, 54.0 at 24 (few fat leaves: waiting for a fuller batch only idles lanes)
    if (kn.leaf_min) sc.leaf_min = std::max(1, *kn.leaf_min);
    if (kn.trav_mode) sc.trav_mode = *kn.trav_mode;
    // XCD bands of the work list (rt_render_kernel.h): frames whose rays stay coherent (Whitted / DirectLighting: camera, shadow and specular rays)
    // gain from each private L2 holding one band's lines -- C3 13.37 -> 12.62 ms; path frames, whose rays scatter after the first bounce, lose
    // 5 % (1 M path 62.2 -> 65.5 ms, C4 64.1 -> 67.5; profiles/r04_xcd_bands_scan.txt)
    sc.xcd_bands = rd.integrator != RT_INTEGRATOR_PATH ? 1 : 0;
    if (kn.xcd_bands) sc.xcd_bands = *kn.xcd_bands != 0;
    if (kn.exit_thresh) sc.exit_thresh = *kn.exit_thresh;
    sc.dbg_x = kn.dbg_x; sc.dbg_y = kn.dbg_y;
    sc.phase_sync = tiny ? 1 : 0;                          // C2: 63.6 vs 82.4 ms; 100k/1M soups (early-exit rounds): 8 % slower
    if (kn.phase_sync) sc.phase_sync = *kn.phase_sync;
    // large trees (traversal bound by memory latency): the queue pipeline of rt_pipeline.h; tiny cache-resident ones: the megakernel
    // (measured on the 1 M-triangle frames, 1x MI355X: the pipeline's trace kernel is faster than the megakernel's traversal, but its
    // state traffic and sparse last iterations cost more than that gains, except where shading suspends often: volume marching)
    // round 3: a path without a medium can take the by-vertex form (rt_pipe_vertex.h: 1 M-triangle frame 69.9 ms); since the kernels are
    // built without the SLP vectorizer the 4-wave megakernel no longer spills and is as fast there (69.3 ms) and faster on C4's
    // material mix (71.3 vs 76.3 ms), so it stays the default for frames without a medium
    sc.pipeline = (!tiny && sf.medium) ? 1 : 0;
    if (kn.pipeline) sc.pipeline = *kn.pipeline != 0;
    const bool weighted = rd.integrator == RT_INTEGRATOR_DIRECT && rd.strategy == RT_STRATEGY_WEIGHTED;
    if (rd.max_depth > 250 || rd.max_depth < 0) sc.pipeline = 0;     // the slot's control word holds depth in 8 bits
    if (rq.dims_max_n >= 65535) sc.pipeline = 0;                     // ... and the light / sample cursors in 16 bits each
    if (sf.n_lights >= 65535u) sc.pipeline = 0;
    if (weighted) sc.pipeline = 0;    // three megakernel passes (rt_weighted.h)
    if (rd.integrator == RT_INTEGRATOR_BIDIRECTIONAL) { sc.pipeline = 0; sc.xcd_bands = 0; }   // rt::bidir_kernel (rt_bidir.h): a persistent kernel of its own, one work counter
    if (rd.integrator == RT_INTEGRATOR_DEBUG) { sc.pipeline = 0; sc.high_occupancy = 0; }     // flavour::Debug: the megakernel, one kernel per (medium, accelerator, counting), whatever the knobs say
    if (ext.shard_count == 1 && !sc.pipeline) {
        // One shard: the tiles partition nothing, and the megakernel then renders the sample extent in scanline order.  2-D tiles pad the extent to
        // whole tiles and every dropped padding item idles a lane for about a ray's time: 64 x 64 tiles cost C3 5 % of its frame
        // (profiles/r03_work_order.txt).  The queue pipeline keeps the caller's tiles: with millions of paths in flight their compactness is
        // worth more (C5: L2 misses 5.3 G per frame in 64 x 64 tiles, 6.3 G in scanline order; 328 vs 332 ms).
        Extent &e = sc.extent;
        e.tile_w = e.tile_h = e.tiles_x = 0; e.tile_pixels = 1;
        e.total_work = e.total_pixels * e.spp;
        // The counter hands the scanline-addressed samples out in 32 x 32-pixel blocks (clipped at the extent's edges: no padding, nothing dropped):
        // C3's kernel 12.68 -> 12.18 ms on top of the XCD bands, the path frames and C2 unchanged (profiles/r04_mega_tile_scan.txt).
        sc.mega_tile = 32;
        if (kn.mega_tile) sc.mega_tile = std::max(0, *kn.mega_tile);
        if (sc.mega_tile > 4096 || e.total_work > 0xffffffffull) sc.mega_tile = 0;
    }
    if (sc.trav_mode != 3 || sc.high_occupancy) sc.trav_mode = 2;  // (the high-occupancy kernels carry no pooled-leaf scratch)
    // A frame whose sampler, camera, work order and sample requests are what fixed::Frame states takes the twin compiled for them (rt_fixed_frame.h);
    // PBRT_HIP_FIXED_FRAME=0 keeps it on the generic kernel (the films are the same bits: tests/test_gpu_fixed_frame.py)
    const fixed::Facts facts{rd.integrator, rd.sampler, weighted, sf.lens_radius, sf.camera_type, ext.shard_count, sc.mega_tile, rq.dims_max_n,
                             sf.counting, sf.has_ext, sf.medium, sc.high_occupancy != 0};
    sc.fixed_frame = fixed::qualifies(facts);
    if (kn.fixed_frame) sc.fixed_frame = sc.fixed_frame && *kn.fixed_frame != 0;
    // ... and where the scene has one light (and, a second axis, no material with a specular lobe) the twin compiled for that too;
    // a scene created under PBRT_HIP_FIXED_SCENE=0 (a scene fact, read with the scene's other knobs: it can only turn the twin off) keeps its frames on
    // the fixed-frame kernel (the same bits again: tests/test_gpu_fixed_scene.py)
    sc.fixed_scene = sc.fixed_frame && sf.scene_twins ? fixed::scene_qualifies(facts, fixed::SceneFacts{sf.n_lights, sf.specular_materials}) : 0;
    // PathIntegrator without a medium in the queue pipeline: one shade pass per path vertex, all of a vertex's rays in one trace launch (rt_pipe_vertex.h)
    sc.by_vertex = sc.pipeline && rd.integrator == RT_INTEGRATOR_PATH && !sf.medium;
    if (kn.pipe_vertex) sc.by_vertex = sc.by_vertex && *kn.pipe_vertex != 0;
    return sc;
}

// ---------------------------------------------------------------------------------------------- 4. the medium's march bounds
struct March { int vol_nmax = 0, dens_cap = 0; };      // DevFrame::vol_nmax (bind_scratch sizes the march samples from it), DevFrame::dens_cap
inline Refusal plan_march(const RtRenderDesc &rd, const SceneFacts &sf, March &m) {
    m = March{};
    if (!sf.medium) return Refusal{};
    if (!(rd.step_size > 0.f)) return refuse(RT_EINVAL, "rt_render: volume integrator stepsize must be positive");
    if (rd.volume_integrator != RT_VOLUME_EMISSION && rd.volume_integrator != RT_VOLUME_SINGLE) return refuse(RT_EINVAL, "rt_render: unknown volume integrator");
    const float ex = sf.vol_p1[0] - sf.vol_p0[0], ey = sf.vol_p1[1] - sf.vol_p0[1], ez = sf.vol_p1[2] - sf.vol_p0[2];
    const double diag = std::sqrt(double(ex) * ex + double(ey) * ey + double(ez) * ez);
    const double nsteps = std::ceil(diag / rd.step_size) + 2;
    if (nsteps > 65536) return refuse(RT_EINVAL, "rt_render: stepsize too small for the medium (more than 65536 march steps)");
    int vol_nmax = int(nsteps);
    if (sf.density_kind != RT_DENSITY_NONE) {
        // DensityRegion::Tau (volume.cpp:137-153) marches `while (t0 < t1) t0 += step` along the normalised world-space ray: its samples are bounded by
        // the volume's world diagonal over the smallest step (.5f * stepsize), and the loop only ends if t + .5f * stepsize > t for every t a ray can
        // reach -- bounded by the union of the scene bound, the camera position and the volume's world bound (ray parameters start at mint >= 0)
        const double *wb = sf.vol_world;
        const double wx = wb[3] - wb[0], wy = wb[4] - wb[1], wz = wb[5] - wb[2];
        const double wdiag = std::sqrt(wx * wx + wy * wy + wz * wz);
        const float half = .5f * rd.step_size;
        const double taus = std::ceil(wdiag / double(half)) + 2;
        if (taus > double(1 << 20)) return refuse(RT_EINVAL, "rt_render: stepsize too small for the density region (an optical-depth march would take more than 2^20 samples)");
        double u[6] = {wb[0], wb[1], wb[2], wb[3], wb[4], wb[5]};
        for (int i = 0; i < 3; ++i) { u[i] = std::min(u[i], sf.cam_pos[i]); u[3 + i] = std::max(u[3 + i], sf.cam_pos[i]); }
        const float *sb = sf.bounds;
        if (sb[0] <= sb[3] && sb[1] <= sb[4] && sb[2] <= sb[5])
            for (int i = 0; i < 3; ++i) { u[i] = std::min(u[i], double(sb[i])); u[3 + i] = std::max(u[3 + i], double(sb[3 + i])); }
        const double ux = u[3] - u[0], uy = u[4] - u[1], uz = u[5] - u[2];
        const float tmax = std::nextafter(float(std::sqrt(ux * ux + uy * uy + uz * uz)), INFINITY);
        volatile float tv = tmax;                                               // the device's float addition, not a wider one
        const float adv = tv + half;
        if (!std::isfinite(tmax) || !(adv > tmax))
            return refuse(RT_EINVAL, "rt_render: stepsize too small for the density region: at the scene's ray parameters t + .5 * stepsize == t, the optical-depth march would not advance");
        m.dens_cap = int(taus);
        vol_nmax = std::max(vol_nmax, int(std::ceil(wdiag / rd.step_size)) + 2);     // march steps along a world-space ray (a scaled volume)
        if (vol_nmax > 65536) return refuse(RT_EINVAL, "rt_render: stepsize too small for the medium (more than 65536 march steps)");
    }
    m.vol_nmax = vol_nmax;
    return Refusal{};
}

// ---------------------------------------------------------------------------------------------- 5. a radiance query (rt_radiance_device)
// Rays first .. first + n - 1 of the caller stand in for the camera rays of camera samples first .. first + n - 1 of the frame `rd` describes, in
// scanline order (pixel * spp + s: the order of rt_samples_read and rt_camera_rays_device on one shard).  The sample requests are the frame's
// (plan_requests: they are the sample set); the schedule is the frame's turned into a query's: the work extent is the n rays, always the
// megakernel (flavour::Rays: natural allocation, no fixed twin), no tile order -- the rays' coherence is the caller's business.
struct QueryRange { unsigned long long first = 0; unsigned n = 0; };
inline Refusal plan_query(const RtRenderDesc &rd, const QueryRange &q, Schedule &sc) {
    if (rd.integrator == RT_INTEGRATOR_BIDIRECTIONAL) return refuse(RT_EINVAL, "rt_radiance_device: the bidirectional integrator is not supported (its light subpaths belong to no single ray)");
    if (rd.integrator == RT_INTEGRATOR_DEBUG) return refuse(RT_EINVAL, "rt_radiance_device: the debug integrator is not supported (it computes no radiance; rt_hit_geometry_device returns its quantities)");
    if (rd.integrator < RT_INTEGRATOR_WHITTED || rd.integrator > RT_INTEGRATOR_PATH) return refuse(RT_EINVAL, "unknown integrator");
    if (rd.integrator == RT_INTEGRATOR_DIRECT && rd.strategy == RT_STRATEGY_WEIGHTED)
        return refuse(RT_EINVAL, "rt_radiance_device: strategy \"weighted\" is not supported (its recurrence spans the whole frame in the sampler's order, transport.cpp:71-122)");
    if (rd.integrator == RT_INTEGRATOR_DIRECT && (rd.strategy < RT_STRATEGY_ALL || rd.strategy > RT_STRATEGY_WEIGHTED)) return refuse(RT_EINVAL, "rt_radiance_device: unknown direct lighting strategy");
    if (rd.max_depth < 0) return refuse(RT_EINVAL, "rt_radiance_device: negative maxdepth");
    Extent &e = sc.extent;
    if (e.shard_count != 1) return refuse(RT_EINVAL, "rt_radiance_device: shard_count != 1 (a query addresses the camera samples of the whole frame: one shard only)");
    const unsigned long long samples = e.total_pixels * (unsigned long long)e.spp;           // (< 2^32: plan_extent)
    if (q.first > samples || q.n > samples - q.first) return refuse(RT_EINVAL, "rt_radiance_device: first + n is beyond the frame's camera samples");
    e.tile_w = e.tile_h = e.tiles_x = 0; e.tile_pixels = 1;
    e.total_work = q.n;
    sc.pipeline = 0; sc.by_vertex = false; sc.fixed_frame = false; sc.fixed_scene = 0; sc.mega_tile = 0;
    sc.high_occupancy = 0;                                   // (the natural-allocation kernels carry the pooled-leaf scratch: trav_mode 3 stays where the frame has it)
    return Refusal{};
}

// ---------------------------------------------------------------------------------------------- 6. a film add (rt_film_add_device)
// Radiances first .. first + n - 1 of the caller stand in for those of camera samples first .. first + n - 1 of the frame `rd` describes, in the
// scanline order of plan_query; the film receives them as Scene::Render would hand them to Film::AddSample.  Only the sampler, film, filter, extent
// and shard fields of `rd` are read.  The plan: the refusals that need no device (film_w x film_h: the bound film, 0 x 0 when none is bound), the
// sample pixels and sample rows the range touches, the film rows a gather for it has to visit -- the sample rows widened by the filter's reach
// floor(width + .5) (a sample of sample pixel sy lies in [sy, sy + 1]: |y - sy| <= width + .5 for every film row y it can reach) and clipped to the
// crop window -- and the size of the call's staging buffer: one image position (two floats) per sample of the range.
struct FilmAdd {
    int spp = 0;
    int reach_x = 0, reach_y = 0;                    // floor(filter width + .5)
    unsigned long long pixel0 = 0, pixel1 = 0;       // sample pixels [pixel0, pixel1] of the sample extent in scanline order, the partial ones at both ends included
    int srow0 = 0, srow1 = -1;                       // sample rows [srow0, srow1], absolute (y_start + pixel / width)
    int row0 = 0, row_end = 0;                       // film rows [row0, row_end) relative to the crop window's first row; empty when the range reaches none
    size_t staging_floats = 0;
};
inline Refusal plan_film_add(const RtRenderDesc &rd, const QueryRange &q, int film_w, int film_h, FilmAdd &p) {
    p = FilmAdd{};
    Extent e;
    if (Refusal r = plan_extent(rd, e)) return r;
    if (e.shard_count != 1) return refuse(RT_EINVAL, "rt_film_add_device: shard_count != 1 (the radiances are addressed as the camera samples of the whole frame: one shard only)");
    const unsigned long long samples = e.total_pixels * (unsigned long long)e.spp;           // (< 2^32: plan_extent)
    if (q.first > samples || q.n > samples - q.first) return refuse(RT_EINVAL, "rt_film_add_device: first + n is beyond the frame's camera samples");
    if (!(rd.filter_x_width > 0.f) || !(rd.filter_y_width > 0.f)) return refuse(RT_EINVAL, "rt_film_add_device: filter widths must be positive");
    if (rd.x_pixel_start + (long long)rd.x_pixel_count > 32767 || rd.y_pixel_start + (long long)rd.y_pixel_count > 32767 || rd.x_pixel_start < -32768 || rd.y_pixel_start < -32768)
        return refuse(RT_EINVAL, "rt_film_add_device: film coordinates beyond 32767 (the gather packs sample footprints as int16)");
    if (rd.x_pixel_count < 1 || rd.y_pixel_count < 1) return refuse(RT_EINVAL, "rt_film_add_device: empty crop window");
    if (film_w == 0 && film_h == 0) return refuse(RT_ESTATE, "rt_film_add_device: no film bound (call rt_film_bind first)");
    if (rd.x_pixel_count != film_w || rd.y_pixel_count != film_h) return refuse(RT_EINVAL, "rt_film_add_device: film size does not match the bound film");
    p.spp = e.spp;
    // (a reach beyond the film's own coordinates reaches nothing more: clamped so that the sums below stay small)
    p.reach_x = int(std::min(std::floor(rd.filter_x_width + 0.5f), 65536.f)); p.reach_y = int(std::min(std::floor(rd.filter_y_width + 0.5f), 65536.f));
    if (q.n == 0) return Refusal{};
    const unsigned long long width = (unsigned long long)(rd.x_end - rd.x_start);
    p.pixel0 = q.first / unsigned(e.spp); p.pixel1 = (q.first + q.n - 1) / unsigned(e.spp);
    p.srow0 = rd.y_start + int(p.pixel0 / width); p.srow1 = rd.y_start + int(p.pixel1 / width);
    const long long lo = (long long)p.srow0 - p.reach_y - rd.y_pixel_start, hi = (long long)p.srow1 + p.reach_y - rd.y_pixel_start + 1;
    p.row0 = int(std::max(lo, 0ll)); p.row_end = int(std::min(hi, (long long)rd.y_pixel_count));
    if (p.row_end <= p.row0) p.row0 = p.row_end = 0;
    p.staging_floats = size_t(q.n) * 2;
    return Refusal{};
}

// ---------------------------------------------------------------------------------------------- 7. the launch
// What a frame asks of the kernel tables (rt_flavour.h: each family's index() turns it into the entry to launch).  rt_trace_* and the device-ray calls
// have no frame: no integrator, no schedule
inline flavour::Request request(const RtRenderDesc *rd, const SceneFacts &sf, const Schedule *sc) {
    return flavour::Request{rd ? rd->integrator : 0, sf.accel_kind == RT_ACCEL_GRID, sf.medium, sf.counting, sf.has_ext, sc && sc->high_occupancy != 0};
}
// The family a frame (or a radiance query) runs and the entry k of that family's table; scene_axes: the axes a FixedScene entry fixes, else 0.
// Pipeline has no one entry: render_pipeline picks its shade, trace and march kernels from the same request.
struct Launch {
    enum Family { Mega, Fixed, FixedScene, Debug, Weighted, Bidir, Rays, Pipeline } family = Mega;
    int integ = 0, k = 0, scene_axes = 0;
};
inline Launch plan_launch(const RtRenderDesc &rd, const SceneFacts &sf, const Schedule &sc, bool query) {
    const flavour::Request rq = request(&rd, sf, &sc);
    const int integ = rd.integrator;
    if (query) return Launch{Launch::Rays, integ, flavour::Rays::index(rq), 0};
    if (sc.pipeline) return Launch{Launch::Pipeline, integ, 0, 0};
    if (integ == RT_INTEGRATOR_BIDIRECTIONAL) return Launch{Launch::Bidir, integ, flavour::Bidir::index(rq), 0};
    if (integ == RT_INTEGRATOR_DIRECT && rd.strategy == RT_STRATEGY_WEIGHTED) return Launch{Launch::Weighted, integ, flavour::Weighted::index(rq), 0};
    if (integ == RT_INTEGRATOR_DEBUG) return Launch{Launch::Debug, integ, flavour::Debug::index(rq), 0};
    // the twin compiled for a fixed frame (rt_fixed_frame.h), where plan_schedule found that the frame qualifies, and that kernel's twin compiled for the
    // scene's one light (and all-matte material table) as well, where the schedule names its axes and the integrator has such twins
    if (sc.fixed_frame && flavour::FixedScene::has(integ) && flavour::FixedScene::has_axes(sc.fixed_scene))
        return Launch{Launch::FixedScene, integ, flavour::FixedScene::index(rq, sc.fixed_scene), sc.fixed_scene};
    if (sc.fixed_frame) return Launch{Launch::Fixed, integ, flavour::Fixed::index(rq), 0};
    return Launch{Launch::Mega, integ, flavour::Mega::index(rq), 0};
}

}  // namespace plan
}  // namespace rt
