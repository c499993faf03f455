// rt_fixed_frame.h -- the "fixed frame": what the large-scene megakernels may assume at compile time.  The between-rays code of rt_integrate.h and the
// work fetch of rt_render_kernel.h select the sampler, the camera model, the lens and the work order at run time (a scalar load of a descriptor field, a
// wait, a compare and a branch each, and the code of every alternative in every instantiation).  A traits type as their trailing template parameter turns
// those selections into constants: fixed::Any (the default) is the code as it always was, fixed::Frame the twin for the frames qualifies() admits.  What a
// fixed kernel still computes are the expressions the generic kernel runs for such a frame, so the films are bit-identical.  The family of the fixed
// kernels (flavour::Fixed, rt_mega_f.hip) is declared here too, and so are the traits of the scene (fixed::Scene: its one light, its all-matte material
// table) with the family of their kernels (flavour::FixedScene, rt_mega_fs{d,p}.hip).  No HIP header: tests/fixed_frame_host_test.cpp and
// tests/fixed_scene_host_test.cpp check the rules with a host compiler.
#pragma once
#include "rt_flavour.h"

// Each axis can be switched off alone with -DRT_FIXED_<AXIS>=0 (measurements: profiles/fixed_frame_kernels.txt); qualifies() stays as strict as it is.
#ifndef RT_FIXED_SAMPLER
#define RT_FIXED_SAMPLER 1
#endif
#ifndef RT_FIXED_N1
#define RT_FIXED_N1 1
#endif
#ifndef RT_FIXED_CAMERA
#define RT_FIXED_CAMERA 1
#endif
#ifndef RT_FIXED_TILE_ORDER
#define RT_FIXED_TILE_ORDER 1
#endif
// ... and the two axes of the scene (fixed::Scene below; measurements: profiles/fixed_scene_kernels.txt); scene_qualifies() stays as strict as it is
#ifndef RT_FIXED_ONE_LIGHT
#define RT_FIXED_ONE_LIGHT 1
#endif
#ifndef RT_FIXED_NO_SPECULAR
#define RT_FIXED_NO_SPECULAR 1
#endif

namespace rt {
namespace fixed {

// nothing known at compile time: every selection is made at run time
struct Any {
    static constexpr int sampler = -1;               // RT_SAMPLER_*, or -1: any (DevFrame::sampler decides)
    static constexpr bool no_lens = false;           // RtCamera::lens_radius == 0
    static constexpr bool no_env_camera = false;     // RtCamera::type is perspective or orthographic (still a run-time value between those two)
    static constexpr bool tile_order = false;        // single shard with DevFrame::mega_tile > 0: tile_order_to_sample hands out the work, fewer than 2^32 samples
    static constexpr bool all_n1 = false;            // every DimReq of the frame has n == 1 (one_d, two_d, light_dims)
    static constexpr bool caller_rays = false;       // the ray-source axis: the camera (false), or the caller's RtRay array (DevFrame::q_rays; Rays below)
};
// the frames of qualifies()
struct Frame {
    static constexpr int sampler = RT_FIXED_SAMPLER ? int(RT_SAMPLER_STRATIFIED) : -1;
    static constexpr bool no_lens = RT_FIXED_CAMERA != 0;
    static constexpr bool no_env_camera = RT_FIXED_CAMERA != 0;
    static constexpr bool tile_order = RT_FIXED_TILE_ORDER != 0;
    static constexpr bool all_n1 = RT_FIXED_N1 != 0;
    static constexpr bool caller_rays = false;
};
// A radiance query (rt_radiance_device): nothing else known at compile time, and the rays are the caller's.  Work item w of [0, DevFrame::total_work) is
// camera sample DevFrame::q_first + w of the frame in scanline order (no tile order, nothing falls off an extent); setup_sample sets the sample set up
// as for that camera sample and loads DevFrame::q_rays[w] in place of camera_ray; the end of the sample stores {L, alpha} at DevFrame::q_out[w].
struct Rays : Any {
    static constexpr bool caller_rays = true;
};

// what the host knows of a frame and its scene when it picks the kernel (plan_schedule and plan_launch, rt_frame_plan.h)
struct Facts {
    int integrator;          // RtRenderDesc::integrator
    int sampler;             // DevFrame::sampler
    bool weighted;           // DirectLighting "weighted": a kernel family of its own
    float lens_radius;       // RtCamera::lens_radius
    int camera_type;         // RtCamera::type
    int shard_count;         // DevFrame::shard_count
    int mega_tile;           // DevFrame::mega_tile
    int dims_max_n;          // DevFrame::dims_max_n: the largest n of the frame's sample requests (a light's nsamples); 0 when it has none
    bool counting, ext, vol; // RtScene::counting, has_ext, a medium
    bool high_occ;           // DevFrame::high_occupancy
};
// A frame takes the fixed kernel when everything Frame states holds, and the kernel it would take otherwise is one of the six that have a fixed twin
// (Whitted, DirectLighting "all" / "one", Path; timed, no EXT code, no medium, high occupancy).  Jitter stays a run-time value.
constexpr bool qualifies(const Facts &f) {
    return f.integrator >= RT_INTEGRATOR_WHITTED && f.integrator <= RT_INTEGRATOR_PATH && !f.weighted &&
           f.sampler == RT_SAMPLER_STRATIFIED &&
           f.lens_radius == 0.f &&
           (f.camera_type == RT_CAMERA_PERSPECTIVE || f.camera_type == RT_CAMERA_ORTHOGRAPHIC) &&
           f.shard_count == 1 && f.mega_tile > 0 &&
           f.dims_max_n <= 1 &&
           !f.counting && !f.ext && !f.vol && f.high_occ;
}

// ---- the scene.  The stage bodies also ask, in every pass, what the SCENE fixed when it was loaded: which light (a per-lane index into the light
// records, their triangles and their sample requests, although a scene with one light has one address for all 64 lanes), and whether the material at
// hand has a specular lobe (three draws and a bsdf_sample_f per direction of the Whitted / DirectLighting recursion, which an all-matte table answers
// with "no lobe" every time).  A second traits type, the parameter after FX, turns these into constants the same way: fixed::AnyScene (the default) is
// the code as it was, fixed::Scene<...> the twin for the scenes scene_qualifies() admits.  The two axes are independent.
struct AnyScene {
    static constexpr bool one_light = false;         // DevScene::n_lights == 1: the light index is 0 wherever a light, its triangles or its sample requests are read
    static constexpr bool no_specular = false;       // no material has a specular lobe: no recursion frame is ever pushed, PathIntegrator's specularBounce stays false
    static constexpr bool accel_known = false;       // launch_ray takes the accelerator from the kernel's ACCEL, not from DevScene::accel_kind
};
template <bool ONE_LIGHT, bool NO_SPECULAR> struct Scene {
    static constexpr bool accel_known = true;
    static constexpr bool one_light = ONE_LIGHT && RT_FIXED_ONE_LIGHT != 0;
    static constexpr bool no_specular = NO_SPECULAR && RT_FIXED_NO_SPECULAR != 0;
};
enum { SCENE_ONE_LIGHT = 1, SCENE_NO_SPECULAR = 2 };      // a bit per axis: Schedule::fixed_scene, RtRenderStats::fixed_scene
// what the host knows of the scene's lights and materials (plan::SceneFacts::n_lights, ::specular_materials)
struct SceneFacts {
    unsigned n_lights;       // DevScene::n_lights
    bool specular;           // some material is not matte (mirror, glass: the materials of a scene without EXT code), whether or not its lobes are black
};
// The axes of the scene twin a frame takes, or 0: the frame takes a fixed-frame kernel of DirectLighting or Path (the integrators that have scene twins),
// and the scene has one light -- every twin is compiled for that, with or without "no specular lobe" (flavour::FixedScene)
constexpr int scene_qualifies(const Facts &f, const SceneFacts &s) {
    if (!qualifies(f) || (f.integrator != RT_INTEGRATOR_DIRECT && f.integrator != RT_INTEGRATOR_PATH)) return 0;
    if (s.n_lights != 1u) return 0;
    return SCENE_ONE_LIGHT | (s.specular ? 0 : SCENE_NO_SPECULAR);
}

}  // namespace fixed

namespace flavour {
// rt::render_kernel_fixed<..., fixed::Frame> (rt_mega_f.hip): the fixed twins of Mega's entries 8 and 9 (high occupancy, timed, no EXT, no medium; kd-tree and
// grid) of the three integrators, in one table: entry 2 * integrator + grid
struct Fixed {
    static constexpr int N = 6;
    static constexpr int index(const Request &r) { return 2 * r.integ + (r.grid ? 1 : 0); }
    static constexpr int integrator(int k) { return k >> 1; }
    static constexpr Flavour flavour(int k) { return Flavour{false, k & 1, false, false, RT_HIGH_OCC_WAVES, true}; }
    // the request entry k serves (Flavour::request() does not know the integrator)
    static constexpr Request request(int k) { Request r = flavour(k).request(); r.integ = integrator(k); return r; }
    // ... and the entry of Mega's table it is the twin of
    static constexpr int generic(int k) { return Mega::index(request(k)); }
};
constexpr bool fixed_round_trips() {
    for (int k = 0; k < Fixed::N; ++k) {
        if (Fixed::index(Fixed::request(k)) != k) return false;
        const Flavour g = Mega::flavour(Fixed::generic(k), Fixed::integrator(k)), f = Fixed::flavour(k);
        if (g.count != f.count || g.accel != f.accel || g.vol != f.vol || g.ext != f.ext || g.waves != f.waves || g.high_occ != f.high_occ) return false;
    }
    return true;
}
static_assert(fixed_round_trips(), "Fixed: index(request(k)) != k, or entry k is not the twin of a Mega entry");

// rt::render_kernel_scene<..., fixed::Frame, fixed::Scene<...>> (rt_mega_fs{d,p}.hip): the scene twins of Fixed's DirectLighting and Path entries, a table
// per integrator: entry 2 * grid + (no specular lobe).  Every entry is compiled for one light.
struct FixedScene {
    static constexpr int N = 4;
    static constexpr bool has(int integ) { return integ == RT_INTEGRATOR_DIRECT || integ == RT_INTEGRATOR_PATH; }
    static constexpr bool has_axes(int axes) { return axes == fixed::SCENE_ONE_LIGHT || axes == (fixed::SCENE_ONE_LIGHT | fixed::SCENE_NO_SPECULAR); }
    static constexpr int index(const Request &r, int axes) { return (r.grid ? 2 : 0) + ((axes & fixed::SCENE_NO_SPECULAR) ? 1 : 0); }
    static constexpr int axes(int k) { return fixed::SCENE_ONE_LIGHT | ((k & 1) ? fixed::SCENE_NO_SPECULAR : 0); }
    static constexpr Flavour flavour(int k) { return Flavour{false, k >> 1, false, false, RT_HIGH_OCC_WAVES, true}; }
    static constexpr Request request(int k, int integ) { Request r = flavour(k).request(); r.integ = integ; return r; }
    // ... and the entry of Fixed's table it is the twin of
    static constexpr int fixed_twin(int k, int integ) { return Fixed::index(request(k, integ)); }
};
constexpr bool fixed_scene_round_trips() {
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ) {
        if (!FixedScene::has(integ)) continue;
        for (int k = 0; k < FixedScene::N; ++k) {
            if (FixedScene::index(FixedScene::request(k, integ), FixedScene::axes(k)) != k || !FixedScene::has_axes(FixedScene::axes(k))) return false;
            const int t = FixedScene::fixed_twin(k, integ);
            const Flavour g = Fixed::flavour(t), f = FixedScene::flavour(k);
            if (Fixed::integrator(t) != integ) return false;
            if (g.count != f.count || g.accel != f.accel || g.vol != f.vol || g.ext != f.ext || g.waves != f.waves || g.high_occ != f.high_occ) return false;
        }
    }
    return true;
}
static_assert(fixed_scene_round_trips(), "FixedScene: index(request(k), axes(k)) != k, or entry k is not the twin of a Fixed entry");
}  // namespace flavour
}  // namespace rt
