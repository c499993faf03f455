// rt_flavour.h -- which kernel instantiation a frame runs.  A frame asks with a Request; each of the eight kernel families has index(request), the
// entry of its table that serves the request, flavour(k), the template arguments of entry k, and N, the table's size.  The translation units build
// their tables from flavour(k) (RT_FLAVOUR_TABLE below), rt_host.h sizes the resident grids by N and rt_kernels.hip picks entries with index():
// a table's order, its size and the host's choice cannot disagree.  (A ninth family, flavour::Fixed -- the twins of six Mega entries compiled for a
// fixed frame -- lives in rt_fixed_frame.h with the traits it is built from; flavour::Rays below, the radiance query, is built from fixed::Rays of that header.)  No HIP header: tests/flavour_host_test.cpp checks the rules with a host compiler.
#pragma once
#include "../../../include/pbrt_hip.h"
#include <array>
#include <utility>

// The -D knobs of rt_render_kernel.h (waves per SIMD the register allocator must make room for: natural allocation, and the high-occupancy
// flavour), with its defaults for a unit that does not include it
#ifndef RT_MIN_WAVES
#define RT_MIN_WAVES 1
#endif
#ifndef RT_HIGH_OCC_WAVES
#define RT_HIGH_OCC_WAVES 4
#endif

namespace rt {
namespace flavour {

// what a frame asks for: the integrator, the accelerator (grid or kd-tree), a medium, ray counters (RtScene::counting), the glossy / quadric code
// (EXT: RtScene::has_ext) and the register-capped kernel (DevFrame::high_occupancy)
struct Request { int integ; bool grid, vol, count, ext, high_occ; };

// the template arguments of one table entry (those its family has; the others stay false), and the request that selects it
struct Flavour {
    bool count; int accel; bool vol, ext; int waves; bool high_occ;
    constexpr Request request() const { return Request{0, accel == RT_ACCEL_GRID, vol, count, ext, high_occ}; }
};

// Megakernel, shade, by-vertex and march kernels come in threes: 0 the timed kernel, 1 its counting twin, which always carries the EXT code (it is not
// timed), 2 the timed kernel with the EXT code (powf and the second lobe cost ~17 VGPRs, one wave per SIMD less for DirectLighting)
constexpr int triple(const Request &r) { return r.count ? 1 : r.ext ? 2 : 0; }
constexpr Flavour of_triple(int f, int accel, bool vol) { return Flavour{f == 1, accel, vol, f != 0, RT_MIN_WAVES, false}; }

// rt::render_kernel per integrator (rt_mega_{w,d,p}.hip): the triple at (VOL, ACCEL) -- 0..7 hold the timed kernel and its counting twin, 12..15 the timed
// kernel with EXT -- and at 8..11 the high-occupancy flavour, which only a timed frame without EXT takes: EXT beats high occupancy
struct Mega {
    static constexpr int N = 16;
    static constexpr int index(const Request &r) {
        const int va = (r.vol ? 2 : 0) + (r.grid ? 1 : 0), f = triple(r);
        return f == 2 ? 12 + va : (f == 0 && r.high_occ) ? 8 + va : va * 2 + f;
    }
    // waves per SIMD the timed natural-allocation kernels (no medium, no EXT) are held to: DirectLighting's kd-tree kernel allocates 170 VGPRs on
    // its own, 2 above the 3-wave step of gfx950 (168); asking for 3 waves costs two spilled registers and buys the third wave
    static constexpr int natural_waves(int integ, bool vol) { return integ == RT_INTEGRATOR_DIRECT && !vol ? 3 : RT_MIN_WAVES; }
    static constexpr Flavour flavour(int k, int integ) {
        const int va = k < 8 ? k >> 1 : k & 3, f = k < 8 ? k & 1 : k < 12 ? 0 : 2;
        Flavour fl = of_triple(f, va & 1, (va & 2) != 0);
        fl.high_occ = k >= 8 && k < 12;
        if (f == 0) fl.waves = fl.high_occ ? RT_HIGH_OCC_WAVES : natural_waves(integ, fl.vol);
        return fl;
    }
};
// rt::render_kernel for DirectLighting "weighted" (rt_mega_dw.hip): all with EXT at natural allocation -- this strategy's frame time is set by its
// sequential recurrence, not by these kernels.  The timed kernels without a medium allocate 170 VGPRs on their own since the shinymetal / translucent
// lobes and the infinite light, 2 above the 3-wave step: they are held to 3 waves as DirectLighting's is, which costs no scratch
struct Weighted {
    static constexpr int N = 8;
    static constexpr int index(const Request &r) { return ((r.vol ? 2 : 0) + (r.grid ? 1 : 0)) * 2 + (r.count ? 1 : 0); }
    static constexpr Flavour flavour(int k) { return Flavour{(k & 1) != 0, (k >> 1) & 1, (k & 4) != 0, true, (k & 1) == 0 && (k & 4) == 0 ? 3 : RT_MIN_WAVES, false}; }
};
// rt::bidir_kernel (rt_mega_b.hip): one flavour per accelerator covers every material, quadric and light (the EXT shading set) at natural allocation
struct Bidir {
    static constexpr int N = 4;
    static constexpr int index(const Request &r) { return (r.grid ? 2 : 0) + (r.count ? 1 : 0); }
    static constexpr Flavour flavour(int k) { return Flavour{(k & 1) != 0, k >> 1, false, true, RT_MIN_WAVES, false}; }
};
// rt::render_kernel for the debug integrator (RT_INTEGRATOR_DEBUG, rt_mega_g.hip): the timed kernel and its counting twin per (VOL, ACCEL), all with the
// hit-frame code of the EXT set (quadric u / v, per-vertex N / S, mesh uvs); no second flavour -- a debug frame always runs these.  All allocate what the
// compiler asks for.  Without a medium that is 95 - 107 VGPRs, below the 4-wave step (128), so those four are launched with that bound: it caps nothing and
// leaves out the pooled-leaf LDS (rt_render_kernel.h POOL), which held the kd-tree kernels to 3 waves per SIMD (1 M-triangle frame 2.31 -> 1.92 ms)
struct Debug {
    static constexpr int N = 8;
    static constexpr int index(const Request &r) { return ((r.vol ? 2 : 0) + (r.grid ? 1 : 0)) * 2 + (r.count ? 1 : 0); }
    static constexpr Flavour flavour(int k) { return Flavour{(k & 1) != 0, (k >> 1) & 1, (k & 4) != 0, true, (k & 4) != 0 ? RT_MIN_WAVES : RT_HIGH_OCC_WAVES, false}; }
};
// rt::render_kernel_fixed<..., fixed::Rays> per integrator (rt_mega_r{w,d,p}.hip): the radiance query for caller-supplied rays (rt_radiance_device).  A
// caller's scene may hold any material, quadric or light and a query is not the headline: as Bidir and Debug, one flavour per (VOL, ACCEL, counting), all
// with the EXT shading set at natural allocation -- the code of Mega's entries 12..15 (timed) and 1, 3, 5, 7 (counting) with another ray source.  No
// high-occupancy and no fixed-frame twins.  The path integrator's counting kernel on a grid is held to 3 waves as its Mega twin is (rt_render_kernel.h)
struct Rays {
    static constexpr int N = 8;
    static constexpr int index(const Request &r) { return ((r.vol ? 2 : 0) + (r.grid ? 1 : 0)) * 2 + (r.count ? 1 : 0); }
    static constexpr Flavour flavour(int k, int integ) {
        const bool count = (k & 1) != 0, grid = ((k >> 1) & 1) != 0, vol = (k & 4) != 0;
        return Flavour{count, grid ? 1 : 0, vol, true, (count && integ == RT_INTEGRATOR_PATH && grid && !vol && RT_MIN_WAVES < 3) ? 3 : RT_MIN_WAVES, false};
    }
    // the entry of Mega's table whose shading code entry k carries
    static constexpr int generic(int k) { Request r = flavour(k, 0).request(); r.ext = true; return Mega::index(r); }
};
// rt::pipe_shade_kernel per integrator (rt_pipe_{w,d,p}.hip): the triple per VOL
struct Shade {
    static constexpr int N = 6;
    static constexpr int index(const Request &r) { return (r.vol ? 3 : 0) + triple(r); }
    static constexpr Flavour flavour(int k) { return of_triple(k % 3, 0, k >= 3); }
};
// rt::pipe_vertex_kernel (rt_pipe_v.hip): the triple
struct Vertex {
    static constexpr int N = 3;
    static constexpr int index(const Request &r) { return triple(r); }
    static constexpr Flavour flavour(int k) { return of_triple(k, 0, false); }
};
// rt::pipe_march_kernel (rt_march.hip): the triple per ACCEL
struct March {
    static constexpr int N = 6;
    static constexpr int index(const Request &r) { return (r.grid ? 3 : 0) + triple(r); }
    static constexpr Flavour flavour(int k) { return of_triple(k % 3, k / 3, false); }
};
// rt::pipe_trace_kernel (rt_trace.hip), the one family with a counting kernel without EXT (per-primitive records + leaf entries, like the timed one):
// per ACCEL the triple, then that kernel
struct Trace {
    static constexpr int N = 8;
    static constexpr int index(const Request &r) { return (r.grid ? 4 : 0) + (r.count && !r.ext ? 3 : triple(r)); }
    static constexpr Flavour flavour(int k) { return (k & 3) == 3 ? Flavour{true, k >> 2, false, false, RT_MIN_WAVES, false} : of_triple(k & 3, k >> 2, false); }
};

template <class Family, class... Integ> constexpr bool round_trips(Integ... integ) {
    for (int k = 0; k < Family::N; ++k) if (Family::index(Family::flavour(k, integ...).request()) != k) return false;
    return true;
}
static_assert(round_trips<Mega>(RT_INTEGRATOR_WHITTED) && round_trips<Mega>(RT_INTEGRATOR_DIRECT) && round_trips<Mega>(RT_INTEGRATOR_PATH), "Mega: index(flavour(k)) != k");
static_assert(round_trips<Weighted>() && round_trips<Bidir>(), "Weighted / Bidir: index(flavour(k)) != k");
static_assert(round_trips<Debug>(), "Debug: index(flavour(k)) != k");
static_assert(round_trips<Rays>(RT_INTEGRATOR_WHITTED) && round_trips<Rays>(RT_INTEGRATOR_DIRECT) && round_trips<Rays>(RT_INTEGRATOR_PATH), "Rays: index(flavour(k)) != k");
static_assert(round_trips<Shade>() && round_trips<Vertex>() && round_trips<March>() && round_trips<Trace>(), "pipeline: index(flavour(k)) != k");

// A family's table: one value per entry, in the order of flavour(k) -- the kernels of a translation unit, the resident grids of a scene (rt_host.h)
template <class T, class Family> using Table = std::array<T, Family::N>;
template <class Unit, int... K> constexpr auto table(std::integer_sequence<int, K...>) {
    return std::array<decltype(Unit::template entry<0>()), sizeof...(K)>{{Unit::template entry<K>()...}};
}

}  // namespace flavour
}  // namespace rt

// The one table of a translation unit (inside namespace rt): entry K is the kernel named after the flavour `f` = flavour::FLAVOUR_OF_K, e.g.
//     RT_FLAVOUR_TABLE(g_pipe_march, PipeMarchFn, March, March::flavour(K), pipe_march_kernel<f.count, f.accel, f.ext>)
#define RT_FLAVOUR_TABLE(NAME, FN, FAMILY, FLAVOUR_OF_K, ...)                                                                                       \
    namespace { struct Unit { template <int K> static constexpr FN entry() { constexpr flavour::Flavour f = flavour::FLAVOUR_OF_K; return __VA_ARGS__; } }; }  \
    extern const flavour::Table<FN, flavour::FAMILY> NAME;                                                                                          \
    const flavour::Table<FN, flavour::FAMILY> NAME = flavour::table<Unit>(std::make_integer_sequence<int, flavour::FAMILY::N>{});
