// rt_render_kernel.h -- the persistent-thread megakernel: Scene::Render's sample loop (scene.cpp:42-84) with every lane running
// the state machine of rt_integrate.h and all lanes of a wave sharing ONE traversal loop.  Used for small, cache-resident scenes
// (Cornell: VALU-bound); large scenes go through the queue pipeline of rt_pipeline.h.  Instantiated per integrator in
// rt_mega_{w,d,p}.hip (separate translation units so that the library builds in parallel).
#pragma once
#include "rt_integrate.h"

namespace rt {

#ifndef RT_MEGA_CHUNK
#define RT_MEGA_CHUNK 64          // camera samples a megakernel wave takes from the global work counter at a time
#endif
static_assert(RT_MEGA_CHUNK >= 64, "one fresh chunk must cover a whole wave's fetch");
// a value every lane of the wave holds equally, moved to scalar registers
RT_DEV unsigned long long uniform64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(v)), hi = __builtin_amdgcn_readfirstlane(unsigned(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}


// first work item of band r of n (multiples of the chunk size, so that a chunk never straddles two bands; band n ends at `total`)
RT_DEV unsigned long long band_lo(unsigned long long total, unsigned r, unsigned n) {
    if (r >= n) return total;
    return (total / RT_MEGA_CHUNK) * r / n * RT_MEGA_CHUNK;
}

// ------------------------------------------------------------------------------------------ kernels
#ifndef RT_MIN_WAVES
#define RT_MIN_WAVES 1
#endif
// the path integrator by vertex (rt_integrate.h advance_pass_byv) in the register-capped flavour of the kd-tree / grid kernels without a medium
#ifndef RT_MEGA_BYV
#define RT_MEGA_BYV 1
#endif


// waves per SIMD of the high-occupancy flavour: 4 = 128 VGPRs.  5 (96 VGPRs) was marginally faster at one point but its
// spill placement swings with every code change (measured 108 -> 153 ms on the 1 M-triangle path frame for the same
// algorithm); 4 is stable: 101 ms there, 138 ms on the 100 k soup.
#ifndef RT_HIGH_OCC_WAVES
#define RT_HIGH_OCC_WAVES 4
#endif
// Scene and frame descriptors are read through pointers (uniform addresses -> scalar loads on demand) instead of
// being passed by value: the by-value form pinned >100 SGPRs and spilled them.
// MINW = minimum waves per SIMD the register allocator must make room for: 1 = natural allocation (~160 VGPRs, 3 waves/SIMD,
// best when VALU-bound: tiny cache-resident scenes); RT_HIGH_OCC_WAVES = 4 caps at 128 VGPRs (some spills to scratch) for
// 4 waves/SIMD: +20 % on the memory-latency-bound 100k..1M-triangle scenes, -15 % on Cornell.
// The body is rt_render_body.inc, the text of both kernels below: FX (rt_fixed_frame.h) is what it may assume of its frame at compile time.
// render_kernel keeps its six template arguments and assumes nothing (fixed::Any) -- its instantiations keep their symbol names, which tests/test_abi.py
// looks up in the compiler's resource reports, and their code (a body inlined from a function of its own moved spills in a dozen of them);
// render_kernel_fixed carries the traits as a seventh argument.
template <bool COUNT, int INTEG, int ACCEL, bool VOL, int MINW, bool EXT>
__global__ __launch_bounds__(RT_BLOCK, (EXT && COUNT && INTEG == RT_INTEGRATOR_PATH && ACCEL == RT_ACCEL_GRID && !VOL && MINW < 3) ? 3 : MINW) void render_kernel(const DevScene *__restrict__ scp,
                                                                       const DevFrame *__restrict__ frp) {
    using FX = fixed::Any;
    using SX = fixed::AnyScene;
#include "rt_render_body.inc"
}
// the twin of render_kernel<COUNT, INTEG, ACCEL, VOL, MINW, EXT> for the frames FX describes (flavour::Fixed, rt_mega_f.hip)
template <bool COUNT, int INTEG, int ACCEL, bool VOL, int MINW, bool EXT, class FX>
__global__ __launch_bounds__(RT_BLOCK, MINW) void render_kernel_fixed(const DevScene *__restrict__ scp, const DevFrame *__restrict__ frp) {
    using SX = fixed::AnyScene;
#include "rt_render_body.inc"
}
// ... and the twin of render_kernel_fixed<..., FX> for the scenes SX describes (flavour::FixedScene, rt_mega_fs{d,p}.hip): a kernel of its own name, so that
// the fixed-frame kernels keep theirs
template <bool COUNT, int INTEG, int ACCEL, bool VOL, int MINW, bool EXT, class FX, class SX>
__global__ __launch_bounds__(RT_BLOCK, MINW) void render_kernel_scene(const DevScene *__restrict__ scp, const DevFrame *__restrict__ frp) {
#include "rt_render_body.inc"
}

typedef void (*RenderKernelFn)(const DevScene *, const DevFrame *);

}  // namespace rt
