// rt_ray_guard.h -- which caller-supplied rays may reach traversal (rt_rays.hip: rt_trace_closest_device / rt_trace_any_device).
// The rays of a frame come from camera_ray() and from the integrators, which never produce a non-finite origin or direction; rays a caller
// hands over in device memory can hold anything.  GridAccel's DDA turns ray values into voxel indices (rt_traverse.h grid_begin), so a ray is
// looked at BEFORE it is laid out for the trace kernel, and an unusable one is replaced by an empty ray: a miss.
//   unusable: a component of o or d that is not finite, d == (0, 0, 0), mint or maxt NaN
//   usable:   everything else -- maxt = +inf (geometry.h:204-217: a Ray's default), denormal directions, mint > maxt (an ordinary empty ray)
// The tests are on the bit patterns, so they hold whatever floating-point options the including unit is compiled with.
// No HIP header: tests/rays_host_test.cpp runs the predicate with a host compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_RAY_HD __host__ __device__ inline
#else
#define RT_RAY_HD inline
#endif

namespace rt {

RT_RAY_HD uint32_t ray_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, sizeof u); return u; }
RT_RAY_HD bool ray_finite(float f) { return (ray_bits(f) & 0x7f800000u) != 0x7f800000u; }
RT_RAY_HD bool ray_nan(float f) { return (ray_bits(f) & 0x7fffffffu) > 0x7f800000u; }
RT_RAY_HD bool ray_zero(float f) { return (ray_bits(f) & 0x7fffffffu) == 0u; }

// r = one RtRay record: o[3], d[3], mint, maxt
RT_RAY_HD bool ray_usable(float ox, float oy, float oz, float dx, float dy, float dz, float mint, float maxt) {
    const bool finite = ray_finite(ox) && ray_finite(oy) && ray_finite(oz) && ray_finite(dx) && ray_finite(dy) && ray_finite(dz);
    const bool zero_d = ray_zero(dx) && ray_zero(dy) && ray_zero(dz);
    return finite && !zero_d && !ray_nan(mint) && !ray_nan(maxt);
}
RT_RAY_HD bool ray_usable(const float *r) { return ray_usable(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]); }

// what an unusable ray becomes: mint > maxt, so every slab and primitive test fails; origin and direction are finite
#define RT_EMPTY_RAY_O 0.f, 0.f, 0.f
#define RT_EMPTY_RAY_D 0.f, 0.f, 1.f
#define RT_EMPTY_RAY_MINT 0.f
#define RT_EMPTY_RAY_MAXT (-1.f)

}  // namespace rt
