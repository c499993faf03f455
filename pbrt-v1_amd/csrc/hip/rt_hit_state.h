// rt_hit_state.h -- what the entry points that take (ray, RtHit) pairs in DEVICE memory share (rt_rays.hip: rt_hit_geometry_device; rt_bsdf.hip:
// rt_bsdf_device): the block size of their one-lane-per-record kernels, the rebuild of the traversal's hit state from a caller's records, and the
// refusals of the ray and hit pointers before anything is launched.
#pragma once
#include "rt_host.h"

#define RT_RAYS_BLOCK 256
#define RT_RAYS_MAX_N (1u << 30)

// The state the traversal leaves behind a closest-hit ray -- what make_vertex<true> / hit_point_uv / resolve_hit_material read -- from ray i of
// `rays` (RtRay: o.xyz d.x | d.yz mint maxt) and record i of `hits` (RtHit: prim, t, b1, b2).  Declares `Trav tv` and `const bool hit`: whether the
// record names a primitive of the scene (a record that names none counts as a miss).  A macro, not a function: through an inlined function the same
// statements reach the optimiser in another order, and hit_geometry_kernel then allocates 67 registers where it had 69 -- its code stays what it was.
#define RT_HIT_STATE(tv, hit, sc, rays, hits, i)                                                                                                       \
    const float4 a = RT_GPTR(const float4, rays)[size_t(2) * i], b = RT_GPTR(const float4, rays)[size_t(2) * i + 1];                                   \
    const float4 h = RT_GPTR(const float4, hits)[i];                                                                                                   \
    Trav tv;                                                                                                                                           \
    tv.o = mk3(a.x, a.y, a.z); tv.d = mk3(a.w, b.x, b.y); tv.mint = b.z;                                                                               \
    tv.hit_prim = __float_as_int(h.x); tv.maxt = h.y; tv.b1 = h.z; tv.b2 = h.w;     /* primitive.cpp:120: the accepted hit shortened the ray to t */   \
    tv.any = false;                                                                                                                                    \
    const bool hit = unsigned(tv.hit_prim) < (sc).n_tris

static inline unsigned blocks_for(uint32_t n) { return (n + RT_RAYS_BLOCK - 1) / RT_RAYS_BLOCK; }

// the refusals every call shares, before anything is launched (rt_host.h)
static inline int check_rays(const std::string &fn, const RtScene *s, const void *dev_rays, uint32_t n) {
    int rc;
    if ((rc = refuse_null(fn, s, "scene")) || (rc = refuse_null(fn, dev_rays, "ray pointer")) || (rc = refuse_unaligned16(fn, dev_rays, "dev_rays"))) return rc;
    return n > RT_RAYS_MAX_N ? fail(RT_EINVAL, fn + ": n = " + std::to_string(n) + " is above 2^30") : RT_OK;
}
// ... and a call's hit array
static inline int check_hits(const std::string &fn, const void *dev_hits) {
    if (int rc = refuse_null(fn, dev_hits, "hit pointer")) return rc;
    return refuse_unaligned16(fn, dev_hits, "dev_hits");
}
