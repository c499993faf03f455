/* pbrt_hip.h -- C ABI of the MI355X (gfx950) implementation of pbrt-v1's
 * Scene::Render hot path.  Plain C: pointers, sizes and PODs only.
 *
 * The reference has NO foreign-function interface for this path: Scene::Render
 * (core/scene.cpp:32-88) is a non-virtual C++ loop that calls C++ plugin objects
 * created by extern "C" factories taking C++ types (core/dynload.cpp:112-260).  The
 * boundary below is therefore the one a maintainer would introduce between
 * RenderOptions::MakeScene (core/api.cpp:484-529) and Scene::Render
 * (core/api.cpp:475): everything MakeScene has produced is handed over as flat
 * arrays, the frame is rendered on the GPU, and the film comes back in the layout
 * ImageFilm keeps (film/image.cpp:57-65).  INTEGRATION.md shows the reference-side
 * stub.  Each entry point cites the reference interface it replaces.
 *
 * Conventions: every function returns 0 on success, a negative RT_E* code on
 * failure (no exceptions cross the boundary, like the reference);
 * rt_last_error() gives the message.  The caller owns all host buffers; the
 * library owns device memory.  One hipStream_t per handle; a handle may be used
 * from one thread at a time.  All arithmetic is IEEE float32 compiled without
 * FMA contraction so that results track the reference's SSE build.
 */
#ifndef PBRT_HIP_H
#define PBRT_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_EINVAL (-1)   /* bad argument / inconsistent description          */
#define RT_EDEVICE (-2)  /* HIP runtime error (no device, OOM, launch failed) */
#define RT_ESTATE (-3)   /* call out of order (e.g. render before film bind)  */
#define RT_ENOMEM (-4)   /* host memory exhausted while building the scene    */

typedef struct RtScene RtScene; /* opaque */

/* ---- materials: materials/matte.cpp:46-64, glass.cpp:46-63, mirror.cpp:42-55, plastic.cpp:47-69, uber.cpp:52-89 ---- */
/*      shinymetal.cpp:43-73, translucent.cpp:45-94 (both need the EXT kernels, as plastic and uber do)                       */
enum { RT_MAT_MATTE = 0, RT_MAT_MIRROR = 1, RT_MAT_GLASS = 2, RT_MAT_PLASTIC = 3, RT_MAT_UBER = 4, RT_MAT_SHINYMETAL = 5, RT_MAT_TRANSLUCENT = 6 };
typedef struct RtMaterial {
    int32_t type;
    float kd[3];   /* matte/plastic Kd  | mirror/glass Kr  (already .Clamp()'ed >= 0) */
    float kt[3];   /* glass Kt                                                   */
    float sigma;   /* matte: Oren-Nayar sigma in degrees, clamped [0,90]; 0 = Lambertian */
    float ior;     /* glass "index"                                              */
    float ks[3];   /* plastic Ks (.Clamp()'ed): Microfacet(Ks, FresnelDielectric(1.5, 1), Blinn(1/roughness)) */
    float roughness; /* plastic / uber "roughness"                                */
    float kr[3];   /* uber: op*Kr (SpecularReflection, FresnelDielectric(1.5, 1)).  For uber kd = op*Kd, ks = op*Ks,
                    * kt = 1 - op (SpecularTransmission(1 - op, 1, 1), present iff op != 1), ior = 1; lobe order T, D, G, R */
    /* shinymetal (types 5, 6 reuse the fields above; the layout of types 0-4 is unchanged): ks = Ks, kr = Kr (.Clamp()'ed), roughness.
     *   Lobes {Microfacet(1, FresnelConductor(FresnelApproxEta(Ks), 0), Blinn(1/roughness)), SpecularReflection(1,
     *   FresnelConductor(FresnelApproxEta(Kr), 0))}, both always present (shinymetal.cpp:52-61, reflection.cpp:40-56, :74-76).
     * translucent: kd = Kd, ks = Ks, kr = "reflect", kt = "transmit" (.Clamp()'ed), roughness.  Lobes, each present iff its colour
     *   is not black: Lambertian(reflect*Kd), BRDFToBTDF(Lambertian(transmit*Kd)), Microfacet(reflect*Ks, FresnelDielectric(1.5, 1),
     *   Blinn(1/roughness)), BRDFToBTDF(Microfacet(transmit*Ks, ...)) (translucent.cpp:53-80, reflection.cpp:63-73, :231-234).
     * include/pbrt_hip_material.h derives the etas, the products and the lobe flags exactly as rt_scene_create does. */
} RtMaterial;

/* ---- lights: lights/point.cpp:49-69, lights/area.cpp:28-105, lights/spot.cpp:54-79, lights/distant.cpp:51-62 ---- */
/*      RT_LIGHT_INFINITE: InfiniteAreaLight with a constant radiance (lights/infinite.cpp:66-131, :155-169; no radiance map).  It needs the EXT
 *      kernels.  It uses `color` (= L, Le of every ray that leaves the scene: whitted.cpp:52-58, directlighting.cpp:186-191, path.cpp:68-82,
 *      transport.cpp:184-185) and `n_samples`; every other field is ignored, the record keeps its size and offsets.  One estimate of it draws one
 *      RandomFloat() (infinite.cpp:104), so rt_render refuses it together with RT_STRATEGY_WEIGHTED.                      */
enum { RT_LIGHT_POINT = 0, RT_LIGHT_AREA = 1, RT_LIGHT_SPOT = 2, RT_LIGHT_DISTANT = 3, RT_LIGHT_INFINITE = 4 };
typedef struct RtLight {
    int32_t type;
    float color[3];      /* point/spot: I   area: Lemit   distant / infinite: L      */
    float pos[3];        /* point/spot light position (world, LightToWorld(0,0,0))  */
    int32_t n_samples;   /* Light::nSamples (light.h:39)                            */
    uint32_t first_tri;  /* area: range in light_tris (ShapeSet order, shape.h:112) */
    uint32_t n_tris;
    int32_t reverse_orientation; /* Triangle::Sample flips Ns by this only (trianglemesh.cpp:346) */
    int32_t flip_normal;         /* reverseOrientation ^ transformSwapsHandedness (shape.cpp:49)   */
    float dir[3];                /* distant: lightDir = Normalize(LightToWorld(from - to)) (distant.cpp:51-56) */
    float world_to_light[9];     /* spot: upper-left 3x3 of WorldToLight, row-major (Falloff, spot.cpp:68-79)   */
    float cos_total_width, cos_falloff_start;   /* spot.cpp:58-59 */
    int32_t quadric_plus1;       /* area light whose shape is a quadric (AreaLight keeps a CanIntersect shape as is,
                                  * area.cpp:38-39): 1 + index into RtSceneDesc::quadrics, n_tris = 0; 0 = triangle set */
} RtLight;

/* ---- camera: core/camera.cpp:50-70, cameras/perspective.cpp:51-82, orthographic.cpp:48-79, environment.cpp:47-61 ---- */
enum { RT_CAMERA_PERSPECTIVE = 0, RT_CAMERA_ORTHOGRAPHIC = 1, RT_CAMERA_ENVIRONMENT = 2 };
typedef struct RtCamera {
    float raster_to_camera[16]; /* row-major 4x4, as Matrix4x4::m (core/transform.h) */
    float camera_to_world[16];
    float lens_radius, focal_distance, hither, yon;
    float shutter_open, shutter_close;
    int32_t type;                /* RT_CAMERA_*                                                        */
    int32_t x_res, y_res;        /* film resolution (environment camera: theta/phi from imageY/imageX) */
} RtCamera;

/* ---- homogeneous medium: volumes/homogeneous.cpp:27-74 ---- */
typedef struct RtVolume {
    int32_t present;
    float world_to_volume[16];
    float p0[3], p1[3];
    float sigma_a[3], sigma_s[3], le[3];
    float g;
} RtVolume;

/* ---- density media: DensityRegion (core/volume.h:62-90, core/volume.cpp:137-153) with ExponentialDensity
 * (volumes/exponential.cpp:27-69) or VolumeGrid (volumes/volumegrid.cpp:27-110).  Kept out of RtVolume and
 * RtSceneDesc so that their byte images stay those of every scene without one: RtVolume still carries
 * world_to_volume, the extent p0 / p1, sigma_a, sigma_s, Le and g, and this record names how the density
 * Density(WorldToVolume(p)) scales them.  Handed over with rt_scene_set_density. ---- */
enum { RT_DENSITY_NONE = 0, RT_DENSITY_EXPONENTIAL = 1, RT_DENSITY_GRID = 2 };
typedef struct RtDensityRegion {
    int32_t kind;          /* RT_DENSITY_*                                                                     */
    float a, b;            /* exponential: a * expf(-b * Dot(Pobj - pMin, updir)) inside the extent             */
    float updir[3];        /* exponential: Normalize(updir), as the constructor stores it                       */
    int32_t nx, ny, nz;    /* grid: voxel counts, nx*ny*nz > 0 and below 2^31                                  */
    const float *density;  /* grid: [nz][ny][nx] (density[z*nx*ny + y*nx + x]); caller-owned, copied by the call */
} RtDensityRegion;

/* ---- accelerator parameters: accelerators/kdtree.cpp:489-498, grid.cpp:431-434 ---- */
enum { RT_ACCEL_KDTREE = 0, RT_ACCEL_GRID = 1 };
typedef struct RtAccelParams {
    int32_t kind;
    int32_t isect_cost, trav_cost, max_prims, max_depth; /* kd defaults 80, 1, 1, -1 */
    float empty_bonus;                                    /* kd default 0.5           */
    int32_t build_threads;                                /* 0 = auto; -1 = the checking form of the kd build: one thread, every node
                                                           * sorts its own edges as kdtree.cpp:246 does (same arrays, by test)  */
} RtAccelParams;

/* ---- quadrics: shapes/sphere.cpp:89-215, disk.cpp:51-130, cylinder.cpp:52-180, cone.cpp:41-186, paraboloid.cpp:44-190,
 * hyperboloid.cpp:46-240.  A quadric is ONE primitive of the accelerator
 * (Shape::CanIntersect, primitive.cpp:40-53).  In the primitive arrays below it occupies one slot whose tri_verts
 * hold its world bound as a degenerate triangle {pMin, pMax, pMin} (Shape::WorldBound shape.h:57-59) and whose
 * tri_flags has bit1 set; the k-th such slot is quadrics[k]. ---- */
enum { RT_QUADRIC_SPHERE = 0, RT_QUADRIC_DISK = 1, RT_QUADRIC_CYLINDER = 2, RT_QUADRIC_CONE = 3, RT_QUADRIC_PARABOLOID = 4, RT_QUADRIC_HYPERBOLOID = 5 };
typedef struct RtQuadric {
    int32_t type;
    float object_to_world[16], world_to_object[16]; /* Transform::m / ::mInv, row-major                      */
    float radius, zmin, zmax, theta_min, theta_max, phi_max; /* as the ctors store them (sphere.cpp:89-99, cylinder.cpp:52-59);
                                                              * disk (disk.cpp:51-59): zmin = height, zmax = innerRadius;
                                                              * cone (cone.cpp:41-48): zmin = 0, zmax = height; paraboloid (paraboloid.cpp:44-52);
                                                              * hyperboloid (hyperboloid.cpp:46-70): radius = rmax + the fields below */
    float p1[3], p2[3], a, c;                                /* hyperboloid: end points (after the ctor's swap) and the implicit form's a, c */
} RtQuadric;

/* ---- per-vertex shading data of triangle meshes: "uv" / "st", "N", "S" (shapes/trianglemesh.cpp:71-133 GetShadingGeometry,
 * :248-274 the (u,v)-dependent dpdu / dpdv of Triangle::Intersect, :315-328 GetUVs, checks of the factory :350-406).  A triangle
 * whose mesh has any of them refers to one record.  n and s are object-space (the mesh keeps them so, :155-164) and go through
 * the mesh's ObjectToWorld at shading time: xform indexes RtSceneDesc::xforms. ---- */
enum { RT_SHADING_UV = 1, RT_SHADING_N = 2, RT_SHADING_S = 4 };
typedef struct RtTriShading {
    uint32_t flags;            /* RT_SHADING_*                                                               */
    uint32_t xform;
    float uv[6];               /* uvs[3][2] as GetUVs returns them (the defaults (0,0) (1,0) (1,1) without "uv") */
    float n[9];                /* normals of the three vertices, object space                                */
    float s[9];                /* tangents of the three vertices, object space                               */
} RtTriShading;

/* Scene description = what MakeScene hands to Scene::Scene (core/scene.cpp:100-119),
 * flattened.  Triangles are in the order KdTreeAccel's FullyRefine produces
 * (kdtree.cpp:146-148: per mesh, last triangle first). Vertices are world space
 * (trianglemesh.cpp:166-168). */
typedef struct RtSceneDesc {
    uint32_t n_tris;
    const float *tri_verts;       /* [n_tris][9]  p1 p2 p3                                   */
    const uint16_t *tri_material; /* [n_tris] index into materials                             */
    const int32_t *tri_light;     /* [n_tris] area-light index (GetAreaLight) or -1           */
    const uint8_t *tri_flags;     /* [n_tris] bit0 = flip geometric normal (shape.cpp:49-50), bit1 = quadric slot */
    uint32_t n_materials;
    const RtMaterial *materials;
    uint32_t n_lights;
    const RtLight *lights;
    uint32_t n_light_tris;
    const float *light_tris;      /* [n_light_tris][9] emitter triangles, ShapeSet order       */
    RtCamera camera;
    RtVolume volume;
    RtAccelParams accel;
    uint32_t n_quadrics;          /* may be 0 / NULL                                           */
    const RtQuadric *quadrics;
    const int32_t *tri_shading;   /* [n_tris] index into shading[] or -1; NULL when no mesh has uv / N / S */
    uint32_t n_shading;
    const RtTriShading *shading;
    uint32_t n_xforms;
    const float *xforms;          /* [n_xforms][32]: Transform::m then ::mInv of a mesh's ObjectToWorld, row-major */
} RtSceneDesc;

/* ---- per-frame description ---- */
enum { RT_INTEGRATOR_WHITTED = 0, RT_INTEGRATOR_DIRECT = 1, RT_INTEGRATOR_PATH = 2, RT_INTEGRATOR_BIDIRECTIONAL = 3 };
/* RT_INTEGRATOR_BIDIRECTIONAL: BidirIntegrator (integrators/bidirectional.cpp:80-131), eye and light sub-paths of at most 4 vertices each.  Its factory
 * reads no parameter (:211-213): max_depth and strategy are ignored.  rt_render refuses it in a participating medium and in a scene without lights. */
/* Values from 0x100 on are integrators that estimate no radiance (value 4 stays an unknown integrator).
 * RT_INTEGRATOR_DEBUG: DebugIntegrator (integrators/debug.cpp:61-133): the film's three channels are hit data of the camera ray, one RT_DEBUG_* code
 * per channel, carried in `strategy` as red | green << 8 | blue << 16; max_depth is ignored.  A code above RT_DEBUG_HIT is refused (RT_EINVAL).  alpha is 1
 * for every sample, misses included (:69).  It takes no integrator samples, renders a scene without lights, and in a medium Scene::Li's T * Lo + Lv
 * applies to it as to the others (scene.cpp:120-126). */
enum { RT_INTEGRATOR_DEBUG = 0x100 };
/* ... in the order of the reference's DebugVariable (debug.cpp:33-44): dg.u, dg.v, |x|, |y|, |z| of the geometric normal isect.dg.nn and of the shading
 * normal bsdf->dgShading.nn, the constants, and 1 where the camera ray hit something.  A miss leaves every hit-dependent channel 0. */
enum { RT_DEBUG_U = 0, RT_DEBUG_V = 1, RT_DEBUG_NX = 2, RT_DEBUG_NY = 3, RT_DEBUG_NZ = 4, RT_DEBUG_SNX = 5, RT_DEBUG_SNY = 6, RT_DEBUG_SNZ = 7,
       RT_DEBUG_ONE = 8, RT_DEBUG_ZERO = 9, RT_DEBUG_HIT = 10 };
enum { RT_STRATEGY_ALL = 0, RT_STRATEGY_ONE = 1, RT_STRATEGY_WEIGHTED = 2 };
/* RT_STRATEGY_WEIGHTED: WeightedSampleOneLight (transport.cpp:71-122), a recurrence over every shading point of the frame in program order.
 * rt_render accepts it on one shard (shard_count == 1) with at most 2048 lights of any mix (round 5: emitters of several triangles, which draw one
 * random number per estimate -- ShapeSet::Sample, shape.h:115-121 -- next to lights that draw none: the survey then keeps one estimate per possible
 * position of that draw in the sample's stream).
 * Such a frame is five launches (RtRenderStats.weighted_ms); rt_render waits on the stream once in the middle of it, for the number of shading
 * points that sizes the survey's tables (every other frame is asynchronous from the first launch on).  That wait is also the one place where
 * rt_render can fail AFTER launching work (2^32 or more shading points, no memory for the survey's tables): the film and the sample buffer are
 * untouched then (the count pass writes neither), rt_last_render_stats / rt_samples_read report "no frame".  In a participating medium the
 * strategy needs lights that draw no random numbers at all (delta lights, single-triangle / quadric emitters): the medium makes an estimate's
 * draws depend on occlusion, and an emitter of several triangles would draw its triangle from a different place in the stream than the
 * survey did -- refused.
 * Cost and limit with lights of mixed RNG use: a camera sample with P shading points keeps P (1 + 2 (nLights - nD)) + nD P (P + 1) floats of survey records
 * (nD = emitters of several triangles) -- QUADRATIC in P, i.e. in the depth of the specular recursion -- capped at 2^32 floats per frame (refused after the
 * count pass, as above), and the recurrence itself is sequential by definition: one lane walks every shading point of the frame in program order (~0.45 us per
 * point on MI355X; the reference pays the same dependence on one core).  High maxdepth with many such emitters is therefore slow or refused, never wrong. */
enum { RT_VOLUME_NONE = 0, RT_VOLUME_EMISSION = 1, RT_VOLUME_SINGLE = 2 };
enum { RT_SAMPLER_STRATIFIED = 0, RT_SAMPLER_LOWDISCREPANCY = 1, RT_SAMPLER_RANDOM = 2 };

typedef struct RtRenderDesc {
    /* SurfaceIntegrator: integrators/{whitted,directlighting,path,bidirectional,debug}.cpp factories (debug: strategy = the three channel codes) */
    int32_t integrator, max_depth, strategy;
    /* VolumeIntegrator: integrators/{emission,single}.cpp */
    int32_t volume_integrator;
    float step_size;
    /* Sampler: samplers/{stratified,lowdiscrepancy,random}.cpp */
    int32_t sampler, x_samples, y_samples, jitter, pixel_samples;
    uint32_t seed;            /* counter-RNG seed (see oracle/ref/keyed_rng.cpp)         */
    /* Film: film/image.cpp:69-101,148-156 */
    int32_t x_res, y_res;
    int32_t x_pixel_start, y_pixel_start, x_pixel_count, y_pixel_count; /* crop window in pixels */
    int32_t x_start, x_end, y_start, y_end;  /* sample extent (GetSampleExtent)               */
    float filter_x_width, filter_y_width;
    float filter_table[256];  /* 16x16, image.cpp:89-101                                   */
    /* Work partition (reference: cropwindow processes, image.cpp:220-228): pixels of the
     * sample extent, in scanline order, are grouped into tiles of tile_pixels consecutive
     * pixels; this call renders tiles t with t % shard_count == shard_index.
     * tile_pixels < 0 selects 2-D tiles: -tile_pixels = tile_w | tile_h << 16, blocks of tile_w x tile_h pixels of the sample extent
     * numbered row by row (border blocks are clipped).  A rank then owns compact pieces of the film: its film gather touches only the
     * blocks around them, and the partial films can be merged row-wise (bench.py: reduce-scatter + per-rank resolve).
     * Border blocks are whole blocks whose pixels outside the extent are fetched and dropped (a lane idles for about a ray's time per dropped
     * item): pick sizes that pad the extent little (pbrt-v1_amd ParsedScene.set_shard(fit=True)).  With shard_count == 1 the tiles partition
     * nothing and a frame without a medium is rendered in scanline order whatever is passed here. */
    int32_t shard_index, shard_count, tile_pixels;
} RtRenderDesc;

/* per-frame counters (reference: StatsCounters, core/util.cpp:186-285) */
typedef struct RtCounters {
    uint64_t camera_rays;     /* "Camera Rays Traced" scene.cpp:80            */
    uint64_t closest_rays;    /* every Scene::Intersect  (camera+bounce+MIS)  */
    uint64_t any_rays;        /* every Scene::IntersectP ("shadow rays", light.cpp:32) */
    uint64_t nodes_visited;   /* kd nodes / grid voxels touched               */
    uint64_t leaf_refs;       /* leaf primitive references read               */
    uint64_t tri_tests;       /* Triangle::Intersect(P) calls, trianglemesh.cpp:217 */
    uint64_t bad_samples;     /* NaN/negative/inf radiance, scene.cpp:60-74   */
    uint64_t stack_overflows; /* traversal stack entries spilled beyond LDS   */
} RtCounters;

typedef struct RtRay { float o[3], d[3], mint, maxt; } RtRay;             /* geometry.h:204-217 */
typedef struct RtHit { int32_t prim; float t, b1, b2; } RtHit;            /* prim < 0 : miss      */
typedef struct RtAccelInfo {
    uint32_t n_nodes, n_leaf_refs, max_depth, n_tris; /* grid: n_nodes = voxels, n_leaf_refs = voxel list entries */
    float bounds[6];
    double build_seconds;
    int32_t kind;                                       /* RT_ACCEL_KDTREE / RT_ACCEL_GRID */
    int32_t grid_nvoxels[3];                            /* GridAccel::NVoxels (grid.cpp:146-152) */
    float grid_width[3], grid_inv_width[3];             /* GridAccel::Width / InvWidth (grid.cpp:154-158) */
} RtAccelInfo;

const char *rt_last_error(void);
int rt_device_count(int *count);

/* Build accelerator (KdTreeAccel ctor kdtree.cpp:141-190 / GridAccel ctor grid.cpp:122-210),
 * upload everything.  device < 0 = current device. */
int rt_scene_create(const RtSceneDesc *desc, int device, RtScene **out);
/* The same with an accelerator built elsewhere -- by rt_accel_build, or copied out of another process' scene (rt_scene_accel_info /
 * rt_scene_accel_copy): the ranks of one node build the tree once (reference: every cropwindow process of image.cpp:220-228 builds its
 * own, kdtree.cpp:141-312).  Arrays as rt_accel_copy writes them; they are checked (every index in range) and copied. */
typedef struct RtPrebuiltAccel {
    int32_t kind;                       /* RT_ACCEL_KDTREE / RT_ACCEL_GRID, must equal desc->accel.kind */
    uint32_t n_nodes, n_leaf_refs, max_depth;
    const uint32_t *nodes;              /* [n_nodes][2] */
    const uint32_t *leaf_refs;          /* [n_leaf_refs] */
    float bounds[6];
    int32_t grid_nvoxels[3]; float grid_width[3], grid_inv_width[3];   /* grid only (RtAccelInfo) */
} RtPrebuiltAccel;
int rt_scene_create_prebuilt(const RtSceneDesc *desc, int device, const RtPrebuiltAccel *accel, RtScene **out);
/* Make the scene's medium a DensityRegion: what pbrtVolume (core/api.cpp:403-409) keeps when MakeVolumeRegion
 * (core/dynload.cpp:365-375) returns an ExponentialDensity or a VolumeGrid.  Call once, after rt_scene_create or
 * rt_scene_create_prebuilt and before the first rt_render; the scene's RtVolume (desc->volume) must be present and
 * supplies the transform, the extent and the constants.  A grid is copied to device memory (the library owns it;
 * `region->density` may be freed on return).  Frames of such a scene run the EXT kernels, whose optical depth is
 * DensityRegion::Tau's ray march (volume.cpp:137-153) at the reference's three call sites: .5f * stepSize per march step
 * (emission.cpp:82-83, single.cpp:83-84), 4.f * stepSize for Scene::Transmittance (scene.cpp:127-129) and stepSize
 * with the sampler's tau value for Scene::Li's T (scene.cpp:120-126).
 * Returns RT_EINVAL (null argument, unknown kind, no medium in the scene, grid counts not positive or
 * nx*ny*nz >= 2^31, null grid), RT_ESTATE (called twice, or after rt_render), RT_EDEVICE (upload failed);
 * rt_last_error() says which. */
int rt_scene_set_density(RtScene *s, const RtDensityRegion *region);
/* The spot lights' LightToWorld (upper-left 3x3, row-major), 9 floats per light of the scene in the order of RtSceneDesc::lights; entries of other
 * lights are not read.  The bidirectional integrator starts its light path with SpotLight::Sample_L(scene, ...) (spot.cpp:87-95), which multiplies
 * by this matrix -- the product CreateLight formed, not the inverse of WorldToLight: the two differ in their last bits, and with them hit / miss and
 * black / not black decisions further down the path.  Optional: without it the device inverts RtLight::world_to_light.  Call once, after
 * rt_scene_create and before the first rt_render.  RT_EINVAL (null argument, n_lights differs from the scene's, an entry not finite), RT_ESTATE
 * (after rt_render), RT_EDEVICE. */
int rt_scene_set_light_transforms(RtScene *s, const float *light_to_world, uint32_t n_lights);
/* Textured material parameters (include/pbrt_hip_texture.h has the records, the limits and the evaluation): what MakeMaterial keeps when
 * TextureParams::GetSpectrumTexture / GetFloatTexture (core/paramset.cpp:434-465) return something other than a ConstantTexture.  Call once,
 * after rt_scene_create or rt_scene_create_prebuilt and before the first rt_render.  `nodes` is a flat table of n_nodes texture nodes whose
 * children precede them; `mats` has one record per material of the scene (n_mats == RtSceneDesc.n_materials): the raw parameters and, per
 * parameter slot, the node that supplies it at every hit or -1.  A material with a textured slot is resolved per hit on the device (the
 * clamps, Oren-Nayar's A and B, the Blinn exponent, the conductor etas, the products and the lobes present), from `mats[i].raw` with the
 * textured slots replaced; a material without one keeps what rt_scene_create made of RtSceneDesc.materials[i].  Frames of such a scene run
 * the EXT kernels.  Both tables are copied.
 * Returns RT_EINVAL (null argument, n_nodes == 0 or above RT_TEX_MAX_NODES, n_mats != the scene's materials, an unknown kind or mapping, a
 * child index that is not below its node -- which is how a cycle shows --, a missing child, a child or a slot of the wrong value type, a
 * material type that differs from the scene's, a parameter graph of more than RT_TEX_MAX_PROGRAM nodes or one that needs more than
 * RT_TEX_MAX_STACK values at once, more than 65534 materials), RT_ESTATE (called twice, or after rt_render), RT_EDEVICE (upload failed);
 * rt_last_error() says which.  Nothing is launched. */
struct RtTexture; struct RtMaterialTextures;
int rt_scene_set_textures(RtScene *s, const struct RtTexture *nodes, uint32_t n_nodes, const struct RtMaterialTextures *mats, uint32_t n_mats);
int rt_scene_destroy(RtScene *s);
int rt_scene_set_stream(RtScene *s, void *hip_stream);
int rt_scene_accel_info(const RtScene *s, RtAccelInfo *info);
/* copy the flattened kd-tree back (tests / oracle traverse the same tree):
 * nodes = [n_nodes][2] u32, leaf_refs = [n_leaf_refs] u32 */
int rt_scene_accel_copy(const RtScene *s, uint32_t *nodes, uint32_t *leaf_refs);

/* The accelerator build alone, host-only (no device needed): KdTreeAccel's constructor,
 * accelerators/kdtree.cpp:141-312.  rt_scene_create runs exactly this. */
/* Either accelerator, host-only: kd-tree as above, or GridAccel's constructor in its "refineimmediately" form
 * (accelerators/grid.cpp:122-210).  nodes = [n_nodes][2] u32: kd nodes, or per-voxel {offset, count}. */
typedef struct RtKdTree RtAccel;
int rt_accel_build(const float *tri_verts, uint32_t n_tris, const RtAccelParams *params, RtAccel **out);
int rt_accel_info(const RtAccel *t, RtAccelInfo *info);
int rt_accel_copy(const RtAccel *t, uint32_t *nodes, uint32_t *leaf_refs);
/* Host only, for tests of the host logic: the leaves of a kd-tree as rt_scene_create lays them out for the flat traversal -- ONE 48-byte record per primitive, `stride` float4
 * units apart, in the order the depth-first leaf walk first meets the primitives (`slot_prim[slot]` = primitive), and per leaf node its primitives as ENTRIES = position | flags
 * (the reference keeps index lists, accelerators/kdtree.cpp:55-64): word 0 = position of the first primitive's record << 2 | 3, word 1 = bit 31 "more follow",
 * bit 30 "the others' entries are a list" | the second entry (leaf of two) or HALF the index of the list in `entries`, whose items carry the same two flags; an empty leaf's first entry
 * is 0xffffffff.  `runs` != 0: every leaf owns a run of consecutive records, word 1 = bit 31 (more than one) | the count (what scenes of a few thousand references get); `copies` != 0:
 * one record per leaf reference (measurements).  Call with null arrays for the sizes (tnodes [n_nodes][2], slot_prim [n_slots], entries [n_entries]). */
typedef struct RtLeafLayoutInfo { uint64_t n_nodes, n_slots, n_entries; uint32_t stride, pad; } RtLeafLayoutInfo;
int rt_accel_leaf_layout(const RtAccel *t, int runs, int copies, uint32_t *tnodes, uint32_t *slot_prim, uint32_t *entries, RtLeafLayoutInfo *info);
int rt_accel_destroy(RtAccel *t);
typedef struct RtKdTree RtKdTree;
int rt_kdtree_build(const float *tri_verts, uint32_t n_tris, const RtAccelParams *params, RtKdTree **out);
int rt_kdtree_info(const RtKdTree *t, RtAccelInfo *info);
int rt_kdtree_copy(const RtKdTree *t, uint32_t *nodes, uint32_t *leaf_refs);
int rt_kdtree_destroy(RtKdTree *t);

/* Unit entry points (parity of one stage in isolation) */
/* Camera::GenerateRay for `count` samples starting at camera-sample index `first`
 * (perspective.cpp:51-82 + the sampler's image/lens positions) */
int rt_camera_rays(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, RtRay *rays_out);
/* Scene::Intersect (kdtree.cpp:313-403 + trianglemesh.cpp:213-278) */
int rt_trace_closest(RtScene *s, const RtRay *rays, uint32_t n, RtHit *hits_out);
/* Scene::IntersectP (kdtree.cpp:404-488 + trianglemesh.cpp:279-314); occluded_out[i] in {0,1} */
int rt_trace_any(RtScene *s, const RtRay *rays, uint32_t n, uint8_t *occluded_out);

/* ---- Rays and hits in DEVICE memory (additive; the three entry points above are unchanged) ----
 * For a caller whose rays are already on the GPU (a tensor of origins and directions: a G-buffer, a custom camera model, a collision query)
 * and who wants the answers there too.  Contract of all four calls:
 *  - Asynchronous on the scene's stream (rt_scene_set_stream / rt_scene_get_stream).  They never copy to or from the host and never wait for
 *    the stream, with two exceptions that happen at most once per size / scene: the workspace (two float4 planes of n rays; n more float4s for
 *    rt_trace_any_device) grows only when n exceeds the largest n seen so far on that scene -- a call with a smaller or equal n allocates
 *    nothing -- and growing waits for the work queued on the stream before the old block goes; and the first rt_hit_geometry_device call that
 *    asks for `uv` on a scene with a mesh that has "uv" uploads those uvs (as the first debug frame of rt_render does).  The stream the scene
 *    creates itself is non-blocking: it is NOT ordered against the null stream or anybody else's -- order it with events, or hand the scene
 *    your stream.
 *  - The queue counters of the trace launch are written by a kernel (the host-array entry points upload them from the host).
 *  - dev_rays is RtRay[n] (32 bytes each: o, d, mint, maxt -- a contiguous float32 [n][8] array), dev_hits is RtHit[n] (16 bytes); both must be
 *    16-byte aligned.
 *  - The trace is the kernel of rt_trace_closest / rt_trace_any (rt::pipe_trace_kernel) and the caller's dev_hits is its hit plane: for the same
 *    rays the hits are those of rt_trace_closest bit for bit; a miss is prim = -1, t = b1 = b2 = 0.  rt_set_counting is honoured: the counting
 *    twin when enabled (nodes_visited, leaf_refs, tri_tests advance), the timed kernel otherwise; the hits are the same either way.
 *  - Refused before any launch with RT_EINVAL (rt_last_error says which): a null scene, ray or output pointer; an RtHitGeometry whose fields
 *    are all null; a ray or hit pointer that is not 16-byte aligned; n above 2^30.  n == 0 is RT_OK and launches nothing.
 *  - Unusable rays never reach traversal (GridAccel's DDA would turn their values into voxel indices).  A ray is unusable when a component of
 *    o or d is not finite, when d is (0, 0, 0), or when mint or maxt is NaN; the kernel that lays the rays out for the trace kernel replaces
 *    it by an empty ray, i.e. it misses.  maxt = +inf is an ordinary ray (geometry.h:204-217), and so is mint > maxt (it is empty by itself).
 *    The predicate is rt::ray_usable in pbrt-v1_amd/csrc/hip/rt_ray_guard.h (no HIP header; tested on the host). */
/* Scene::Intersect (core/scene.h:60-62 -> Primitive::Intersect, kdtree.cpp:313-403 / grid.cpp:224-286) for n rays */
int rt_trace_closest_device(RtScene *s, const RtRay *dev_rays, uint32_t n, RtHit *dev_hits);
/* Scene::IntersectP (core/scene.h:63-65, kdtree.cpp:404-488 / grid.cpp:331-390); dev_occluded[i] in {0,1}, any alignment */
int rt_trace_any_device(RtScene *s, const RtRay *dev_rays, uint32_t n, uint8_t *dev_occluded);
/* What Scene::Intersect leaves in Intersection (core/primitive.h:107-121): its DifferentialGeometry dg (core/shape.h:34-51: p, nn, u, v), the
 * shading normal of the BSDF Intersection::GetBSDF builds (primitive.cpp:160-167: Shape::GetShadingGeometry + Material::GetBSDF, bsdf->dgShading.nn),
 * the primitive's material and GetAreaLight() (primitive.cpp:155-158).  Computed from (ray, hit) with the render kernels' code: triangles with
 * and without per-vertex uv / N / S, ReverseOrientation, handedness-swapping transforms and the six quadrics.  dev_hits are the records
 * rt_trace_closest_device wrote for dev_rays (a record whose prim is no primitive of the scene counts as a miss).  Only the fields whose pointer
 * is not NULL are computed and stored.  A miss yields zeros in every float field and -1 in both index fields. */
typedef struct RtHitGeometry {      /* device pointers, each may be NULL (field not wanted) */
    float   *p;          /* [n][3] dg.p                                                   */
    float   *ng;         /* [n][3] dg.nn: geometric normal, orientation flips applied     */
    float   *ns;         /* [n][3] shading normal (bsdf->dgShading.nn)                    */
    float   *uv;         /* [n][2] dg.u, dg.v                                             */
    int32_t *material;   /* [n] index into RtSceneDesc.materials, -1 on a miss            */
    int32_t *light;      /* [n] area-light index of the primitive, -1 if none or a miss   */
} RtHitGeometry;
int rt_hit_geometry_device(RtScene *s, const RtRay *dev_rays, const RtHit *dev_hits, uint32_t n, const RtHitGeometry *out);
/* What an integrator asks of a hit: Intersection::GetBSDF (primitive.cpp:135-141 -> Shape::GetShadingGeometry + Material::GetBSDF), then BSDF::f,
 * BSDF::Pdf, BSDF::Sample_f and BSDF::NumComponents (core/reflection.cpp, core/reflection.h:382-388), and Intersection::Le (primitive.cpp:142-145).
 * One query per (ray, hit) pair; computed with the render kernels' code (rt_shade.h, rt_texture.h), so a lobe is one call.
 *  - Outgoing direction.  wo = -d of ray i, as every integrator forms it (whitted.cpp:69, directlighting.cpp:100, path.cpp:98).  d must be of unit
 *    length; the library does not renormalise.  dev_hits are the records rt_trace_closest_device wrote for dev_rays.
 *  - The BSDF is the one Intersection::GetBSDF builds at that hit, unchanged: the shading frame of the render kernels (per-vertex N / S,
 *    ReverseOrientation, handedness-swapping transforms, the quadrics' dpdu; BSDF ctor reflection.cpp:471-479), the geometric normal that decides
 *    between BRDFs and BTDFs (:483-488), the scene's material -- resolved from its textures at the hit where it has textured parameters -- and the
 *    lobes in the order the seven materials add them (matte.cpp, plastic.cpp, uber.cpp:62-87, shinymetal.cpp:60-61, translucent.cpp:59-78,
 *    mirror.cpp:51-53, glass.cpp:56-61).
 *  - A miss, or a record whose prim is no primitive of the scene, gives zeros in every float output, 0 in n_components and 0 in s_type.
 *  - A sample with pdf == 0 gives s_wi = s_f = 0, s_pdf = 0 and s_type = 0, as the reference returns (reflection.cpp:407-411, :428-431).
 *  - Asynchronous on the scene's stream; no copy from the device and no wait.  The only workspace is for scenes with textured materials: one resolved
 *    record per resident thread, the pool the frames use -- its size does not depend on n, and as for rt_radiance_device it grows (waiting for the
 *    stream once) only when no frame or query before has made it.  A kernel lane beyond the resident threads takes its next query a grid further.
 *  - It is not a frame and it traces nothing: the film, the sample buffer, the counters and the record of the last launch are untouched, and a later
 *    rt_render gives the film it gave before.
 *  - Refused before any launch with RT_EINVAL (rt_last_error says which): a null scene; with n > 0 a null ray, hit or query pointer, a query with no
 *    output, f or pdf wanted without wi, an s_* output wanted without u, ray or hit pointers that are not 16-byte aligned; n above 2^30.  n == 0 is
 *    RT_OK and launches nothing. */
/* BxDFType bits, core/reflection.h:52-68 */
enum { RT_BSDF_REFLECTION = 1, RT_BSDF_TRANSMISSION = 2, RT_BSDF_DIFFUSE = 4, RT_BSDF_GLOSSY = 8, RT_BSDF_SPECULAR = 16, RT_BSDF_ALL = 31 };
typedef struct RtBsdfQuery {   /* device pointers; any output may be NULL (not wanted) */
    const float *wi;           /* in  [n][3] world directions, for f / pdf; may be NULL if neither is wanted   */
    const float *u;            /* in  [n][3] u1, u2, u3 of BSDF::Sample_f; may be NULL if no s_* is wanted      */
    const int32_t *flags;      /* in  [n] BxDFType mask per query, or NULL: RT_BSDF_ALL for all                 */
    float   *f;                /* out [n][3] BSDF::f(wo, wi, flags)          reflection.cpp:480-494             */
    float   *pdf;              /* out [n]    BSDF::Pdf(wo, wi, flags)        :458-470                           */
    float   *s_wi, *s_f;       /* out [n][3] BSDF::Sample_f(wo, &wi, u1, u2, u3, &pdf, flags, &type) :402-457   */
    float   *s_pdf;            /* out [n]                                                                       */
    int32_t *s_type;           /* out [n]    sampledType, 0 when pdf == 0                                       */
    int32_t *n_components;     /* out [n]    BSDF::NumComponents(flags)      reflection.h:382-388               */
    float   *le;               /* out [n][3] Intersection::Le(wo) (primitive.cpp:142-145, area.h: Lemit if Dot(dg.nn, wo) > 0) */
} RtBsdfQuery;
int rt_bsdf_device(RtScene *s, const RtRay *dev_rays, const RtHit *dev_hits, uint32_t n, const RtBsdfQuery *q);
/* What EstimateDirect asks of a light (core/transport.cpp:123-193): Light::Sample_L, Light::Pdf, Light::Le and Light::IsDeltaLight, one query per
 * (point, light) pair, computed with the render kernels' code (rt_shade.h).  With it a caller can write next-event estimation:
 * light -> rt_trace_any_device(s_ray) -> rt_bsdf_device(f at wi = s_wi) -> f * s_L * |s_wi . ns| / s_pdf.
 *  - Sampling forms.  With `nrm` the call is Sample_L(p, n, u1, u2, &wi, &pdf, &vis) and Pdf(p, n, wi), the forms EstimateDirect uses: area.cpp:58-72,
 *    infinite.cpp:96-120 (a cosine-weighted direction about +-n), and for point, spot and distant lights the light.h:58-66 defaults, which drop n.
 *    With nrm == NULL it is Sample_L(p, u1, u2, &wi, &pdf, &vis) and Pdf(p, wi): area.cpp:73-82, :93-95; infinite.cpp:121-131 (the uniform sphere,
 *    no draw).  Whitted's Sample_L(p, &wi, &vis) and the emission form Sample_L(scene, u1..u4, &ray, &pdf) are not offered.
 *  - The outputs are the reference's, unchanged: a sample with pdf == 0 or black L still returns its wi and ray, as Sample_L does; the caller applies
 *    EstimateDirect's own test (transport.cpp:153).
 *  - Delta lights (point.cpp:61-69, spot.cpp:79-86, distant.cpp:66-73) return s_pdf = 1 and pdf = 0 and ignore u.
 *  - Shadow ray.  s_ray is VisibilityTester::r (light.h:78-83): SetSegment, {p, ps - p, RAY_EPSILON, 1 - RAY_EPSILON}, for point, spot and area
 *    lights; SetRay, {p, wi, RAY_EPSILON, inf}, for distant and infinite lights.  It can be handed to rt_trace_any_device as it is.  The transmittance
 *    of a medium along s_ray (VisibilityTester::Transmittance, light.cpp) is rt_medium_device's `tr` of that ray, below.
 *  - Random draws.  Two places draw one RandomFloat() each: ShapeSet::Sample (shape.h:115-121; emitters of more than one triangle) and the infinite
 *    light's z flip (infinite.cpp:104).  They come from the keyed stream of camera sample `key` under `seed` (draw c of sample k is
 *    pcg(c + pcg(k + seed * 0x9E3779B9)), as a frame derives it), starting at the supplied counter; s_draws says how far the stream moved.  A caller who
 *    passes a camera sample's index and the counter the frame's integrator would be at reproduces the frame's draw.
 *  - Le is Light::Le(ray(p, wi)) of that light alone: the infinite light's L (infinite.cpp:83-95), black for every other (light.cpp).
 *  - A `light` outside [0, n_lights) gives zeros in every output.
 *  - The light's type is read per query: a wavefront whose queries name lights of several types runs each type's code in turn, so callers do best to
 *    group queries by light.
 *  - Asynchronous on the scene's stream; no host copy, no wait, no workspace.  It is not a frame and it traces nothing: the film, the sample buffer,
 *    the counters, rt_last_render_stats and rt_last_render_ms are untouched.
 *  - Refused before any launch with RT_EINVAL (rt_last_error names the function and the field): a null scene; with n > 0 a null query, null p or null
 *    light, a query with no output wanted, an s_* output wanted without u, pdf or le wanted without wi, an s_ray that is not 16-byte aligned; n above
 *    2^30.  n == 0 is RT_OK and launches nothing. */
typedef struct RtLightQuery {      /* device pointers unless said otherwise */
    const float    *p;        /* in  [n][3] reference points                                              */
    const float    *nrm;      /* in  [n][3] normal at p, or NULL: the forms without a normal              */
    const int32_t  *light;    /* in  [n]    index into RtSceneDesc.lights (scene order)                   */
    const float    *u;        /* in  [n][2] u1, u2; may be NULL if no s_* output is wanted                */
    const uint32_t *rng;      /* in  [n][2] key, first counter of the keyed stream; NULL: key = i, 0      */
    const float    *wi;       /* in  [n][3] unit directions for pdf / le; may be NULL if neither wanted   */
    uint32_t        seed;     /* host value, the meaning of RtRenderDesc.seed                             */
    float   *s_wi, *s_L;      /* out [n][3] Light::Sample_L(p, n, u1, u2, &wi, &pdf, &vis) / (p, u1, u2, ...) */
    float   *s_pdf;           /* out [n]                                                                  */
    RtRay   *s_ray;           /* out [n]    VisibilityTester::r (light.h:78-83): SetSegment or SetRay; 16-byte aligned */
    int32_t *s_draws;         /* out [n]    RandomFloat() calls the sample made (0 or 1)                  */
    float   *pdf;             /* out [n]    Light::Pdf(p, n, wi) / Pdf(p, wi)                             */
    float   *le;              /* out [n][3] Light::Le(ray(p, wi)) of that light                           */
    int32_t *is_delta;        /* out [n]    Light::IsDeltaLight()                                         */
} RtLightQuery;
int rt_light_device(RtScene *s, uint32_t n, const RtLightQuery *q);
/* What an integrator asks of the participating medium (scene->volumeRegion) and of the volume integrator, one query per row, computed with the
 * render kernels' code (rt_integrate.h).  With it a caller's next-event estimation holds in a scene with a Volume:
 * ... * s_L * tr(s_ray) ..., and Scene::Li's T * Lo + Lv (core/scene.cpp:120-126) can be had factor by factor.
 *  - Point outputs.  VolumeRegion::sigma_a / sigma_s / sigma_t / Lve / p at p (with w, wp for the phase function).  A homogeneous region
 *    (homogeneous.cpp:47-62) tests extent.Inside(WorldToVolume(p)) for all five; a density region (core/volume.h:62-90 with exponential.cpp /
 *    volumegrid.cpp Density) scales the constants by Density(WorldToVolume(p)), and its p() is PhaseHG without an inside test.
 *  - hit, t01.  VolumeRegion::IntersectP(ray, &t0, &t1); t01 is 0, 0 where hit is 0.
 *  - tau.  VolumeRegion::Tau(ray, step_size, u[i]): homogeneous.cpp:63-67 (step and offset ignored), core/volume.cpp:137-153.
 *  - tr.  With `u` it is VolumeIntegrator::Transmittance(scene, ray, sample, alpha) with a sample: Exp(-Tau(ray, step_size, u[i])), no draw.  With
 *    u == NULL it is Scene::Transmittance(ray) (scene.cpp:127-129; emission.cpp:47-59, single.cpp:48-56): step 4.f * step_size and, as offset, one
 *    RandomFloat() of the keyed stream at the caller's counter -- drawn for a homogeneous region too, which ignores it.
 *  - lv.  EmissionIntegrator::Li(scene, ray, sample, alpha) (emission.cpp:60-95) with a sample whose scatter value is u_scatter[i]: one RandomFloat()
 *    per step for the step's Tau (at .5f * step_size), the Russian-roulette draw when Tr.y() < 1e-3, all from the keyed stream at the caller's
 *    counter.  The ray is taken as given (a frame hands over camera rays cut at their hits).  SingleScattering::Li is not offered: its shadow rays
 *    make it a frame's job (rt_radiance_device).
 *  - Random draws.  As for rt_light_device: draw c of key k under `seed`; rng == NULL means key = i, counter 0.  tr (without u) and lv each start at
 *    the caller's counter; draws is the larger of the two advances.
 *  - A scene without a medium gives tr = 1, 0 in every other float output, hit = 0, and draws = 1 where tr without u was asked, else 0: what
 *    Transmittance returns for a null volumeRegion -- nothing else is ever asked of one.
 *  - Every march ends.  Before any launch the call refuses (RT_EINVAL) a step_size that is not positive and finite, and one for which the volume's
 *    diagonal takes more than 2^20 Tau samples or more than 65536 march steps: rt_render's limits, and the kernel's loop caps.  Per query, after
 *    clipping, a march cannot advance when t + step == t at the larger in magnitude of t0, t1 for the smallest step the query uses (.5f * step_size
 *    with lv, step_size with tau or u, else 4.f * step_size); an unusable ray (a non-finite o or d, d == 0, a NaN mint or maxt) and a clipped interval
 *    that is not finite count the same.  Such a query gets 0 in tau, tr and lv and bit 0 (RT_MEDIUM_NO_ADVANCE) in status.  Bit 1
 *    (RT_MEDIUM_TOO_LONG): lv along a ray whose direction is so short that the march would take more than 65536 steps; lv is 0.  Other queries are
 *    unaffected.  maxt = +inf and mint > maxt are ordinary rays.
 *  - Asynchronous on the scene's stream; no host copy, no wait, no workspace.  It is not a frame: the film, the sample buffer, the counters,
 *    rt_last_render_stats and rt_last_render_ms are untouched, and a later rt_render gives the film it gave before.
 *  - Refused before any launch with RT_EINVAL (rt_last_error names the function and the field): a null scene; with n > 0 a null query, a query with
 *    no output wanted, a point output without p, phase without w or wp, a ray output without rays, rays that are not 16-byte aligned, tau without
 *    u, lv without u_scatter, lv with volume_integrator == RT_VOLUME_SINGLE, the step limits above; n above 2^30.  n == 0 is RT_OK and
 *    launches nothing. */
enum { RT_MEDIUM_NO_ADVANCE = 1, RT_MEDIUM_TOO_LONG = 2 };
typedef struct RtMediumQuery {     /* device pointers unless said otherwise; any output may be NULL (not wanted) */
    const float    *p;         /* in  [n][3] points; may be NULL if no point output is wanted                  */
    const float    *w, *wp;    /* in  [n][3] directions of the phase function; may be NULL if phase is not wanted */
    const RtRay    *rays;      /* in  [n]    16-byte aligned; may be NULL if no ray output is wanted           */
    const float    *u;         /* in  [n]    Tau's offset, or NULL: tr is Scene::Transmittance(ray)            */
    const float    *u_scatter; /* in  [n]    the emission march's start offset; may be NULL if lv is not wanted */
    const uint32_t *rng;       /* in  [n][2] key, first counter of the keyed stream; NULL: key = i, 0          */
    uint32_t        seed;      /* host value, the meaning of RtRenderDesc.seed                                 */
    float           step_size; /* host value, the volume integrator's stepsize                                 */
    int32_t         volume_integrator; /* host value, RT_VOLUME_*: read for lv only                            */
    float   *sigma_a, *sigma_s, *sigma_t, *lve;   /* out [n][3]                                                */
    float   *phase;            /* out [n]    VolumeRegion::p(p, w, wp)                                         */
    int32_t *hit;              /* out [n]    IntersectP                                                        */
    float   *t01;              /* out [n][2] t0, t1                                                            */
    float   *tau, *tr, *lv;    /* out [n][3]                                                                   */
    int32_t *draws;            /* out [n]    how far the keyed stream moved                                    */
    int32_t *status;           /* out [n]    RT_MEDIUM_* bits                                                  */
} RtMediumQuery;
int rt_medium_device(RtScene *s, uint32_t n, const RtMediumQuery *q);
/* Camera::GenerateRay (core/camera.h:33-34; perspective.cpp:51-82, orthographic.cpp:48-79, environment.cpp:47-61) as rt_camera_rays, into
 * dev_rays[count]: the rays of camera samples first .. first + count - 1, bit for bit those of rt_camera_rays */
int rt_camera_rays_device(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, RtRay *dev_rays);
/* Scene::Li (core/scene.cpp:120-126: surfaceIntegrator->Li, then volumeIntegrator->Transmittance and volumeIntegrator->Li) for n rays in device
 * memory.  dev_out[n][4] = L.r, L.g, L.b, alpha (16-byte aligned, like dev_rays).
 *  - Sample set.  Li takes a Sample (scene.cpp:58).  Ray i is evaluated with the sample set of camera sample first + i of the frame `rd` describes:
 *    its keyed RNG stream, its Sample::oneD / twoD values under the frame's sampler (sampling.cpp:41-70), the frame's integrator and its
 *    parameters.  first + i is the index rt_samples_read and rt_camera_rays_device use on one shard: the scanline index pixel * spp + s.  Only
 *    the camera ray (scene.cpp:44-45) is replaced by the caller's.
 *  - The ray is taken as given: o, d, mint, maxt.  d must be of unit length -- the integrators use -d as wo (whitted.cpp:69, directlighting.cpp:100,
 *    path.cpp:98) as Camera::GenerateRay hands them normalised directions -- and the library does not renormalise, so that a camera ray comes
 *    back out bit for bit.  There are no ray differentials (scene.cpp:46-53): the textures that would read them are refused at scene create.
 *  - Defining property.  With dev_rays as rt_camera_rays_device(s, rd, first, n, ...) wrote them, dev_out[i] is floats 0..3 of record first + i
 *    that rt_render of that frame leaves for rt_samples_read, bit for bit -- the radiance check of scene.cpp:60-74 included: a NaN radiance, a
 *    luminance below -1e-5 or an infinite one becomes 0 (and counts as a bad sample).
 *  - Asynchronous on the scene's stream, no host copy and no wait, as the calls above.  The workspace is the per-thread scratch frames use (it
 *    does not depend on n) and grows -- waiting for the stream -- only when the query recurses deeper than any frame or query before it; a
 *    DirectLighting "all" query uploads its per-light sample requests when they differ from the last frame's, as rt_render does.
 *  - It is not a frame: neither the film nor the sample buffer is touched, rt_last_render_stats, rt_last_render_ms, rt_samples_read and
 *    rt_film_* report the last rt_render as before the call, and a later rt_render gives the film it gave before.
 *  - Counters.  With rt_set_counting on, the counting twin runs and rt_counters advances by what rt_render adds for those samples
 *    (camera_rays by n less the unusable rays).  stack_overflows belongs to the kernel form: it agrees where the frame ran the megakernel.
 *  - An unusable ray (rt::ray_usable, above) yields (0, 0, 0, 0) and traces nothing -- an infinite light's Le (infinite.cpp:84-95) would
 *    take its direction -- and counts nothing; the other rays of the call are unaffected.  maxt = +inf and mint > maxt are ordinary rays.
 *  - Accepted: Whitted, DirectLighting "all" and "one", Path; with or without a medium; kd-tree or grid; each sampler; shard_count == 1.
 *    Refused with RT_EINVAL before any launch (rt_last_error says which): DirectLighting "weighted" (its recurrence spans the frame,
 *    transport.cpp:71-122), the bidirectional and the debug integrator, shard_count != 1, first + n beyond the frame's camera samples, a NULL
 *    or misaligned pointer with n > 0, and what rt_render refuses of the description.  n == 0 is RT_OK and launches nothing.
 *  - Always the megakernel with the full shading set (every material, quadric and light) at natural register allocation: a query is
 *    somewhat slower than the frame's own kernel where that is a high-occupancy or fixed-frame one. */
int rt_radiance_device(RtScene *s, const RtRenderDesc *rd, const RtRay *dev_rays, uint64_t first, uint32_t n, float *dev_out);
/* Sample::imageX, imageY of camera samples first .. first + count - 1 of the frame `rd` describes into dev_xy[count][2] (8-byte aligned): floats 4
 * and 5 of the records rt_samples_read returns after rt_render of that frame, bit for bit.  The numbering is that of rt_camera_rays_device and
 * rt_radiance_device (the scanline index pixel * spp + s on one shard); only the sampler, film and extent fields of `rd` are read.  Asynchronous on
 * the scene's stream, no allocation, no copy, no wait.  Refused with RT_EINVAL before any launch: a null scene or description, a null or misaligned
 * pointer with count > 0, shard_count != 1, first + count beyond the frame's camera samples.  count == 0 is RT_OK and launches nothing. */
int rt_sample_positions_device(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, float *dev_xy);
/* What the volume integrator of camera samples first .. first + count - 1 of the frame `rd` describes starts from, into dev_out[count][4] 32-bit
 * words (16-byte aligned): the float value of its tau request (Sample::oneD[tauSampleOffset][0]), the float value of its scatter request
 * (oneD[scatterSampleOffset][0]), the key of the sample's keyed stream, and the counter at which the integrators' RandomFloat() draws start.  With
 * them rt_medium_device reproduces a frame's medium terms: u, u_scatter and rng.  Numbering, stream behaviour and refusals as for
 * rt_sample_positions_device; also refused: a description rt_render refuses for its sample requests, and a frame that plans no volume requests. */
int rt_volume_samples_device(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, uint32_t *dev_out);
/* Film::AddSample (scene.cpp:76 -> film/image.cpp:103-142) for n radiances in device memory: the third stage of Scene::Render's loop, behind
 * rt_camera_rays_device and rt_radiance_device.  dev_L[n][4] = L.r, L.g, L.b, alpha (16-byte aligned; the layout rt_radiance_device writes).
 *  - For i = 0 .. n-1 the bound film receives what Scene::Render would hand it for camera sample first + i of the frame `rd` describes if its
 *    radiance were dev_L[i]: first the radiance check of scene.cpp:60-74 -- a NaN component, a luminance below -1e-5 or an infinite one turns L
 *    into 0; the sample is still added, its weight and alpha * weight count, and with rt_set_counting on it counts as a bad sample -- then
 *    ImageFilm::AddSample at the sample's own imageX, imageY (rt_sample_positions_device), with the filter table, widths and crop window of `rd`.
 *  - Order.  Per film pixel the contributions are added on top of what the film holds, in ascending sample index: sample-pixel rows, then
 *    columns, then sample in pixel -- the order of a frame's own gather.  So the whole frame in one call gives the film of rt_render bit for
 *    bit, and so does every partition of [0, N) into contiguous chunks added in ascending order (a caller never needs the whole frame's
 *    radiances at once).  Chunks added in another order give a deterministic film that may differ from it in the last bit.
 *  - Only the sampler, film, filter, extent and shard fields of `rd` are read; the radiances need not come from an integrator of the library.
 *  - Asynchronous on the scene's stream.  The 1 KB filter table is uploaded as rt_render uploads it; otherwise no host copy and no wait, except
 *    that the call's staging buffer (8 bytes per sample of the range: sized by the chunk, not by the frame) grows when n exceeds the largest n
 *    added so far on the scene, which waits for the stream before the old block goes.
 *  - It is not a frame: rt_samples_read, rt_last_render_stats, rt_last_render_ms and the traversal counters report the last rt_render as
 *    before the call.  Only the film changed, and bad_samples where counting is on.
 *  - A sample pixel further from the crop window than the filter reaches (floor(width + .5) pixels) adds to no film pixel; its radiance is
 *    still checked and counted.
 *  - Refused before any launch (rt_last_error names the function and the reason): a null scene or description, a null or misaligned pointer with
 *    n > 0, shard_count != 1, first + n beyond the frame's camera samples, filter widths that are not positive, film coordinates beyond 32767
 *    (RT_EINVAL); no film bound (RT_ESTATE) or a film of another size than the crop window of `rd` (RT_EINVAL), as rt_render.  n == 0 is RT_OK
 *    and launches nothing. */
int rt_film_add_device(RtScene *s, const RtRenderDesc *rd, const float *dev_L, uint64_t first, uint32_t n);
/* The stream the scene's calls are queued on: its own (non-blocking) one, or what rt_scene_set_stream was given */
int rt_scene_get_stream(RtScene *s, void **hip_stream_out);

/* Film accumulators, ImageFilm::Pixel (image.cpp:57-65) as planes:
 * float accum[5][y_pixel_count][x_pixel_count] = sum w*L.r, .g, .b, sum w*alpha, sum w.
 * rt_film_bind: accumulate into caller-provided DEVICE memory (e.g. a torch tensor that is
 * later all-reduced by RCCL); pass NULL to let the library allocate. Zeroes nothing. */
int rt_film_bind(RtScene *s, void *device_accum, int32_t x_pixel_count, int32_t y_pixel_count);
int rt_film_clear(RtScene *s);
int rt_film_read(RtScene *s, float *host_accum);          /* 5*W*H floats, synchronises */
/* ImageFilm::WriteImage minus the file: XYZ round trip, /weightSum, clamps, premultiply
 * (image.cpp:157-203).  rgb_out[H][W][3], alpha_out[H][W] host buffers. */
int rt_film_resolve(RtScene *s, int premultiply_alpha, float *rgb_out, float *alpha_out);

/* Scene::Render's sample loop (scene.cpp:42-84) for this shard, asynchronous on the
 * handle's stream.  rt_sync waits.  Counters accumulate until rt_counters_reset.
 * With a medium the frame is refused (RT_EINVAL, before any launch) when a march needs more than 65536 steps; with a
 * density region also when an optical-depth march could take more than 2^20 samples of .5f * stepSize across the
 * volume's world bound, or when a ray parameter t within the union of the scene bound, the camera position and that
 * world bound is so large that t + .5f * stepSize == t (DensityRegion::Tau's loop would not advance). */
int rt_render(RtScene *s, const RtRenderDesc *rd);
int rt_sync(RtScene *s);
/* per-camera-sample results of the last rt_render, before filtering: out[count][8] = L.rgb, alpha, imageX, imageY, 0, 0 in the
 * sampler's order (what Scene::Render hands to Film::AddSample, scene.cpp:76).  The reference-side binding
 * (oracle/ref/hip_adapter.cpp) serves SurfaceIntegrator::Li from it.
 * Order: record w is work item w of this shard's work list.  shard_count == 1 rendered by the megakernel (every frame without a
 * medium): scanline order of the sample extent, whatever tile shape the descriptor names (one shard's tiles partition nothing).
 * Otherwise the shard's tiles in order, a tile's pixels in scanline order, a pixel's samples consecutively; with 2-D tiles the
 * border tiles are padded to whole tiles and the work items that fall off the sample extent are never rendered: their records hold
 * zeros or what an earlier frame left there (finite), and the film gathers never look at them. */
int rt_samples_read(RtScene *s, uint64_t first, uint64_t count, float *out);
int rt_counters(RtScene *s, RtCounters *out);             /* synchronises */
int rt_counters_reset(RtScene *s);
/* per-ray statistics cost a few VALU ops per node visit: enabled (default) for parity/accounting runs,
 * disabled for timed runs; the frame is deterministic so counts of one run describe the other */
int rt_set_counting(RtScene *s, int enabled);
/* elapsed GPU milliseconds of the last rt_render launch sequence (HIP events on the
 * handle's stream) and of its dominant kernel */
int rt_last_render_ms(RtScene *s, float *total_ms, float *kernel_ms);
/* The same by kernel.  Small, cache-resident scenes render with one persistent megakernel (pipeline = 0: trace_ms == render_ms);
 * large ones with the queue pipeline (pipeline = 1): `iterations` alternations of the shade kernel (SurfaceIntegrator::Li between
 * two rays, for every path slot) and the trace kernel (KdTreeAccel::Intersect / IntersectP for the queued rays); trace_ms is the
 * sum over the first `timed_iterations` trace launches (all of them unless a frame needs more than 256). */
typedef struct RtRenderStats {
    float total_ms, render_ms, trace_ms, gather_ms;
    int32_t pipeline, iterations, timed_iterations;
    uint32_t slots;
    float shade_ms;            /* queue pipeline: the shade launches summed */
    int32_t bands;             /* megakernel: 1 (one launch per frame); pipeline: 0 */
    float march_ms;            /* queue pipeline with a medium: the ray-march launches summed (rt::pipe_march_kernel: the marches' shadow rays are traced inside it) */
    /* DirectLighting "weighted" (three megakernel passes + the recurrence; render_ms is all of them): the frame's shading points = calls of
     * WeightedSampleOneLight, and the ms of the count pass, the scan, the survey pass, the recurrence kernel and the frame pass; zeros otherwise */
    uint64_t weighted_points;
    float weighted_ms[5];
    int32_t fixed_frame;       /* megakernel: 1 when the frame ran a kernel compiled for its sampler, camera and work order (stratified, n == 1 requests, no lens,
                                * no environment camera, one shard; same film bit for bit), 0 when it ran the generic kernel */
    int32_t fixed_scene;       /* ... and non-zero when that kernel was compiled for the scene as well, a bit per axis: 1 the scene's one light, 2 no material with a
                                * specular lobe (same film bit for bit again); 0 otherwise */
} RtRenderStats;
/* ImageFilm::WriteImage's normalisation (image.cpp:157-203) of ANY 5-plane accumulator in device memory (planes of n floats each), e.g. the
 * rows of the film a rank owns after a reduce-scatter; rgb[n][3] and alpha[n] stay on the device.  Asynchronous on the scene's stream. */
int rt_film_resolve_device(RtScene *s, const float *dev_accum, uint64_t n, int premultiply, float *dev_rgb, float *dev_alpha);
/* The same with the result interleaved, dev_rgba[n][4] (16-byte aligned): what ONE all-gather moves when every rank resolves its own rows. */
int rt_film_resolve_device_rgba(RtScene *s, const float *dev_accum, uint64_t n, int premultiply, float *dev_rgba);
/* N > 1 film merge, send side.  The reference has no in-process merge: every cropwindow process writes its own image
 * (film/image.cpp:220-228) and tools/exrassemble.cpp:42-75 adds them up.  Here a rank's full-frame 5-plane film `dev_accum`
 * (h rows of w) is re-laid as `world` parts of `rows` film rows each, part r = [5][rows][w] (rows beyond h zero; world * rows >= h):
 * the send buffer of ONE reduce-scatter whose r-th chunk is everything rank r resolves.  dev_parts = world*5*rows*w floats.
 * Asynchronous on the scene's stream. */
int rt_film_pack_parts(RtScene *s, const float *dev_accum, int32_t w, int32_t h, int32_t world, int32_t rows, float *dev_parts);
int rt_last_render_stats(RtScene *s, RtRenderStats *out);

#ifdef __cplusplus
}
#endif
#endif /* PBRT_HIP_H */
