// rt_scene.hip -- rt_scene_create: the flattened accelerator (kd_build.cpp / grid_build.cpp, or a prebuilt one) and everything the kernels read derived from it and
// uploaded -- primitive records and leaf entries, sibling-pair blocks, shading constants, lights -- plus the launch geometry of the persistent kernels;
// rt_scene_destroy, and the accelerator-only entry points (rt_accel_* / rt_kdtree_*) of the C ABI.
#include "rt_host.h"
#include "../../../include/pbrt_hip_material.h"

// tri_frame() of rt_shade.h on the host: same operations in the same order (trianglemesh.cpp:248-274, shape.cpp:43-50,
// reflection.cpp:475-476)
static void host_tri_frame(const float *v, bool flip, float nn[3], float sn[3]) {
    const float du1 = 0.f - 1.f, du2 = 1.f - 1.f, dv1 = 0.f - 1.f, dv2 = 0.f - 1.f;
    const float determinant = du1 * dv2 - dv1 * du2;
    const float invdet = 1.f / determinant;
    float dpdu[3], dpdv[3];
    for (int a = 0; a < 3; ++a) {
        const float dp1 = v[a] - v[6 + a], dp2 = v[3 + a] - v[6 + a];
        dpdu[a] = invdet * ((dv2 * dp1) - (dv1 * dp2));
        dpdv[a] = invdet * ((-du2 * dp1) + (du1 * dp2));
    }
    float c[3] = {(dpdu[1] * dpdv[2]) - (dpdu[2] * dpdv[1]), (dpdu[2] * dpdv[0]) - (dpdu[0] * dpdv[2]), (dpdu[0] * dpdv[1]) - (dpdu[1] * dpdv[0])};
    float inv = 1.f / sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int a = 0; a < 3; ++a) { nn[a] = c[a] * inv; if (flip) nn[a] = -1.f * nn[a]; }
    inv = 1.f / sqrtf(dpdu[0] * dpdu[0] + dpdu[1] * dpdu[1] + dpdu[2] * dpdu[2]);
    for (int a = 0; a < 3; ++a) sn[a] = dpdu[a] * inv;
}

// the records on the host (the check of rt::derive_leaf_records_kernel below: PBRT_HIP_VERIFY_DERIVED compares the two byte for byte)
static void leaf_records_fill_host(const RefVec &slot_prim, const std::vector<DevTri> &tris, std::vector<float4> &ltris) {
    ltris.assign(slot_prim.size() * RT_TRI_STRIDE + 4, make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t i = 0; i < slot_prim.size(); ++i) {
        const uint32_t prim = slot_prim[i];
        float4 q2 = tris[prim].q2; std::memcpy(&q2.w, &prim, 4);
        float4 *dst = ltris.data() + i * RT_TRI_STRIDE;
        dst[0] = tris[prim].q0; dst[1] = tris[prim].q1; dst[2] = q2;
    }
}
// ... and on the device: one thread per record copies its primitive out of the mesh-order records that are in HBM anyway (the primitive's index goes
// into the spare word; the padding was zeroed by a memset before the launch)
namespace rt {
__global__ void derive_leaf_records_kernel(const unsigned *__restrict__ slot_prim, const DevTri *__restrict__ tris, float4 *__restrict__ ltris, size_t n_slots) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const unsigned prim = slot_prim[i];
    const DevTri t = tris[prim];
    float4 q2 = t.q2; q2.w = __uint_as_float(prim);
    float4 *dst = ltris + i * RT_TRI_STRIDE;
    dst[0] = t.q0; dst[1] = t.q1; dst[2] = q2;
}
}  // namespace rt

// Triangle::Intersect's frame with the mesh's own uvs (trianglemesh.cpp:248-268 incl. the zero-determinant fallback through
// CoordinateSystem, geometry.h:324-334) + DifferentialGeometry ctor (shape.cpp:43-50): geometric normal, raw dpdu
static void host_tri_frame_uv(const float *v, const float *uv, bool flip, float nn[3], float dpdu[3]) {
    const float du1 = uv[0] - uv[4], du2 = uv[2] - uv[4], dv1 = uv[1] - uv[5], dv2 = uv[3] - uv[5];
    const float determinant = du1 * dv2 - dv1 * du2;
    float dpdv[3];
    if (determinant == 0.f) {
        const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        float c[3] = {(e2[1] * e1[2]) - (e2[2] * e1[1]), (e2[2] * e1[0]) - (e2[0] * e1[2]), (e2[0] * e1[1]) - (e2[1] * e1[0])};
        const float inv = 1.f / sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const float v1[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
        if (fabsf(v1[0]) > fabsf(v1[1])) { const float invLen = 1.f / sqrtf(v1[0] * v1[0] + v1[2] * v1[2]); dpdu[0] = -v1[2] * invLen; dpdu[1] = 0.f; dpdu[2] = v1[0] * invLen; }
        else { const float invLen = 1.f / sqrtf(v1[1] * v1[1] + v1[2] * v1[2]); dpdu[0] = 0.f; dpdu[1] = v1[2] * invLen; dpdu[2] = -v1[1] * invLen; }
        dpdv[0] = (v1[1] * dpdu[2]) - (v1[2] * dpdu[1]); dpdv[1] = (v1[2] * dpdu[0]) - (v1[0] * dpdu[2]); dpdv[2] = (v1[0] * dpdu[1]) - (v1[1] * dpdu[0]);
    } else {
        const float invdet = 1.f / determinant;
        for (int a = 0; a < 3; ++a) {
            const float dp1 = v[a] - v[6 + a], dp2 = v[3 + a] - v[6 + a];
            dpdu[a] = ((dv2 * dp1) - (dv1 * dp2)) * invdet;
            dpdv[a] = ((-du2 * dp1) + (du1 * dp2)) * invdet;
        }
    }
    const float c[3] = {(dpdu[1] * dpdv[2]) - (dpdu[2] * dpdv[1]), (dpdu[2] * dpdv[0]) - (dpdu[0] * dpdv[2]), (dpdu[0] * dpdv[1]) - (dpdu[1] * dpdv[0])};
    const float inv = 1.f / sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int a = 0; a < 3; ++a) { nn[a] = c[a] * inv; if (flip) nn[a] = -1.f * nn[a]; }
}

// The tree as sibling pairs (rt_device.h DevScene::tpairs: a record holds the two node words of a node's below child and the two of its above
// child, addressed by absolute index) laid out in BLOCKS for the two-level step (kdp_step, rt_traverse.h): an "owner" node P is followed by the pairs of
// its interior children -- {pair(P), pair(below(P)), pair(above(P))}, 16 / 32 / 48 bytes, never across a 64-byte boundary (next-fit
// padding) -- and bits 30 / 31 of every word 1 that points at P say which of the two follow.  The owners are the root and, recursively,
// the interior grandchildren of an owner; the nodes in between are "members" of their parent's block (flags 0: when a member is reached
// through a pop it takes a one-level step).  Blocks are emitted depth-first, the below side first, so a subtree stays contiguous.
// Two phases: pair_blocks_order() decides where every pair goes (a sequential depth-first walk that looks at the tree's SHAPE only, so it runs
// beside leaf_cursor_layout on another thread), pair_blocks_fill() writes the records (needs the leaves in entry form; 64 threads).
// Round 5: the blocks of the tree's TOP levels come first, breadth-first (owner level by owner level, below side first) and packed without
// padding, RT_TOP_PREFIX records at most (any prefix of the array is "the topmost blocks": what an LDS copy would want -- measured, not kept,
// profiles/r05_lds_top_scan.txt -- and what every ray walks sits in 64 KB).  The subtrees below that frontier follow depth-first in 64-byte-aligned blocks as before.
#ifndef RT_TOP_PREFIX
#define RT_TOP_PREFIX 4095u          // 1365 blocks of three records: 11-12 levels of a full tree
#endif
struct PairBlockOrder { std::vector<uint32_t> order, pos; std::vector<uint8_t> owner; uint32_t top = 0; };
static void pair_blocks_order(const NodeVec &tn, PairBlockOrder &o) {
    o.order.clear(); o.pos.clear(); o.owner.clear(); o.top = 0;
    if (tn.empty() || (tn[0].x & 3u) == 3u) return;
    auto interior = [&](uint32_t n) { return (tn[n].x & 3u) != 3u; };
    std::vector<uint32_t> &order = o.order;                                   // parent node of each emitted pair (~0u = padding)
    o.pos.assign(tn.size(), ~0u);                                             // node -> index of its children's pair
    o.owner.assign(tn.size(), 0);
    // emit the block of owner P behind `ord`; `next` receives the owners below it (the interior children of its members), below side first
    auto emit = [&](std::vector<uint32_t> &ord, uint32_t P, bool aligned, std::vector<uint32_t> &next, bool reversed) {
        const uint32_t b = P + 1u, a = tn[P].y;
        const bool bI = interior(b), aI = interior(a);
        const size_t size = 1u + (bI ? 1u : 0u) + (aI ? 1u : 0u);
        if (aligned && (ord.size() % 4) + size > 4) while (ord.size() % 4) ord.push_back(~0u);
        o.owner[P] = 1;
        ord.push_back(P);
        if (bI) ord.push_back(b);
        if (aI) ord.push_back(a);
        const uint32_t mem[2] = {reversed ? a : b, reversed ? b : a};
        const bool memI[2] = {reversed ? aI : bI, reversed ? bI : aI};
        for (int k = 0; k < 2; ++k) {
            if (!memI[k]) continue;
            const uint32_t m = mem[k], mb = m + 1u, ma = tn[m].y;
            const uint32_t c[2] = {reversed ? ma : mb, reversed ? mb : ma};
            for (int j = 0; j < 2; ++j) if (interior(c[j])) next.push_back(c[j]);
        }
    };
    // the top: breadth-first, dense
    std::vector<uint32_t> level{0u}, below;
    size_t li = 0;
    while (li < level.size() && order.size() + 3u <= RT_TOP_PREFIX) {
        emit(order, level[li++], false, below, false);
        if (li == level.size()) { level.swap(below); below.clear(); li = 0; }
    }
    o.top = uint32_t(order.size());
    while (order.size() % 4) order.push_back(~0u);
    for (size_t i = 0; i < order.size(); ++i) if (order[i] != ~0u) o.pos[order[i]] = uint32_t(i);
    // what is left: the rest of the current level, then the owners found below it.  Each of these frontier subtrees is laid out depth-first on its own (a stack:
    // below(below(P)) follows P), starting on a 64-byte boundary -- so its layout depends on nothing outside it, and the subtrees are walked by all threads (the walk
    // over 123 M interior nodes took 2 s at 10 M triangles); the pieces follow the prefix in frontier order whatever the thread count.
    std::vector<uint32_t> roots;
    for (size_t k = li; k < level.size(); ++k) roots.push_back(level[k]);
    for (uint32_t r : below) roots.push_back(r);
    std::vector<std::vector<uint32_t>> sub(roots.size());
    const size_t nthreads = tn.size() < (size_t(1) << 22) ? 1 : std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
    auto run = [&](auto fn) {
        if (nthreads == 1) { for (size_t k = 0; k < roots.size(); ++k) fn(k); return; }
        std::atomic<size_t> next(0);
        ThreadGroup pool;
        for (size_t t = 0; t < nthreads; ++t) pool.spawn([&] { for (;;) { const size_t k = next.fetch_add(1); if (k >= roots.size()) return; fn(k); } });
    };
    run([&](size_t k) {
        std::vector<uint32_t> &ord = sub[k], todo{roots[k]};
        while (!todo.empty()) { const uint32_t P = todo.back(); todo.pop_back(); emit(ord, P, true, todo, true); }
        while (ord.size() % 4) ord.push_back(~0u);
    });
    std::vector<size_t> base(roots.size() + 1, order.size());
    for (size_t k = 0; k < roots.size(); ++k) base[k + 1] = base[k] + sub[k].size();
    order.resize(base[roots.size()]);
    run([&](size_t k) {
        const std::vector<uint32_t> &ord = sub[k];
        uint32_t *dst = order.data() + base[k];
        for (size_t i = 0; i < ord.size(); ++i) { dst[i] = ord[i]; if (ord[i] != ~0u) o.pos[ord[i]] = uint32_t(base[k] + i); }
        std::vector<uint32_t>().swap(sub[k]);
    });
}
// `tn`: the nodes with the leaves in entry form (LeafLayout::tnodes; interior nodes as in the tree: same shape as pair_blocks_order saw)
static void pair_blocks_fill(const NodeVec &tn, const PairBlockOrder &o, std::vector<uint4> &pairs, uint32_t &root_x, uint32_t &root_y) {
    pairs.clear();
    if (tn.empty()) { root_x = 3u; root_y = 0u; pairs.push_back(make_uint4(3u, 0u, 3u, 0u)); return; }
    root_x = tn[0].x;
    if ((tn[0].x & 3u) == 3u) { root_y = tn[0].y; pairs.push_back(make_uint4(3u, 0u, 3u, 0u)); return; }
    const std::vector<uint32_t> &order = o.order;
    if (order.size() >= (size_t(1) << 30)) return;
    auto interior = [&](uint32_t n) { return (tn[n].x & 3u) != 3u; };
    auto word1 = [&](uint32_t n) -> uint32_t {
        if (!interior(n)) return tn[n].y;                                     // leaf: flags of its first entry | cursor
        uint32_t y = o.pos[n];
        if (o.owner[n]) y |= (interior(n + 1u) ? 1u << 30 : 0u) | (interior(tn[n].y) ? 1u << 31 : 0u);
        return y;
    };
    pairs.resize(order.size());
    auto fill = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const uint32_t P = order[i];
            if (P == ~0u) { pairs[i] = make_uint4(3u, 0u, 3u, 0u); continue; }
            const uint32_t b = P + 1u, a = tn[P].y;
            pairs[i] = make_uint4(tn[b].x, word1(b), tn[a].x, word1(a));
        }
    };
    const size_t nthreads = order.size() < (size_t(1) << 20) ? 1 : std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
    if (nthreads == 1) fill(0, order.size());
    else {
        ThreadGroup pool;
        for (size_t t = 0; t < nthreads; ++t) pool.spawn(fill, order.size() * t / nthreads, order.size() * (t + 1) / nthreads);
    }
    root_y = word1(0u);
}

static void fill_info(const KdTree &tree, const GridAccelData &g, int kind, uint32_t n_tris, RtAccelInfo *info);
extern "C" int rt_scene_destroy(RtScene *s);

extern "C" {

// structural check of an accelerator handed in by the caller (rt_scene_create_prebuilt): every index the traversal follows stays in range
static int check_prebuilt(const RtPrebuiltAccel *a, uint32_t n_tris) {
    if (!a->nodes || (a->n_leaf_refs && !a->leaf_refs)) return fail(RT_EINVAL, "rt_scene_create_prebuilt: null accelerator arrays");
    const uint32_t *nd = a->nodes;
    for (uint32_t i = 0; i < a->n_leaf_refs; ++i) if (a->leaf_refs[i] >= n_tris) return fail(RT_EINVAL, "rt_scene_create_prebuilt: primitive index out of range");
    if (a->kind == RT_ACCEL_KDTREE) {
        if (a->n_nodes == 0 && n_tris != 0) return fail(RT_EINVAL, "rt_scene_create_prebuilt: empty tree");
        // The per-thread spill area of the traversal stack is sized from max_depth (scene_create), so the claim is checked, not trusted: a
        // child's index is larger than its parent's, hence one forward sweep gives every node's depth (the deeper path wins if a node has two parents).
        if (a->max_depth > 64) return fail(RT_EINVAL, "rt_scene_create_prebuilt: max_depth beyond 64");
        std::vector<uint8_t> depth(a->n_nodes, 0);
        for (uint32_t i = 0; i < a->n_nodes; ++i) {
            const uint32_t x = nd[2 * size_t(i)], y = nd[2 * size_t(i) + 1];
            if ((x & 3u) != 3u) {
                if (y <= i + 1u || y >= a->n_nodes || i + 1u >= a->n_nodes) return fail(RT_EINVAL, "rt_scene_create_prebuilt: child index out of range");
                if (!std::isfinite(*reinterpret_cast<const float *>(&nd[2 * size_t(i)]))) return fail(RT_EINVAL, "rt_scene_create_prebuilt: split position is not finite");
                const unsigned dc = unsigned(depth[i]) + 1u;
                if (dc > a->max_depth) return fail(RT_EINVAL, "rt_scene_create_prebuilt: the tree is deeper than its max_depth says");
                if (depth[i + 1u] < dc) depth[i + 1u] = uint8_t(dc);
                if (depth[y] < dc) depth[y] = uint8_t(dc);
            } else {
                const uint32_t np = x >> 2;
                if (np == 1u ? y >= n_tris : (np > 1u && (y > a->n_leaf_refs || np > a->n_leaf_refs - y))) return fail(RT_EINVAL, "rt_scene_create_prebuilt: leaf list out of range");
            }
        }
    } else {
        const unsigned long long nv = (unsigned long long)a->grid_nvoxels[0] * a->grid_nvoxels[1] * a->grid_nvoxels[2];
        if (a->grid_nvoxels[0] < 1 || a->grid_nvoxels[1] < 1 || a->grid_nvoxels[2] < 1 || nv != a->n_nodes) return fail(RT_EINVAL, "rt_scene_create_prebuilt: voxel counts do not match");
        for (uint32_t i = 0; i < a->n_nodes; ++i) {
            const uint32_t off = nd[2 * size_t(i)], cnt = nd[2 * size_t(i) + 1];
            if (off > a->n_leaf_refs || cnt > a->n_leaf_refs - off) return fail(RT_EINVAL, "rt_scene_create_prebuilt: voxel list out of range");
        }
    }
    for (int k = 0; k < 6; ++k) if (!std::isfinite(a->bounds[k])) return fail(RT_EINVAL, "rt_scene_create_prebuilt: bounds are not finite");
    for (int k = 0; k < 3; ++k) {
        if (a->bounds[k] > a->bounds[3 + k] && n_tris != 0) return fail(RT_EINVAL, "rt_scene_create_prebuilt: bounds are inverted");
        // (a flat scene has width = inv_width = 0 on its thin axis, as GridAccel's constructor makes them: grid.cpp:102-104)
        if (a->kind == RT_ACCEL_GRID && (!(a->grid_width[k] >= 0.f) || !(a->grid_inv_width[k] >= 0.f) || !std::isfinite(a->grid_width[k]) || !std::isfinite(a->grid_inv_width[k])))
            return fail(RT_EINVAL, "rt_scene_create_prebuilt: voxel widths must be non-negative and finite");
    }
    return RT_OK;
}

static int scene_create(const RtSceneDesc *d, int device, const RtPrebuiltAccel *pre, RtScene **out);
int rt_scene_create(const RtSceneDesc *d, int device, RtScene **out) { return guarded("rt_scene_create", [&] { return scene_create(d, device, nullptr, out); }); }
// The same scene with the accelerator somebody else built (rt_accel_build / rt_scene_accel_copy of another rank's scene): the ranks of one
// node build the kd-tree ONCE (10 M triangles: 15 s on all host cores) instead of once per process.  The arrays are the canonical flattened
// tree (pbrt_hip.h RtAccelInfo / rt_accel_copy); everything the device derives from them (primitive records and leaf entries, pair blocks) is rebuilt here.
int rt_scene_create_prebuilt(const RtSceneDesc *d, int device, const RtPrebuiltAccel *pre, RtScene **out) {
    if (!pre) return fail(RT_EINVAL, "rt_scene_create_prebuilt: null accelerator");
    return guarded("rt_scene_create_prebuilt", [&] { return scene_create(d, device, pre, out); });
}
static int scene_create(const RtSceneDesc *d, int device, const RtPrebuiltAccel *pre, RtScene **out) {
    if (!d || !out) return fail(RT_EINVAL, "rt_scene_create: null argument");
    if (pre) {
        if (pre->kind != d->accel.kind) return fail(RT_EINVAL, "rt_scene_create_prebuilt: accelerator kind differs from the scene's");
        int rc = check_prebuilt(pre, d->n_tris); if (rc) return rc;
    }
    if (d->n_tris && (!d->tri_verts || !d->tri_material || !d->tri_light || !d->tri_flags))
        return fail(RT_EINVAL, "rt_scene_create: missing triangle arrays");
    if (d->accel.kind != RT_ACCEL_KDTREE && d->accel.kind != RT_ACCEL_GRID) return fail(RT_EINVAL, "rt_scene_create: unknown accelerator kind");
    for (uint32_t i = 0; i < d->n_tris; ++i) {
        if (d->tri_material[i] >= d->n_materials) return fail(RT_EINVAL, "rt_scene_create: material index out of range");
        const int32_t tl = d->tri_light[i];               // the device indexes `lights` with it (make_vertex, prim_normal_light)
        if (tl < -1 || tl >= int32_t(d->n_lights) || (tl >= 0 && d->lights[tl].type != RT_LIGHT_AREA))
            return fail(RT_EINVAL, "rt_scene_create: triangle refers to a light that is out of range or not an area light");
    }
    if (d->n_lights > 65534u) return fail(RT_EINVAL, "rt_scene_create: more than 65534 lights");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(RT_EDEVICE, "rt_scene_create: no HIP device visible (the product path has no CPU fallback)");
    // every error exit below goes through the guard: rt_scene_destroy deletes the scene, whose members release whatever has been created so far
    struct Guard { RtScene *p; ~Guard() { if (p) rt_scene_destroy(p); } } guard{new RtScene()};
    RtScene *s = guard.p;
    if (device >= 0) { hipError_t e = hipSetDevice(device); if (e != hipSuccess) return fail(RT_EDEVICE, "hipSetDevice failed"); }
    HIPCHK(hipGetDevice(&s->device));
    HIPCHK(hipStreamCreateWithFlags(&s->own_stream.p, hipStreamNonBlocking)); s->stream = s->own_stream;
    HIPCHK(hipEventCreate(&s->ev0.p)); HIPCHK(hipEventCreate(&s->ev1.p));
    s->n_tris = d->n_tris;

    const bool tlog = knob("PBRT_HIP_CREATE_LOG") != nullptr;           // where a scene create spends its time (10 M triangles: a minute)
    auto t_prev = std::chrono::steady_clock::now();
    auto tick = [&](const char *what) {
        if (!tlog) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "CREATE %-28s %.3f s\n", what, std::chrono::duration<double>(now - t_prev).count()); t_prev = now;
    };
    s->facts.accel_kind = d->accel.kind;
    if (pre) {
        const Node *pn = reinterpret_cast<const Node *>(pre->nodes);
        s->tree.nodes.assign(pn, pn + pre->n_nodes); s->tree.leaf_refs.assign(pre->leaf_refs, pre->leaf_refs + pre->n_leaf_refs);
        s->tree.max_depth = int(pre->max_depth); s->tree.build_seconds = 0.0;
        std::memcpy(s->tree.bounds, pre->bounds, sizeof s->tree.bounds);
        if (s->facts.accel_kind == RT_ACCEL_GRID) {
            s->gridacc.voxels = s->tree.nodes; s->gridacc.refs = s->tree.leaf_refs; s->gridacc.build_seconds = 0.0;
            std::memcpy(s->gridacc.bounds, pre->bounds, sizeof s->gridacc.bounds);
            for (int a = 0; a < 3; ++a) { s->gridacc.nvox[a] = pre->grid_nvoxels[a]; s->gridacc.width[a] = pre->grid_width[a]; s->gridacc.inv_width[a] = pre->grid_inv_width[a]; }
        }
    } else if (s->facts.accel_kind == RT_ACCEL_GRID) {
        build_grid(d->tri_verts, d->n_tris, s->gridacc);
        s->tree.nodes = s->gridacc.voxels; s->tree.leaf_refs = s->gridacc.refs; s->tree.max_depth = 0;
        std::memcpy(s->tree.bounds, s->gridacc.bounds, sizeof s->tree.bounds); s->tree.build_seconds = s->gridacc.build_seconds;
    } else build_kdtree(d->tri_verts, d->n_tris, d->accel, s->tree);

    {   // what the scheduling policy asks of the tree (plan_schedule, rt_frame_plan.h): its size and how fat its leaves are.  Here, where the nodes are at
        // hand, once per scene: a pass over 36 M nodes costs 12 ms, not something to pay per frame
        size_t leaves = 0, refs = 0;
        if (s->facts.accel_kind == RT_ACCEL_KDTREE) for (const Node &n : s->tree.nodes) if ((n.x & 3u) == 3u && (n.x >> 2)) { ++leaves; refs += n.x >> 2; }
        s->facts.n_nodes = s->tree.nodes.size();
        s->facts.per_leaf = leaves ? double(refs) / double(leaves) : 1.0;
    }
    tick("accelerator");
    // the order of the pair blocks: a sequential walk over the tree's shape (1.8 s at 10 M triangles) on its own thread, beside everything up to the pair fill
    PairBlockOrder pbo;
    std::thread order_thread;
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{order_thread};
    if (s->facts.accel_kind == RT_ACCEL_KDTREE) order_thread = std::thread([&] { pair_blocks_order(s->tree.nodes, pbo); });
    // ... and so do the leaf entries (four passes over the leaf lists by all host threads: 1.3 s at 10 M triangles) while this thread fills the per-triangle records
    // and uploads the tree.  Scenes of a few thousand references (C2's 14 triangles: cache resident, bound by instruction issue -- the entry form costs it 2.8 %,
    // profiles/r06_dedup_scan.txt) get runs of consecutive records per leaf; everything larger shares one record per primitive.
    LeafLayout ll;
    int ll_status = 0;                                  // 1 laid out, -1 index ranges exceeded, -2 out of memory
    bool runs = s->tree.leaf_refs.size() + s->tree.nodes.size() / 2 <= 32768;
    if (const char *e = knob("PBRT_HIP_LEAF_RUNS")) runs = std::atoi(e) != 0;
    const bool copies = knob("PBRT_HIP_LEAF_COPIES") != nullptr;
    std::thread layout_thread;
    Joiner joiner2{layout_thread};
    if (s->facts.accel_kind == RT_ACCEL_KDTREE) layout_thread = std::thread([&] {
        try { ll_status = leaf_cursor_layout(s->tree.nodes, s->tree.leaf_refs, d->n_tris, copies, runs, ll) ? 1 : -1; } catch (...) { ll_status = -2; }
    });
    // triangles -> 48-byte records
    std::vector<DevTri> tris(d->n_tris);
    uint32_t n_quadric_slots = 0;
    for (uint32_t i = 0; i < d->n_tris; ++i) {
        const float *v = d->tri_verts + size_t(9) * i;
        uint32_t bits = uint32_t(d->tri_material[i]) | (uint32_t(d->tri_flags[i] & 1u) << 16);
        int32_t light = d->tri_light[i];
        float fb, fl; std::memcpy(&fb, &bits, 4); std::memcpy(&fl, &light, 4);
        if (d->tri_flags[i] & 2u) {                       // quadric slot: {index, -, -} | bits | light
            bits |= RT_PRIM_QUADRIC; std::memcpy(&fb, &bits, 4);
            float fi; std::memcpy(&fi, &n_quadric_slots, 4); ++n_quadric_slots;
            tris[i].q0 = make_float4(fi, 0.f, 0.f, 0.f); tris[i].q1 = make_float4(0.f, 0.f, 0.f, 0.f); tris[i].q2 = make_float4(0.f, fb, fl, 0.f);
            continue;
        }
        const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        tris[i].q0 = make_float4(v[0], v[1], v[2], e1[0]);
        tris[i].q1 = make_float4(e1[1], e1[2], e2[0], e2[1]);
        tris[i].q2 = make_float4(e2[2], fb, fl, 0.f);
    }
    // per-triangle shading constants: tri_frame() (rt_shade.h) evaluated once on the host with the same float
    // expressions (this file is compiled -ffp-contract=off for the host too; sqrt and divide are IEEE on both sides)
    std::vector<float4> shade(size_t(2) * d->n_tris);
    if (n_quadric_slots != d->n_quadrics || (d->n_quadrics && !d->quadrics)) return fail(RT_EINVAL, "rt_scene_create: quadric slots do not match n_quadrics");
    s->facts.has_ext = s->facts.has_ext || d->n_quadrics > 0;
    std::vector<DevTriShading> dshading; std::vector<int> shading_idx;
    if (d->tri_shading) {
        if (d->n_shading && !d->shading) return fail(RT_EINVAL, "rt_scene_create: tri_shading without shading records");
        shading_idx.assign(d->n_tris, -1);
    }
    for (uint32_t i = 0; i < d->n_tris; ++i) {
        float nn[3] = {0.f, 0.f, 0.f}, sn[3] = {0.f, 0.f, 0.f};
        const int sh = (d->tri_shading && !(d->tri_flags[i] & 2u)) ? d->tri_shading[i] : -1;
        bool smooth = false;
        if (sh >= 0) {                                   // the mesh has uv / N / S: the frame depends on its uvs (trianglemesh.cpp:248-268)
            if (uint32_t(sh) >= d->n_shading) return fail(RT_EINVAL, "rt_scene_create: shading record index out of range");
            const RtTriShading &r = d->shading[sh];
            if ((r.flags & (RT_SHADING_N | RT_SHADING_S)) && (r.xform >= d->n_xforms || !d->xforms)) return fail(RT_EINVAL, "rt_scene_create: shading record refers to a transform out of range");
            float dpdu[3];
            host_tri_frame_uv(d->tri_verts + size_t(9) * i, r.uv, (d->tri_flags[i] & 1u) != 0, nn, dpdu);
            const float inv = 1.f / sqrtf(dpdu[0] * dpdu[0] + dpdu[1] * dpdu[1] + dpdu[2] * dpdu[2]);
            for (int a = 0; a < 3; ++a) sn[a] = dpdu[a] * inv;
            if (r.flags & RT_SHADING_UV) {                                        // kept on the host: rt_scene_set_textures uploads the uvs of a scene that gets textures (hit_point_uv)
                if (s->tex_uv_idx_host.empty()) s->tex_uv_idx_host.assign(d->n_tris, -1);
                s->tex_uv_idx_host[i] = int(s->tex_uv_host.size() / 6);
                s->tex_uv_host.insert(s->tex_uv_host.end(), r.uv, r.uv + 6);
            }
            if (r.flags & (RT_SHADING_N | RT_SHADING_S)) {
                smooth = true; s->facts.has_ext = true;
                DevTriShading o; std::memset(&o, 0, sizeof o);
                o.flags = r.flags; o.xform = r.xform;
                std::memcpy(o.uv, r.uv, sizeof o.uv); std::memcpy(o.dpdu, dpdu, sizeof o.dpdu);
                std::memcpy(o.n, r.n, sizeof o.n); std::memcpy(o.s, r.s, sizeof o.s);
                shading_idx[i] = int(dshading.size()); dshading.push_back(o);
            }
        } else if (!(d->tri_flags[i] & 2u)) host_tri_frame(d->tri_verts + size_t(9) * i, (d->tri_flags[i] & 1u) != 0, nn, sn);
        uint32_t bits = uint32_t(d->tri_material[i]) | (uint32_t(d->tri_flags[i] & 1u) << 16) | ((d->tri_flags[i] & 2u) ? RT_PRIM_QUADRIC : 0u) |
                        (smooth ? RT_PRIM_SHADING : 0u);
        int32_t light = d->tri_light[i];
        float fb, fl; std::memcpy(&fb, &bits, 4); std::memcpy(&fl, &light, 4);
        shade[2 * i] = make_float4(nn[0], nn[1], nn[2], fb);
        shade[2 * i + 1] = make_float4(sn[0], sn[1], sn[2], fl);
    }
    int rc;
    if ((rc = upload(s, shade.data(), shade.size(), &s->dev.tri_shade))) return rc;
    if (!dshading.empty()) {
        if ((rc = upload(s, shading_idx.data(), shading_idx.size(), &s->dev.tri_shading_idx))) return rc;
        if ((rc = upload(s, dshading.data(), dshading.size(), &s->dev.tri_shading))) return rc;
        if ((rc = upload(s, d->xforms, size_t(d->n_xforms) * 32, &s->dev.xforms))) return rc;
    }
    if ((rc = upload(s, tris.data(), tris.size(), &s->dev.tris))) return rc;
    {
        std::vector<DevQuadric> dq(d->n_quadrics);
        for (uint32_t i = 0; i < d->n_quadrics; ++i) {
            const RtQuadric &q = d->quadrics[i]; DevQuadric &o = dq[i];
            if (q.type < RT_QUADRIC_SPHERE || q.type > RT_QUADRIC_HYPERBOLOID) return fail(RT_EINVAL, "rt_scene_create: unknown quadric type");
            std::memcpy(o.w2o, q.world_to_object, sizeof o.w2o); std::memcpy(o.o2w, q.object_to_world, sizeof o.o2w);
            o.radius = q.radius; o.zmin = q.zmin; o.zmax = q.zmax; o.theta_min = q.theta_min; o.theta_max = q.theta_max; o.phi_max = q.phi_max;
            o.type = q.type; o.pad = 0;
            for (int c = 0; c < 3; ++c) { o.p1[c] = q.p1[c]; o.p2[c] = q.p2[c]; }
            o.a = q.a; o.c = q.c;
        }
        if ((rc = upload(s, dq.data(), dq.size(), &s->dev.quadrics))) return rc;
    }
    tick("triangle / shading records");
    // nodes (+ one node of padding: the traversal may fetch node i+1 together with node i) and the leaf lists
    auto upload_nodes = [&](const NodeVec &v, const uint2 **dev) -> int {
        void *p = nullptr;
        if (int rc = scene_alloc(s, (v.size() + 1) * sizeof(uint2), &p)) return rc;
        if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(uint2), hipMemcpyHostToDevice));
        const uint2 pad = make_uint2(3u, 0u);
        HIPCHK(hipMemcpy((uint2 *)p + v.size(), &pad, sizeof pad, hipMemcpyHostToDevice));
        *dev = (const uint2 *)p;
        return RT_OK;
    };
    const uint2 *nodes_dev = nullptr;
    if ((rc = upload_nodes(s->tree.nodes, &nodes_dev))) return rc;
    if ((rc = upload(s, s->tree.leaf_refs.data(), s->tree.leaf_refs.size(), &s->dev.leaf_refs))) return rc;
    s->dev.nodes = nodes_dev;
    s->dev.tnodes = nodes_dev;
    if (s->facts.accel_kind == RT_ACCEL_KDTREE) {
        tick("node / leaf-list upload");
        layout_thread.join();
        if (ll_status == -2) return fail(RT_ENOMEM, "rt_scene_create: out of host memory while laying out the leaf entries");
        if (ll_status != 1) return fail(RT_EINVAL, "rt_scene_create: primitive records beyond 2^30 float4 units or leaf entries beyond 2^31");
        s->dev.leaf_runs = runs ? 1u : 0u;
        const NodeVec &tn = ll.tnodes;
        tick("leaf entries (rest)");
        if ((rc = upload_nodes(tn, &s->dev.tnodes))) return rc;
        if ((rc = upload(s, ll.lrefs.data(), ll.lrefs.size(), &s->dev.lrefs))) return rc;
        {
            const unsigned *slot_prim_dev = nullptr;
            if ((rc = upload(s, ll.slot_prim.data(), ll.slot_prim.size(), &slot_prim_dev))) return rc;
            const size_t units = ll.n_slots * RT_TRI_STRIDE + 4;            // (+ one record of padding: a lane without a primitive never loads, but the array is never empty)
            void *p = nullptr;
            if ((rc = scene_alloc(s, units * sizeof(float4), &p))) return rc;
            s->dev.ltris = (const float4 *)p;
            HIPCHK(hipMemsetAsync(p, 0, units * sizeof(float4), s->stream));
            if (ll.n_slots) hipLaunchKernelGGL(derive_leaf_records_kernel, dim3(unsigned((ll.n_slots + 255) / 256)), dim3(256), 0, s->stream, slot_prim_dev,
                                               (const DevTri *)s->dev.tris, (float4 *)p, ll.n_slots);
            HIPCHK(hipGetLastError());
            if (knob("PBRT_HIP_VERIFY_DERIVED")) {             // tests: the device fill against the host fill, byte for byte
                std::vector<float4> lt, back(units); leaf_records_fill_host(ll.slot_prim, tris, lt);
                HIPCHK(hipStreamSynchronize(s->stream));
                HIPCHK(hipMemcpy(back.data(), p, units * sizeof(float4), hipMemcpyDeviceToHost));
                if (lt.size() != units || std::memcmp(back.data(), lt.data(), units * sizeof(float4)) != 0) return fail(RT_ESTATE, "rt_scene_create: the device-built primitive records differ from the host fill");
            }
        }
        tick("primitive records (device)");
        std::vector<uint4> pairs;
        order_thread.join();
        pair_blocks_fill(tn, pbo, pairs, s->dev.root_x, s->dev.root_y);
        s->dev.top_pairs = pbo.top;
        if (pairs.empty() || pairs.size() >= (size_t(1) << 30)) return fail(RT_EINVAL, "rt_scene_create: pair records beyond 2^30");
        tick("pair blocks");
        if ((rc = upload(s, pairs.data(), pairs.size(), &s->dev.tpairs))) return rc;
        tick("pair upload");
    }
    // materials (OrenNayar constants: reflection.h:268-277)
    std::vector<DevMaterial> mats(d->n_materials);
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const RtMaterial &m = d->materials[i];
        if (m.type < RT_MAT_MATTE || m.type > RT_MAT_TRANSLUCENT) return fail(RT_EINVAL, "rt_scene_create: unknown material type");
        rt_material_resolve(&m, &mats[i]);                                        // include/pbrt_hip_texture.h: what the EXT kernels do per hit for a textured material
        if (m.type >= RT_MAT_PLASTIC) s->facts.has_ext = true;                           // plastic, uber, shinymetal, translucent: their lobes exist only in the EXT kernels
        if (m.type != RT_MAT_MATTE) s->facts.specular_materials = true;                  // mirror, glass (and the EXT materials): fixed::Scene's "no specular lobe" does not hold
    }
    if (const char *e = knob("PBRT_HIP_FIXED_SCENE")) s->facts.scene_twins = std::atoi(e) != 0;   // 0: this scene's frames take no scene twin (rt_fixed_frame.h); no value forces one
    s->materials_host = mats;                                                     // rt_scene_set_textures / rt_render: the records move when room for resolved ones is added
    if ((rc = upload(s, mats.data(), mats.size(), &s->dev.materials))) return rc;

    // lights + emitter triangles with ShapeSet area CDF (shape.h:122-135)
    std::vector<float> ltris(size_t(d->n_light_tris) * 16, 0.f);
    std::vector<DevLight> lights(d->n_lights);
    s->facts.n_lights = d->n_lights; s->facts.light_samples.assign(d->n_lights, 1);
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        const RtLight &L = d->lights[i]; DevLight &o = lights[i];
        o.type = L.type; o.n_samples = s->facts.light_samples[i] = L.n_samples < 1 ? 1 : L.n_samples;     // (the host keeps them for plan_requests)
        for (int c = 0; c < 3; ++c) { o.color[c] = L.color[c]; o.pos[c] = L.pos[c]; }
        o.first_tri = L.first_tri; o.n_tris = L.n_tris; o.reverse_orientation = L.reverse_orientation;
        o.flip_normal = L.flip_normal; o.area = 0.f;
        for (int c = 0; c < 3; ++c) o.dir[c] = L.dir[c];
        for (int c = 0; c < 9; ++c) o.w2l[c] = L.world_to_light[c];
        o.cos_total = L.cos_total_width; o.cos_falloff = L.cos_falloff_start;
        {   // LightToWorld until rt_scene_set_light_transforms brings the reference's own: the inverse of WorldToLight by cofactors
            const float a = o.w2l[0], b = o.w2l[1], c = o.w2l[2], d3 = o.w2l[3], e = o.w2l[4], f = o.w2l[5], g = o.w2l[6], h = o.w2l[7], i9 = o.w2l[8];
            const float cof[9] = {e * i9 - f * h, c * h - b * i9, b * f - c * e, f * g - d3 * i9, a * i9 - c * g, c * d3 - a * f, d3 * h - e * g, b * g - a * h, a * e - b * d3};
            for (int k = 0; k < 9; ++k) o.l2w[k] = cof[k];
            o.l2w_scale = L.type == RT_LIGHT_SPOT ? 1.f / (a * cof[0] + b * cof[3] + c * cof[6]) : 0.f;
        }
        o.quadric = L.quadric_plus1 - 1;
        if (L.quadric_plus1 < 0 || uint32_t(L.quadric_plus1) > d->n_quadrics) return fail(RT_EINVAL, "rt_scene_create: light refers to a quadric out of range");
        if (L.type < RT_LIGHT_POINT || L.type > RT_LIGHT_INFINITE) return fail(RT_EINVAL, "rt_scene_create: unknown light type");
        if (L.type == RT_LIGHT_INFINITE) { s->facts.has_ext = true; ++s->n_infinite; }      // the light's code exists only in the EXT kernels
        if (L.type != RT_LIGHT_AREA) continue;
        if (size_t(L.first_tri) + L.n_tris > d->n_light_tris) return fail(RT_EINVAL, "rt_scene_create: light triangle range out of bounds");
        float area = 0.f; std::vector<float> areas;
        for (uint32_t k = 0; k < L.n_tris; ++k) {
            const float *v = d->light_tris + size_t(L.first_tri + k) * 9;
            float *q = &ltris[size_t(L.first_tri + k) * 16];
            std::memcpy(q, v, 9 * sizeof(float));
            { float nl[3], sn_unused[3]; host_tri_frame(v, L.flip_normal != 0, nl, sn_unused); q[12] = nl[0]; q[13] = nl[1]; q[14] = nl[2]; }
            // Triangle::Area trianglemesh.cpp:329-335
            float ax = v[3] - v[0], ay = v[4] - v[1], az = v[5] - v[2];
            float bx = v[6] - v[0], by = v[7] - v[1], bz = v[8] - v[2];
            float cx = (ay * bz) - (az * by), cy = (az * bx) - (ax * bz), cz = (ax * by) - (ay * bx);
            float a = 0.5f * sqrtf(cx * cx + cy * cy + cz * cz);
            q[9] = a; area += a; areas.push_back(a);
        }
        float prev = 0.f;
        for (uint32_t k = 0; k < L.n_tris; ++k) {
            float c = prev + areas[k] / area;
            ltris[size_t(L.first_tri + k) * 16 + 10] = c; prev = c;
        }
        o.area = (L.n_tris == 1) ? areas[0] : area;
    }
    if ((rc = upload(s, lights.data(), lights.size(), &s->dev.lights))) return rc;
    s->lights_host = lights;                                                       // rt_scene_set_light_transforms rewrites the spot lights' records
    if ((rc = upload(s, ltris.data(), ltris.size(), &s->dev.light_tris))) return rc;
    {
        std::vector<unsigned> flags(d->n_lights ? d->n_lights : 1, 0u);
        s->n_drawing_lights = 0;
        for (uint32_t i = 0; i < d->n_lights; ++i) {       // ShapeSet::Sample (shape.h:115-121) draws one RandomFloat() when the emitter has several triangles
            const int draws = (d->lights[i].type == RT_LIGHT_AREA && d->lights[i].quadric_plus1 == 0 && d->lights[i].n_tris > 1) ? 1 : 0;
            if (i == 0) s->facts.light_draws = draws; else if (draws != s->facts.light_draws) s->facts.light_draws = -1;
            flags[i] = unsigned(draws); s->n_drawing_lights += unsigned(draws);
        }
        if ((rc = upload(s, flags.data(), flags.size(), &s->light_draw_flags))) return rc;      // (read by the recurrence of a "weighted" frame with lights of mixed RNG use)
    }

    s->dev.n_tris = d->n_tris; s->dev.n_lights = d->n_lights; s->dev.n_infinite = int(s->n_infinite);
    s->dev.accel_kind = s->facts.accel_kind;
    for (int a = 0; a < 3; ++a) { s->dev.nvox[a] = s->gridacc.nvox[a]; s->dev.gwidth[a] = s->gridacc.width[a]; s->dev.ginv_width[a] = s->gridacc.inv_width[a]; }
    std::memcpy(s->dev.bounds, s->tree.bounds, sizeof s->dev.bounds);
    s->dev.cam = d->camera; s->dev.vol = d->volume; s->volume = d->volume;
    {   // the rest of what the frame planners read
        plan::SceneFacts &f = s->facts;
        f.medium = d->volume.present != 0;
        f.lens_radius = d->camera.lens_radius; f.camera_type = d->camera.type;
        std::memcpy(f.bounds, s->dev.bounds, sizeof f.bounds);
        for (int a = 0; a < 3; ++a) { f.vol_p0[a] = d->volume.p0[a]; f.vol_p1[a] = d->volume.p1[a]; f.cam_pos[a] = d->camera.camera_to_world[4 * a + 3]; }   // CameraToWorld(0,0,0)
    }

    // persistent launch geometry: as many resident blocks as the kernels' registers / LDS admit (rt_host.h)
    if ((rc = size_resident_grids(s->device, s->grids, s->n_cus, s->n_threads))) return rc;
    s->spill_depth = s->tree.max_depth > RT_TRACE_STACK ? s->tree.max_depth - RT_TRACE_STACK + 1 : 1;     // RT_TRACE_STACK <= RT_STACK_LDS
    if ((rc = s->work_counter.grow(64))) return rc;             // 8 band counters, one 64-byte line each (the pipeline uses the first)
    if ((rc = s->counters.grow(64))) return rc;                 // 8 RtCounters, 16 RT_PROFILE, 2 x 16 RT_PROFILE_STAGES
    HIPCHK(hipMemsetAsync(s->counters, 0, 64 * sizeof(unsigned long long), s->stream));
    if ((rc = s->filter_dev.grow(256)) || (rc = s->dev_scene.grow(1)) || (rc = s->dev_frame.grow(1)) || (rc = s->query_frame.grow(1))) return rc;
    HIPCHK(hipMemcpy(s->dev_scene, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice));
    HIPCHK(hipEventCreate(&s->ev2.p));
    if ((rc = s->spill.grow(size_t(s->spill_depth) * s->n_threads * 2))) return rc;        // uint4 entries in the pair form, uint2 otherwise
    if ((rc = s->dev_pool.grow(1)) || (rc = s->trace_qc.grow(RT_QC_STRIDE))) return rc;
    HIPCHK(hipHostMalloc((void **)&s->h_qcount.p, size_t(RT_PIPE_QN) * RT_QC_STRIDE * sizeof(unsigned), hipHostMallocDefault));
    HIPCHK(hipStreamSynchronize(s->stream));
    guard.p = nullptr;
    *out = s;
    return RT_OK;
}

int rt_scene_destroy(RtScene *s) {
    if (!s) return RT_OK;
    HIPWARN(hipSetDevice(s->device));
    if (s->stream) hipStreamSynchronize(s->stream);
    delete s;
    return RT_OK;
}

int rt_scene_set_stream(RtScene *s, void *hip_stream) {
    if (!s) return fail(RT_EINVAL, "null scene");
    if (s->own_stream) { HIPWARN(hipStreamSynchronize(s->own_stream)); s->own_stream.reset(); }
    s->stream = static_cast<hipStream_t>(hip_stream);
    return RT_OK;
}
int rt_scene_get_stream(RtScene *s, void **hip_stream_out) {
    if (!s || !hip_stream_out) return fail(RT_EINVAL, "rt_scene_get_stream: null argument");
    *hip_stream_out = s->stream;
    return RT_OK;
}

// DensityRegion (volume.h:62-90) for the scene's medium: the region's parameters go into DevScene (read by the EXT kernels only), a grid into HBM.
int rt_scene_set_density(RtScene *s, const RtDensityRegion *r) {
    if (!s || !r) return fail(RT_EINVAL, "rt_scene_set_density: null argument");
    if (s->rendered) return fail(RT_ESTATE, "rt_scene_set_density: the scene has rendered a frame already");
    if (s->facts.density_kind != RT_DENSITY_NONE) return fail(RT_ESTATE, "rt_scene_set_density: the scene has a density region already");
    if (!s->volume.present) return fail(RT_EINVAL, "rt_scene_set_density: the scene has no medium (RtSceneDesc.volume.present == 0)");
    if (r->kind != RT_DENSITY_EXPONENTIAL && r->kind != RT_DENSITY_GRID) return fail(RT_EINVAL, "rt_scene_set_density: unknown density kind");
    // the volume's world bound, WorldToVolume.GetInverse()(extent) (exponential.cpp:38, volumegrid.cpp:36): its corners through the inverse, in double
    double a[4][8];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { a[i][j] = s->volume.world_to_volume[4 * i + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < 4; ++c) {                                               // Gauss-Jordan with partial pivoting
        int piv = c;
        for (int i = c + 1; i < 4; ++i) if (std::fabs(a[i][c]) > std::fabs(a[piv][c])) piv = i;
        if (!(std::fabs(a[piv][c]) > 0.0)) return fail(RT_EINVAL, "rt_scene_set_density: singular world_to_volume");
        for (int j = 0; j < 8; ++j) std::swap(a[c][j], a[piv][j]);
        const double inv = 1.0 / a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] *= inv;
        for (int i = 0; i < 4; ++i) if (i != c) { const double f = a[i][c]; for (int j = 0; j < 8; ++j) a[i][j] -= f * a[c][j]; }
    }
    double wb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 8; ++k) {
        const double q[3] = {(k & 1) ? s->volume.p1[0] : s->volume.p0[0], (k & 2) ? s->volume.p1[1] : s->volume.p0[1], (k & 4) ? s->volume.p1[2] : s->volume.p0[2]};
        double w[4];
        for (int i = 0; i < 4; ++i) w[i] = a[i][4] * q[0] + a[i][5] * q[1] + a[i][6] * q[2] + a[i][7];
        for (int i = 0; i < 3; ++i) { const double v = w[3] != 1.0 ? w[i] / w[3] : w[i]; wb[i] = std::min(wb[i], v); wb[3 + i] = std::max(wb[3 + i], v); }
    }
    for (double v : wb) if (!std::isfinite(v)) return fail(RT_EINVAL, "rt_scene_set_density: the volume's world bound is not finite");
    HIPCHK(hipSetDevice(s->device));
    const float *grid = nullptr;
    if (r->kind == RT_DENSITY_GRID) {
        const long long total = (long long)r->nx * r->ny * r->nz;
        if (r->nx <= 0 || r->ny <= 0 || r->nz <= 0 || total > 0x7fffffffLL) return fail(RT_EINVAL, "rt_scene_set_density: grid counts must be positive with nx*ny*nz < 2^31");
        if (!r->density) return fail(RT_EINVAL, "rt_scene_set_density: null density grid");
        int rc = upload(s, r->density, size_t(total), &grid); if (rc) return rc;
    }
    DevScene &d = s->dev;
    d.dens_kind = r->kind; d.dens_a = r->a; d.dens_b = r->b;
    for (int i = 0; i < 3; ++i) d.dens_up[i] = r->updir[i];
    d.dens_n[0] = r->nx; d.dens_n[1] = r->ny; d.dens_n[2] = r->nz; d.dens_grid = grid;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(s->dev_scene, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice));
    std::memcpy(s->facts.vol_world, wb, sizeof wb);
    s->facts.density_kind = r->kind;
    s->facts.has_ext = true;                                                          // the density code exists only in the EXT kernels
    return RT_OK;
}

// The spot lights' LightToWorld as the reference holds it (pbrt_hip.h): 9 floats per light of the scene, read for the spot lights only.
int rt_scene_set_light_transforms(RtScene *s, const float *light_to_world, uint32_t n_lights) {
    if (!s || !light_to_world) return fail(RT_EINVAL, "rt_scene_set_light_transforms: null argument");
    if (s->rendered) return fail(RT_ESTATE, "rt_scene_set_light_transforms: the scene has rendered a frame already");
    if (n_lights != s->lights_host.size()) return fail(RT_EINVAL, "rt_scene_set_light_transforms: n_lights differs from the scene's number of lights");
    for (uint32_t i = 0; i < n_lights; ++i) {
        if (s->lights_host[i].type != RT_LIGHT_SPOT) continue;
        for (int k = 0; k < 9; ++k) if (!std::isfinite(light_to_world[9 * size_t(i) + k])) return fail(RT_EINVAL, "rt_scene_set_light_transforms: a matrix entry is not finite");
    }
    if (n_lights == 0) return RT_OK;
    for (uint32_t i = 0; i < n_lights; ++i) {
        DevLight &o = s->lights_host[i];
        if (o.type != RT_LIGHT_SPOT) continue;
        for (int k = 0; k < 9; ++k) o.l2w[k] = light_to_world[9 * size_t(i) + k];
        o.l2w_scale = 1.f;
    }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(const_cast<DevLight *>(s->dev.lights), s->lights_host.data(), s->lights_host.size() * sizeof(DevLight), hipMemcpyHostToDevice));
    return RT_OK;
}

// Textured material parameters (pbrt_hip.h, include/pbrt_hip_texture.h).  Everything is checked before anything is uploaded: every index, kind and
// mapping, the value type of every child and slot, children strictly below their parents (no cycle can be written that way), and per parameter the
// length of its post-order program and the stack it needs.
int rt_scene_set_textures(RtScene *s, const RtTexture *nodes, uint32_t n_nodes, const RtMaterialTextures *mats, uint32_t n_mats) {
    if (!s || !nodes || !mats) return fail(RT_EINVAL, "rt_scene_set_textures: null argument");
    if (s->rendered) return fail(RT_ESTATE, "rt_scene_set_textures: the scene has rendered a frame already");
    if (s->has_textures) return fail(RT_ESTATE, "rt_scene_set_textures: the scene has textures already");
    if (n_nodes == 0 || n_nodes > RT_TEX_MAX_NODES) return fail(RT_EINVAL, "rt_scene_set_textures: the number of texture nodes must be 1 .. " + std::to_string(RT_TEX_MAX_NODES));
    if (n_mats != s->materials_host.size()) return fail(RT_EINVAL, "rt_scene_set_textures: n_mats differs from the scene's number of materials");
    if (n_mats > 65534u) return fail(RT_EINVAL, "rt_scene_set_textures: more than 65534 materials");
    return guarded("rt_scene_set_textures", [&]() -> int {
        for (uint32_t i = 0; i < n_nodes; ++i) {
            const RtTexture &t = nodes[i];
            const std::string at = "rt_scene_set_textures: node " + std::to_string(i) + ": ";
            if (t.kind < 0 || t.kind >= RT_TEX_KIND_COUNT) return fail(RT_EINVAL, at + "unknown texture kind");
            if (t.is_color != 0 && t.is_color != 1) return fail(RT_EINVAL, at + "is_color must be 0 or 1");
            if (t.kind == RT_TEX_UV && !t.is_color) return fail(RT_EINVAL, at + "the uv texture is a colour texture");
            const bool mapped = t.kind == RT_TEX_BILERP || t.kind == RT_TEX_UV || t.kind == RT_TEX_CHECKERBOARD;
            if (mapped && (t.mapping < 0 || t.mapping >= RT_TEXMAP_COUNT)) return fail(RT_EINVAL, at + "unknown mapping");
            const int n_child = (t.kind == RT_TEX_SCALE || t.kind == RT_TEX_CHECKERBOARD) ? 2 : t.kind == RT_TEX_MIX ? 3 : 0;
            for (int c = 0; c < 3; ++c) {
                const int32_t ch = t.child[c];
                if (c >= n_child) { if (ch != -1) return fail(RT_EINVAL, at + "a child index where the kind takes none (must be -1)"); continue; }
                if (ch < 0 || uint32_t(ch) >= n_nodes) return fail(RT_EINVAL, at + "child index out of range");
                if (uint32_t(ch) >= i) return fail(RT_EINVAL, at + "a child must precede its parent in the table (a cycle, or a table out of order)");
                const int want_color = (c == 2) ? 0 : t.is_color;                  // amount is a float texture; tex1 / tex2 have the node's type
                if (nodes[ch].is_color != want_color) return fail(RT_EINVAL, at + "child of the wrong value type (float / color)");
            }
        }
        // post-order programs: tree size and stack need per node (children are below their parents, so one forward pass)
        std::vector<uint32_t> size(n_nodes), need(n_nodes);
        for (uint32_t i = 0; i < n_nodes; ++i) {
            const RtTexture &t = nodes[i];
            uint64_t sz = 1; uint32_t nd = 1, held = 0;
            for (int c = 0; c < 3; ++c) if (t.child[c] >= 0) { sz += size[t.child[c]]; nd = std::max(nd, held + need[t.child[c]]); ++held; }
            size[i] = uint32_t(std::min<uint64_t>(sz, 1u << 20)); need[i] = nd;
        }
        std::vector<DevMatTex> dm(n_mats);
        std::vector<int> prog;
        uint32_t n_textured = 0;
        for (uint32_t i = 0; i < n_mats; ++i) {
            const RtMaterialTextures &m = mats[i]; DevMatTex &o = dm[i];
            const std::string at = "rt_scene_set_textures: material " + std::to_string(i) + ": ";
            if (m.raw.type != s->materials_host[i].type) return fail(RT_EINVAL, at + "type differs from the scene's material");
            o.raw = m.raw; o.textured = 0;
            for (int k = 0; k < RT_MATSLOT_COUNT; ++k) {
                o.prog_off[k] = 0; o.prog_len[k] = 0;
                const int32_t root = m.tex[k];
                if (root == -1) continue;
                if (root < 0 || uint32_t(root) >= n_nodes) return fail(RT_EINVAL, at + "texture index out of range");
                if (nodes[root].is_color != (k == RT_MATSLOT_F ? 0 : 1)) return fail(RT_EINVAL, at + "texture of the wrong value type for its slot (float / color)");
                if (size[root] > RT_TEX_MAX_PROGRAM) return fail(RT_EINVAL, at + "a parameter's texture graph has more than " + std::to_string(RT_TEX_MAX_PROGRAM) + " nodes");
                if (need[root] > RT_TEX_MAX_STACK) return fail(RT_EINVAL, at + "a parameter's texture graph needs more than " + std::to_string(RT_TEX_MAX_STACK) + " values at once");
                o.prog_off[k] = int(prog.size());
                struct Walk { static void go(const RtTexture *nodes, int n, std::vector<int> &out) { for (int c = 0; c < 3; ++c) if (nodes[n].child[c] >= 0) go(nodes, nodes[n].child[c], out); out.push_back(n); } };
                Walk::go(nodes, root, prog);
                o.prog_len[k] = int(prog.size()) - o.prog_off[k];
                o.textured = 1;
            }
            n_textured += uint32_t(o.textured);
        }
        HIPCHK(hipSetDevice(s->device));
        const RtTexture *dnodes = nullptr; const int *dprog = nullptr; const DevMatTex *dmt = nullptr;
        int rc;
        if ((rc = upload(s, nodes, size_t(n_nodes), &dnodes))) return rc;
        if ((rc = upload(s, prog.data(), prog.size(), &dprog))) return rc;
        if ((rc = upload(s, dm.data(), dm.size(), &dmt))) return rc;
        HIPCHK(hipStreamSynchronize(s->stream));
        if (n_textured && s->n_tris) {                                          // mark the primitives of textured materials (RT_PRIM_TEXTURED in the word make_vertex reads)
            std::vector<float4> shade(size_t(2) * s->n_tris);
            HIPCHK(hipMemcpy(shade.data(), s->dev.tri_shade, shade.size() * sizeof(float4), hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < s->n_tris; ++i) {
                uint32_t bits; std::memcpy(&bits, &shade[2 * size_t(i)].w, 4);
                if (dm[bits & 0xffffu].textured) { bits |= RT_PRIM_TEXTURED; std::memcpy(&shade[2 * size_t(i)].w, &bits, 4); }
            }
            HIPCHK(hipMemcpy(const_cast<float4 *>(s->dev.tri_shade), shade.data(), shade.size() * sizeof(float4), hipMemcpyHostToDevice));
        }
        DevScene &d = s->dev;
        d.n_textured = int(n_textured); d.tex_nodes = dnodes; d.tex_prog = dprog; d.mat_tex = dmt;
        if (n_textured) { if ((rc = upload_tex_uv(s))) return rc; }             // the per-vertex uvs of the meshes that have them (copies the scene record too)
        HIPCHK(hipMemcpy(s->dev_scene, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice));
        s->has_textures = true;
        s->facts.has_ext = true;                                                      // the evaluator exists only in the EXT kernels
        return RT_OK;
    });
}
}  // extern "C"
// The uvs rt_scene_create kept on the host (6 floats per triangle of a mesh with "uv"), uploaded once: by rt_scene_set_textures for a scene with a textured
// material, by rt_render before the first debug frame (dg.u / dg.v, hit_point_uv).  Nothing to do when no mesh has "uv" or they are on the device already.
int upload_tex_uv(RtScene *s) {
    if (s->tex_uv_idx_host.empty() || s->dev.tex_uv_idx) return RT_OK;
    const int *duvi = nullptr; const float *duv = nullptr;
    int rc;
    if ((rc = upload(s, s->tex_uv_idx_host.data(), s->tex_uv_idx_host.size(), &duvi))) return rc;
    if ((rc = upload(s, s->tex_uv_host.data(), s->tex_uv_host.size(), &duv))) return rc;
    std::vector<int>().swap(s->tex_uv_idx_host); std::vector<float>().swap(s->tex_uv_host);
    HIPCHK(hipStreamSynchronize(s->stream));                                    // (a frame queued earlier reads the scene record)
    s->dev.tex_uv_idx = duvi; s->dev.tex_uv = duv;
    HIPCHK(hipMemcpy(s->dev_scene, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice));
    return RT_OK;
}
// room for the per-hit records: [the scene's materials | levels * n_slots resolved ones].  Called by rt_render before its first launch.
int ensure_material_pool(RtScene *s, DevFrame &fr, size_t levels, size_t n_slots) {
    fr.mat_pool_base = 0;
    if (!s->has_textures || s->dev.n_textured == 0) return RT_OK;
    const size_t base = s->materials_host.size(), need = levels * n_slots;
    if (base + need >= (size_t(1) << 31)) return fail(RT_EINVAL, "rt_render: more than 2^31 resolved-material records (threads x recursion levels)");
    if (base + need > s->mat_buf.cap) {
        HIPCHK(hipStreamSynchronize(s->stream));
        DevBuf<DevMaterial> nb;                                // (the old block goes once the new one exists: dev.materials never dangles)
        if (int rc = nb.grow(base + need)) return rc;
        s->mat_buf = std::move(nb);
        HIPCHK(hipMemcpy(s->mat_buf, s->materials_host.data(), base * sizeof(DevMaterial), hipMemcpyHostToDevice));
        s->dev.materials = s->mat_buf;
        HIPCHK(hipMemcpy(s->dev_scene, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice));
    }
    fr.mat_pool_base = unsigned(base);
    return RT_OK;
}
extern "C" {

int rt_scene_accel_info(const RtScene *s, RtAccelInfo *info) {
    if (!s || !info) return fail(RT_EINVAL, "null argument");
    fill_info(s->tree, s->gridacc, s->facts.accel_kind, s->n_tris, info);
    return RT_OK;
}

int rt_scene_accel_copy(const RtScene *s, uint32_t *nodes, uint32_t *leaf_refs) {
    if (!s) return fail(RT_EINVAL, "null scene");
    if (nodes) std::memcpy(nodes, s->tree.nodes.data(), s->tree.nodes.size() * sizeof(Node));
    if (leaf_refs) std::memcpy(leaf_refs, s->tree.leaf_refs.data(), s->tree.leaf_refs.size() * sizeof(uint32_t));
    return RT_OK;
}

struct RtKdTree { KdTree tree; GridAccelData grid; int kind = RT_ACCEL_KDTREE; uint32_t n_tris = 0; };
static void fill_info(const KdTree &tree, const GridAccelData &g, int kind, uint32_t n_tris, RtAccelInfo *info) {
    info->n_nodes = uint32_t(tree.nodes.size()); info->n_leaf_refs = uint32_t(tree.leaf_refs.size());
    info->max_depth = uint32_t(tree.max_depth); info->n_tris = n_tris;
    std::memcpy(info->bounds, tree.bounds, sizeof info->bounds); info->build_seconds = tree.build_seconds;
    info->kind = kind;
    for (int a = 0; a < 3; ++a) {
        info->grid_nvoxels[a] = kind == RT_ACCEL_GRID ? g.nvox[a] : 0;
        info->grid_width[a] = kind == RT_ACCEL_GRID ? g.width[a] : 0.f;
        info->grid_inv_width[a] = kind == RT_ACCEL_GRID ? g.inv_width[a] : 0.f;
    }
}
int rt_accel_build(const float *tri_verts, uint32_t n_tris, const RtAccelParams *params, RtAccel **out) {
    if (!out || (n_tris && !tri_verts)) return fail(RT_EINVAL, "rt_accel_build: null argument");
    RtAccelParams p; std::memset(&p, 0, sizeof p);
    if (params) p = *params;
    if (p.kind != RT_ACCEL_GRID && p.kind != RT_ACCEL_KDTREE) return fail(RT_EINVAL, "rt_accel_build: unknown accelerator kind");
    return guarded("rt_accel_build", [&] {
        std::unique_ptr<RtKdTree> t(new RtKdTree()); t->n_tris = n_tris; t->kind = p.kind;
        if (p.kind == RT_ACCEL_GRID) {
            build_grid(tri_verts, n_tris, t->grid);
            t->tree.nodes = t->grid.voxels; t->tree.leaf_refs = t->grid.refs; t->tree.max_depth = 0;
            std::memcpy(t->tree.bounds, t->grid.bounds, sizeof t->tree.bounds); t->tree.build_seconds = t->grid.build_seconds;
        } else build_kdtree(tri_verts, n_tris, p, t->tree);
        *out = t.release(); return RT_OK;
    });
}
int rt_accel_info(const RtAccel *t, RtAccelInfo *info) {
    if (!t || !info) return fail(RT_EINVAL, "null argument");
    fill_info(t->tree, t->grid, t->kind, t->n_tris, info);
    return RT_OK;
}
int rt_accel_copy(const RtAccel *t, uint32_t *nodes, uint32_t *leaf_refs) {
    if (!t) return fail(RT_EINVAL, "null accelerator");
    if (nodes) std::memcpy(nodes, t->tree.nodes.data(), t->tree.nodes.size() * sizeof(Node));
    if (leaf_refs) std::memcpy(leaf_refs, t->tree.leaf_refs.data(), t->tree.leaf_refs.size() * sizeof(uint32_t));
    return RT_OK;
}
int rt_accel_destroy(RtAccel *t) { delete t; return RT_OK; }
// The leaf layout rt_scene_create derives from a kd-tree (leaf_layout.cpp), on the host alone: what the CPU tests check the entry encoding with.
int rt_accel_leaf_layout(const RtAccel *t, int runs, int copies, uint32_t *tnodes, uint32_t *slot_prim, uint32_t *entries, RtLeafLayoutInfo *info) {
    if (!t || !info) return fail(RT_EINVAL, "rt_accel_leaf_layout: null argument");
    if (t->kind != RT_ACCEL_KDTREE) return fail(RT_EINVAL, "rt_accel_leaf_layout: not a kd-tree");
    return guarded("rt_accel_leaf_layout", [&] {
        LeafLayout ll;
        if (!leaf_cursor_layout(t->tree.nodes, t->tree.leaf_refs, t->n_tris, copies != 0, runs != 0, ll)) return fail(RT_EINVAL, "rt_accel_leaf_layout: primitive records beyond 2^30 float4 units or leaf entries beyond 2^31");
        info->n_nodes = ll.tnodes.size(); info->n_slots = ll.n_slots; info->n_entries = ll.lrefs.size(); info->stride = RT_TRI_STRIDE;
        if (tnodes && !ll.tnodes.empty()) std::memcpy(tnodes, ll.tnodes.data(), ll.tnodes.size() * sizeof(Node));
        if (slot_prim && ll.n_slots) std::memcpy(slot_prim, ll.slot_prim.data(), ll.n_slots * sizeof(uint32_t));
        if (entries) std::memcpy(entries, ll.lrefs.data(), ll.lrefs.size() * sizeof(uint32_t));
        return int(RT_OK);
    });
}
int rt_kdtree_build(const float *tri_verts, uint32_t n_tris, const RtAccelParams *params, RtKdTree **out) {
    if (params && params->kind != RT_ACCEL_KDTREE) return fail(RT_EINVAL, "rt_kdtree_build: not a kd-tree description");
    return rt_accel_build(tri_verts, n_tris, params, out);
}
int rt_kdtree_info(const RtKdTree *t, RtAccelInfo *info) { return rt_accel_info(t, info); }
int rt_kdtree_copy(const RtKdTree *t, uint32_t *nodes, uint32_t *leaf_refs) { return rt_accel_copy(t, nodes, leaf_refs); }
int rt_kdtree_destroy(RtKdTree *t) { return rt_accel_destroy(t); }

}  // extern "C"
