"""Degenerate caller-supplied rays: three small scenes and a table of ray classes (plain numpy, seeded), for tests/golden/make_edge_rays_golden.py
(which holds them against the reference's Scene::Intersect / IntersectP through oracle/ref/rayfile_integrator.cpp), tests/test_edge_rays_host.py
and tests/test_gpu_edge_rays.py.  Every ray here is "usable" for rt_ray_guard.h: finite, d != 0.  Coordinates and t stay below 2^10 except in
class (h)."""
import re

import numpy as np

SCENES = ("lattice", "cornell", "quadrics")
ACCELS = ("kdtree", "grid")
FIXTURES = ["edge_%s_%s" % (s, a) for s in SCENES for a in ACCELS]

# class -> the one-line reason it is in the table
CLASSES = {
    "a": "axis-aligned d from generic origins, the two zero components in every combination of +0.f and -0.f: 0 * inf in the slab test, x / 0 in the DDA",
    "b": "a zero-direction (or travel) coordinate of o bit-equal to a stored kd split of the top three levels: tplane NaN / +-inf, belowFirst on o == split",
    "c": "o exactly on a face, an edge and a corner of the world bound, pointing inwards, outwards and along the face: the grid's inside test with <=",
    "d": "o inside the bound with mint = 0, with a mint that puts o + d * mint outside the bound (the grid's other branch) and with negative mint",
    "e": "o bit-equal to a voxel boundary lo + k * width (float32, as the grid computes it), that direction component zero and non-zero",
    "f": "rays in the plane of a triangle (divisor == 0), through a shared edge, through a vertex shared by six or more, and from a point on a triangle with mint = 0",
    "g": "maxt = t, nextafter below t, mint = t, nextafter above t, maxt = +inf, mint == maxt, mint > maxt around the reference's own t of a first pass",
    "h": "d scaled by 2^k (k in -60, -20, 20, 60) with mint, maxt scaled by 2^-k, and d scaled into the denormal range where 1 / d overflows",
    "i": "quadrics: along the object z axis through a pole, the cone's apex and the disk's centre; in the plane y = +-0 across the phi = 0 seam; tangent rays",
}
CODES = "abcdefghi"
# where the reference is not a usable spec: the rays stay in the fixtures and are held to "no fault, position independence" only (INTEGRATION.md, next
# to the ray guard)
OUTSIDE_CONTRACT = {
    "h": "grid only: a denormal d from an origin outside the world bound -- 1 / d = inf makes the slab test's rayT = +inf, the grid's entry point "
         "o + d * rayT is +-inf or NaN, and PosToVoxel converts it to int, which C leaves undefined (x86 gives INT_MIN -> voxel 0, the GPU saturates "
         "to INT_MAX -> the last voxel): the two walk different voxel columns",
}

MAXT = np.float32(1000.0)
H_SCALES = (-60, -20, 20, 60)
H_DENORMAL = -140                 # 2^-140 * |d| is a float32 denormal: 1 / d overflows to +-inf
POINT_LIGHT = {"lattice": (8.5, 15.5, 0.5), "cornell": (278, 540, 280), "quadrics": (8.5, 8.5, -6)}


# ------------------------------------------------------------------------------------------------------------------ scenes
def _fmt(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, np.float32).ravel())


def lattice_tris():
    """About 300 triangles over [0, 16]^3 whose vertices are small integers: three planes of 4 x 4 axis-aligned two-triangle quads (every inner vertex
    of a plane is shared by six triangles), seeded small axis-aligned quads and seeded slanted triangles."""
    rng = np.random.default_rng(11)
    tris = []

    def quad(p, eu, ev):
        a, b, c, d = p, p + eu, p + eu + ev, p + ev
        tris.extend([(a, b, c), (a, c, d)])
    E = np.eye(3)
    for axis, at in ((2, 8), (0, 6), (1, 10)):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for i in range(4):
            for j in range(4):
                quad(E[axis] * at + E[u] * 4 * i + E[v] * 4 * j, 4 * E[u], 4 * E[v])
    for _ in range(70):
        axis = int(rng.integers(3))
        u, v = (axis + 1) % 3, (axis + 2) % 3
        p = rng.integers(0, 15, 3).astype(np.float64)
        su, sv = (min(int(s), 16 - int(p[k])) for s, k in zip(rng.integers(1, 4, 2), (u, v)))
        quad(p, su * E[u], sv * E[v])
    n = 0
    while n < 56:
        t = rng.integers(1, 13, 3) + rng.integers(0, 4, (3, 3))
        if np.abs(np.cross(t[1] - t[0], t[2] - t[0])).sum() == 0:
            continue
        tris.append(tuple(t.astype(np.float64)))
        n += 1
    return np.array(tris, np.float32)


def _mesh(tv):
    tv = np.asarray(tv, np.float32).reshape(-1, 3)
    return 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n' % (" ".join(str(i) for i in range(len(tv))), _fmt(tv))


def _cornell_world():
    """the geometry of tests/golden/probe_cornell.npz (walls on coordinate planes), its emitter as a plain matte quad"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_cornell.npz"))
    text = str(g["scene"])
    world = text[text.index("WorldBegin") + len("WorldBegin\n"):text.index("WorldEnd")]
    return re.sub(r'^\s*AreaLightSource.*\n', "", world, flags=re.M)


QUADRICS = (      # (shape statement, integer translation)
    ('Shape "sphere" "float radius" [1.5]', (3, 3, 3)),
    ('Shape "cylinder" "float radius" [1] "float zmin" [-1] "float zmax" [1]', (8, 3, 3)),
    ('Shape "cone" "float radius" [1] "float height" [2]', (13, 3, 3)),
    ('Shape "disk" "float height" [0] "float radius" [1.5] "float innerradius" [0.5]', (3, 8, 3)),
    ('Shape "paraboloid" "float radius" [1] "float zmin" [0] "float zmax" [2]', (8, 8, 3)),
    ('Shape "hyperboloid" "point p1" [1 0 -1] "point p2" [1 1 1]', (13, 8, 3)),
    ('Shape "sphere" "float radius" [1.5] "float zmin" [-1] "float zmax" [1] "float phimax" [270]', (3, 13, 3)),
)


def world_text(scene):
    light = 'LightSource "point" "point from" [%s] "color I" [40 40 40]\n' % " ".join(str(v) for v in POINT_LIGHT[scene])
    mat = 'Material "matte" "color Kd" [0.5 0.5 0.5]\n'
    if scene == "lattice":
        return light + mat + _mesh(lattice_tris())
    if scene == "cornell":
        return light.replace("40 40 40", "400000 400000 400000") + _cornell_world()
    out = light + mat
    for shape, at in QUADRICS:
        out += "AttributeBegin\nTranslate %d %d %d\n%s\nAttributeEnd\n" % (at + (shape,))
    # the unit quad behind them
    out += 'AttributeBegin\nTranslate 1 1 7\nScale 14 14 1\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 0 1 0 0 1 1 0 0 1 0]\nAttributeEnd\n'
    return out


def scene_text(scene, accel, rays="rays.bin", dump="hits.bin"):
    """the text the reference runs: a 2 x 2 film, SurfaceIntegrator "rayfile" """
    eye = {"lattice": "8 8 -40  8 8 8", "cornell": "278 273 -800  278 273 0", "quadrics": "8 8 -40  8 8 3"}[scene]
    return ('LookAt %s  0 1 0\nCamera "perspective" "float fov" [40]\n'
            'Film "image" "integer xresolution" [2] "integer yresolution" [2] "string filename" ["out.exr"]\n'
            'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\nPixelFilter "box"\n'
            'SurfaceIntegrator "rayfile" "string rays" ["%s"] "string dump" ["%s"]\n%s\nWorldBegin\n%sWorldEnd\n'
            % (eye, rays, dump, ACCEL_LINE[accel], world_text(scene)))


def product_text(text, res=2):
    """what the product parses: Whitted in place of the reference-side plugin, and a film of res x res (DeviceScene.radiance numbers its rays as the
    frame's camera samples, so a query of n rays needs a frame of at least n samples)"""
    text = re.sub(r'^SurfaceIntegrator "rayfile".*$', 'SurfaceIntegrator "whitted"', str(text), flags=re.M)
    text = text.replace('"integer xresolution" [2] "integer yresolution" [2]', '"integer xresolution" [%d] "integer yresolution" [%d]' % (res, res))
    assert text.count('SurfaceIntegrator "whitted"') == 1 and ("[%d]" % res) in text
    return text


# the device's grid is the eager flat one (grid_build.cpp); the reference's default is a lazily refined two-level grid (whole meshes in the top grid, a
# nested grid per mesh), which the same rays in general position cannot tell from it but a ray that walks on -inf or NaN crossings can: the
# reference is asked for the structure the device builds
ACCEL_LINE = {"kdtree": 'Accelerator "kdtree"', "grid": 'Accelerator "grid" "bool refineimmediately" ["true"]'}


def with_accel(text, accel):
    out = re.sub(r'^Accelerator .*$', ACCEL_LINE[accel], str(text), flags=re.M)
    assert out.count(ACCEL_LINE[accel]) == 1
    return out


# ------------------------------------------------------------------------------------------------------------------ what the host builds
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def top_splits(nodes, levels=3):
    """[(axis, stored split as float32)] of the interior nodes of the top `levels` levels of a host-built kd-tree (rt_accel_copy's node words: word 0 =
    the split's bits with the axis in the two low mantissa bits, 3 = leaf; word 1 = the above child; the below child follows its parent)"""
    out, level = [], [0]
    for _ in range(levels):
        nxt = []
        for n in level:
            w = int(nodes[n, 0])
            if (w & 3) == 3:
                continue
            out.append((w & 3, np.array([w], np.uint32).view(np.float32)[0]))
            nxt += [n + 1, int(nodes[n, 1])]
        level = nxt
    return out


def voxel_boundary(info, axis, k):
    """lo + k * width in float32, as grid_begin / VoxelToPos compute it"""
    return np.float32(np.float32(info.bounds[axis]) + np.float32(np.float32(k) * np.float32(info.grid_width[axis])))


def accel_of(pkg, text, accel):
    ps = pkg.ParsedScene(text=product_text(with_accel(text, accel)))
    assert ps.valid and ps.errors == 0
    nodes, refs, bounds, info = ps.kdtree()
    assert info.kind == (1 if accel == "grid" else 0)
    return ps, nodes, refs, bounds, info


def class_b_on_split(rec, nodes):
    """per ray: some coordinate of o is bit-equal to a stored split of that axis among the top three levels"""
    ok = np.zeros(len(rec), bool)
    for axis, s in top_splits(nodes):
        ok |= bits(rec[:, axis]) == bits(s)
    return ok


def class_e_on_voxel_boundary(rec, info):
    ok = np.zeros(len(rec), bool)
    for axis in range(3):
        for k in range(info.grid_nvoxels[axis] + 1):
            ok |= bits(rec[:, axis]) == bits(voxel_boundary(info, axis, k))
    return ok


def class_c_on_bound(rec, bounds):
    ok = np.zeros(len(rec), bool)
    for axis in range(3):
        ok |= (bits(rec[:, axis]) == bits(bounds[axis])) | (bits(rec[:, axis]) == bits(bounds[3 + axis]))
    return ok


def outside_contract(rec, cls, h_k, bounds, accel):
    """the rays of OUTSIDE_CONTRACT, from the fixture and the world bound alone"""
    pm = rec[:, 0:3] + rec[:, 3:6] * rec[:, 6:7]
    inside = ((pm >= bounds[:3]) & (pm <= bounds[3:])).all(1)
    return (cls == CODES.index("h")) & (h_k == H_DENORMAL) & ~inside & (accel == "grid")


def zero_components(rec):
    return (rec[:, 3:6] == 0).sum(1)


# ------------------------------------------------------------------------------------------------------------------ the rays
class _Rays:
    def __init__(self):
        self.rows, self.cls, self.base, self.k = [], [], [], []

    def add(self, c, o, d, mint=0.0, maxt=MAXT, base=-1, k=0):
        r = np.zeros(8, np.float32)
        r[0:3], r[3:6], r[6], r[7] = o, d, mint, maxt
        self.rows.append(r); self.cls.append(CODES.index(c)); self.base.append(base); self.k.append(k)
        return len(self.rows) - 1

    def arrays(self):
        return (np.array(self.rows, np.float32).reshape(-1, 8), np.array(self.cls, np.uint8), np.array(self.base, np.int16), np.array(self.k, np.int16))


def _axis_dir(axis, sign, z1=0.0, z2=0.0):
    d = np.zeros(3, np.float32)
    d[axis] = sign
    d[(axis + 1) % 3], d[(axis + 2) % 3] = z1, z2
    return d


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum())).astype(np.float32)


def first_pass(pkg, scene, accel, text):
    """classes a-f, h, i and the seeds of g: (rays [n, 8], class codes, h_base, h_k).  The kd splits are those of the scene's kd-tree and the voxel
    boundaries those of its grid, whichever accelerator the fixture is for; the world bound is the fixture's own accelerator's."""
    rng = np.random.default_rng({"lattice": 1, "cornell": 2, "quadrics": 3}[scene] * 10 + ACCELS.index(accel))
    ps, kd_nodes, _, _, _ = accel_of(pkg, text, "kdtree")
    _, _, _, _, grid = accel_of(pkg, text, "grid")
    _, _, _, bounds, _ = accel_of(pkg, text, accel)
    tv = ps.tri_verts().astype(np.float32)
    tv = tv[np.abs(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])).sum(1) > 0]      # (a quadric's slot holds its bound's corners: no triangle)
    lo, hi = bounds[:3].astype(np.float64), bounds[3:].astype(np.float64)
    ext = hi - lo
    R = _Rays()
    NEG0 = np.float32(-0.0)

    def generic(margin=0.0):
        return (lo - margin * ext + rng.uniform(0.03, 0.97, 3) * ext * (1 + 2 * margin)).astype(np.float32)

    def oblique():
        d = rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
        return _unit(d)

    def towards(o, target):
        return _unit(np.asarray(target, np.float64) - np.asarray(o, np.float64))

    # a. axis-aligned, every sign of zero
    for axis in range(3):
        for sign in (1.0, -1.0):
            for z1 in (0.0, NEG0):
                for z2 in (0.0, NEG0):
                    for inside in (False, True):                              # one origin in front of the bound, one inside it
                        o = generic()
                        if not inside:
                            o[axis] = np.float32((lo[axis] - 0.137 * ext[axis]) if sign > 0 else (hi[axis] + 0.137 * ext[axis]))
                        R.add("a", o, _axis_dir(axis, sign, z1, z2))
    # b. on a stored split of the top three levels
    for s_axis, s in top_splits(kd_nodes):
        for t_axis in ((s_axis + 1) % 3, (s_axis + 2) % 3):                  # travel along another axis: the split axis' direction component is a zero
            for sign in (1.0, -1.0):
                o = generic(); o[s_axis] = s
                o[t_axis] = np.float32((lo[t_axis] - 0.11 * ext[t_axis]) if sign > 0 else (hi[t_axis] + 0.11 * ext[t_axis]))
                d = _axis_dir(t_axis, sign)
                d[s_axis] = NEG0 if rng.random() < 0.5 else 0.0
                R.add("b", o, d)
        for sign in (1.0, -1.0):                                             # travel along the split axis from the split plane
            o = generic(); o[s_axis] = s
            R.add("b", o, _axis_dir(s_axis, sign, NEG0 if sign > 0 else 0.0, 0.0))
            d = oblique(); d[s_axis] = np.float32(sign * abs(d[s_axis]))
            o = generic(); o[s_axis] = s
            R.add("b", o, d)
    # c. on a face, an edge, a corner of the world bound
    for axis in range(3):
        for side, b in ((0, lo), (1, hi)):
            inward = 1.0 if side == 0 else -1.0
            o = generic(); o[axis] = np.float32(b[axis])
            R.add("c", o, _axis_dir(axis, inward))
            R.add("c", o, _axis_dir(axis, -inward))
            R.add("c", o, _axis_dir((axis + 1) % 3, 1.0, 0.0, NEG0))          # along the face
            d = oblique(); d[axis] = np.float32(inward * abs(d[axis]))
            R.add("c", o, d)
            d = d.copy(); d[axis] = -d[axis]
            R.add("c", o, d)
    for axis in range(3):                                                     # the four edges parallel to `axis`
        for s1 in (0, 1):
            for s2 in (0, 1):
                u, v = (axis + 1) % 3, (axis + 2) % 3
                o = generic(); o[u] = np.float32((lo, hi)[s1][u]); o[v] = np.float32((lo, hi)[s2][v])
                R.add("c", o, _axis_dir(axis, 1.0 if s1 == s2 else -1.0))      # along the edge
                R.add("c", o, towards(o, lo + rng.uniform(0.3, 0.7, 3) * ext))
                R.add("c", o, -towards(o, lo + rng.uniform(0.3, 0.7, 3) * ext))
    for corner in range(8):
        o = np.array([(lo, hi)[(corner >> i) & 1][i] for i in range(3)], np.float32)
        R.add("c", o, towards(o, lo + rng.uniform(0.3, 0.7, 3) * ext))
        R.add("c", o, -towards(o, lo + rng.uniform(0.3, 0.7, 3) * ext))
        R.add("c", o, _axis_dir(corner % 3, -1.0 if (corner >> (corner % 3)) & 1 else 1.0))      # along an edge, inwards
    # d. inside the bound: mint = 0, a mint that leaves the bound, a negative mint
    diag = float(np.sqrt((ext * ext).sum()))
    seeds_oblique = []
    for j in range(12):
        o = generic(-0.1)
        d = oblique() if j % 3 else _axis_dir(j % 3 if j < 6 else (j + 1) % 3, 1.0 if j < 6 else -1.0)
        seeds_oblique.append(R.add("d", o, d, 0.0))
        R.add("d", o, d, np.float32(1.5 * diag))
        R.add("d", o, d, np.float32(-0.5 * diag * rng.uniform(0.2, 1.0)))
    # e. on a voxel boundary of the grid
    for axis in range(3):
        nv = grid.grid_nvoxels[axis]
        for k in sorted({1 if nv > 1 else 0, nv // 2, nv - 1, nv}):
            vb = voxel_boundary(grid, axis, k)
            t_axis = (axis + 1 + k % 2) % 3
            for z in (0.0, NEG0):
                o = generic(); o[axis] = vb
                d = _axis_dir(t_axis, 1.0 if z == 0.0 else -1.0); d[axis] = z
                R.add("e", o, d)
            for sign in (1.0, -1.0):
                o = generic(); o[axis] = vb
                d = oblique(); d[axis] = np.float32(sign * abs(d[axis]))
                R.add("e", o, d)
                R.add("e", o, _axis_dir(axis, sign))
    # f. relative to a triangle
    e1, e2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    nrm = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    pick = rng.choice(len(tv), min(len(tv), 8), replace=False)
    for t in pick:                                                            # in the triangle's plane: d = a combination of its edges, o = a point of the plane
        o = (tv[t, 0].astype(np.float64) - 0.5 * e1[t] - 0.25 * e2[t]).astype(np.float32)
        R.add("f", o, (e1[t] + e2[t]).astype(np.float32))
        R.add("f", o, e1[t])
    edges, verts = {}, {}
    for t in range(len(tv)):
        for a in range(3):
            key = tuple(sorted((tuple(tv[t, a]), tuple(tv[t, (a + 1) % 3]))))
            edges.setdefault(key, []).append(t)
            verts.setdefault(tuple(tv[t, a]), []).append(t)
    shared = sorted(k for k, v in edges.items() if len(v) >= 2)
    for j in rng.choice(len(shared), min(len(shared), 8), replace=False):    # through the midpoint of a shared edge
        (a, b), t = shared[j], edges[shared[j]][0]
        mid = ((np.array(a, np.float64) + np.array(b, np.float64)) / 2)
        n = nrm[t] / np.abs(nrm[t]).max()
        axis = int(np.argmax(np.abs(nrm[t])))
        R.add("f", (mid - 3 * _axis_dir(axis, 1.0)).astype(np.float32), _axis_dir(axis, 1.0))
        o = (mid + 2.5 * n + np.array([0.75, -0.5, 0.25])).astype(np.float32)
        R.add("f", o, (mid - o.astype(np.float64)).astype(np.float32))         # not normalised: o + d * 1 is the edge's midpoint where that is exact
    most = sorted(verts.items(), key=lambda kv: (-len(kv[1]), kv[0]))[:6]
    if scene == "lattice":
        assert all(len(v) >= 6 for _, v in most), [len(v) for _, v in most]
    for p, ts in most:                                                        # through a vertex shared by many
        p = np.array(p, np.float64)
        axis = int(np.argmax(np.abs(nrm[ts[0]])))
        R.add("f", (p - 2 * _axis_dir(axis, 1.0)).astype(np.float32), _axis_dir(axis, 1.0, NEG0, 0.0))
        R.add("f", (p + 2 * _axis_dir(axis, 1.0)).astype(np.float32), _axis_dir(axis, -1.0))
        off = np.array([1.0, 2.0, -2.0])
        R.add("f", (p - off).astype(np.float32), off.astype(np.float32))       # o + d * 1 = the vertex exactly (small integers)
    for t in pick:                                                            # from a point on the triangle, mint = 0
        o = (tv[t, 0].astype(np.float64) + 0.25 * e1[t] + 0.25 * e2[t]).astype(np.float32)
        axis = int(np.argmax(np.abs(nrm[t])))
        R.add("f", o, _axis_dir(axis, 1.0), 0.0)
        R.add("f", o, oblique(), 0.0)
    # h. direction scaling: the unscaled ray (k = 0) and its four scaled twins; then denormal directions
    seeds_axis = []
    for j in range(4):
        o = generic(-0.1); axis = j % 3
        o[axis] = np.float32(lo[axis] - 0.07 * ext[axis])
        seeds_axis.append((o, _axis_dir(axis, 1.0, NEG0 if j & 1 else 0.0, 0.0)))
    for o, d in [(generic(-0.1), oblique()) for _ in range(6)] + seeds_axis:
        b = R.add("h", o, d, 0.0, MAXT, k=0)
        R.base[b] = b
        for k in H_SCALES:
            R.add("h", o, (d.astype(np.float64) * 2.0 ** k).astype(np.float32), 0.0, np.float32(float(MAXT) * 2.0 ** -k), base=b, k=k)
        dd = (d.astype(np.float64) * 2.0 ** H_DENORMAL).astype(np.float32)
        assert (np.abs(dd[dd != 0]) < np.finfo(np.float32).tiny).all() and (dd != 0).any()
        R.add("h", o, dd, 0.0, np.float32(np.inf), base=b, k=H_DENORMAL)
    # i. quadrics: poles, apex, centre; the phi = 0 seam; tangents
    if scene == "quadrics":
        for _, at in QUADRICS:
            c = np.array(at, np.float32)
            for sign in (1.0, -1.0):
                R.add("i", c - np.float32(5 * sign) * _axis_dir(2, 1.0), _axis_dir(2, sign, 0.0, NEG0 if sign < 0 else 0.0))     # along the object z axis
                for zy in (0.0, NEG0):                                                                                            # in the plane y = +-0, along x
                    for dz in (0.0, 0.25, -0.5):
                        o = c - np.float32(4 * sign) * _axis_dir(0, 1.0) + np.float32(0.5 if dz == 0 else 0.0) * _axis_dir(2, 1.0)
                        o[2] -= np.float32(4 * sign * dz) - np.float32(0.25 if dz else 0.0)
                        d = np.array([sign, zy, sign * dz], np.float32)
                        R.add("i", o, d)
        for (_, at), r in ((QUADRICS[0], 1.5), (QUADRICS[1], 1.0), (QUADRICS[6], 1.5)):                                          # tangent along y at x = centre +- r
            c = np.array(at, np.float32)
            for side in (1.0, -1.0):
                o = c + np.float32(side * r) * _axis_dir(0, 1.0) - np.float32(4) * _axis_dir(1, 1.0) + np.float32(0.5 if r == 1.0 else 0.0) * _axis_dir(2, 1.0)
                R.add("i", o, _axis_dir(1, 1.0))
                R.add("i", o + np.float32(8) * _axis_dir(1, 1.0), _axis_dir(1, -1.0, 0.0, NEG0))
    rays, cls, base, k = R.arrays()
    assert np.isfinite(rays[:, :7]).all() and (np.abs(rays[:, 0:3]) < 1024).all()
    return rays, cls, base, k, np.array(seeds_oblique, np.int64)


def second_pass(rays, cls, base, k, seeds_oblique, rec):
    """class g from the reference's records of the first pass: up to 6 hits among class (a) and up to 6 among the oblique rays of class (d)"""
    hit = rec[:, 8] > 0
    a_hits = [i for i in np.nonzero((cls == CODES.index("a")) & hit)[0]][:6]
    o_hits = [i for i in seeds_oblique if hit[i] and zero_components(rec[i:i + 1])[0] == 0][:6]
    assert len(a_hits) >= 3 and len(o_hits) >= 3, (len(a_hits), len(o_hits))
    rows = []
    inf = np.float32(np.inf)
    for i in a_hits + o_hits:
        t = np.float32(rec[i, 9])
        assert 0 < t < 1024
        for mint, maxt in ((0.0, t), (0.0, np.nextafter(t, np.float32(0))), (t, MAXT), (np.nextafter(t, inf), MAXT), (0.0, inf), (t, t),
                           (np.nextafter(t, inf), t)):
            r = rays[i].copy(); r[6], r[7] = mint, maxt
            rows.append(r)
    n = len(rows)
    g = CODES.index("g")
    return (np.concatenate([rays, np.array(rows, np.float32)]), np.concatenate([cls, np.full(n, g, np.uint8)]),
            np.concatenate([base, np.full(n, -1, np.int16)]), np.concatenate([k, np.zeros(n, np.int16)]))


def rays_of_records(pkg, rec):
    rays = np.zeros(len(rec), pkg.RAY_DTYPE)
    rays["o"], rays["d"], rays["mint"], rays["maxt"] = rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7]
    return rays


def nonfinite_reference_fields(rec):
    """hits whose reference record holds a non-finite p, nn, u or v (a pole, the apex)"""
    return (rec[:, 8] > 0) & ~np.isfinite(rec[:, 10:18]).all(1)


TIE_T, TIE_B = 1e-4, 1e-5


def equal_t_ties(tri_verts, rec):
    """hits at whose t the ray meets two or more triangles of the scene: through a shared edge or vertex, or from an edge of the box where two walls
    meet.  Which of them a closest-hit query reports is a matter of list order and of the reference's per-primitive mailbox (kdtree.cpp:376-386;
    this library re-tests): hit mask, t and p are those of either, (u, v) and the normal are not.  Float64 geometry only, from the
    fixture: |t_i - t| <= TIE_T * max(1, |t|) and barycentrics within TIE_B of [0, 1] -- wider than float32's error at coordinates below 2^10, so
    a superset of the exact ties."""
    tv = np.asarray(tri_verts, np.float64).reshape(-1, 3, 3)
    p1, e1, e2 = tv[:, 0], tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    real = np.abs(np.cross(e1, e2)).sum(1) > 0
    p1, e1, e2 = p1[real], e1[real], e2[real]
    out = (rec[:, 8] > 0) & ~np.isfinite(rec[:, 9])          # t = inf (a denormal d): every triangle whose barycentrics pass is met "at" it
    for i in np.nonzero((rec[:, 8] > 0) & np.isfinite(rec[:, 9]))[0]:
        o, d, t = rec[i, 0:3].astype(np.float64), rec[i, 3:6].astype(np.float64), float(rec[i, 9])
        s1 = np.cross(d, e2)
        div = (s1 * e1).sum(1)
        ok = div != 0
        with np.errstate(all="ignore"):
            inv = 1.0 / div
            dd = o - p1
            b1 = (dd * s1).sum(1) * inv
            s2 = np.cross(dd, e1)
            b2 = (s2 * d).sum(1) * inv
            ti = (s2 * e2).sum(1) * inv
            near = ok & (b1 >= -TIE_B) & (b2 >= -TIE_B) & (b1 + b2 <= 1 + TIE_B) & (np.abs(ti - t) <= TIE_T * max(1.0, abs(t)))
        out[i] = near.sum() >= 2
    return out


def class_table(rec, cls):
    """per class: (rays, hits, IntersectP hits)"""
    return {c: (int((cls == i).sum()), int(((cls == i) & (rec[:, 8] > 0)).sum()), int(((cls == i) & (rec[:, 18] > 0)).sum()))
            for i, c in enumerate(CODES) if (cls == i).any()}
