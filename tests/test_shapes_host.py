"""Shape "heightfield", "nurbs" and "loopsubdiv" refined into triangle meshes by the host front end (csrc/host/shape_refine.h): the descriptors against
the images the reference-side adapter dumped of the reference's OWN refined geometry (tests/golden/desc_shapes/, byte for byte), the CPU oracle's film
of the parsed scene against the reference's film (tests/golden/shapes/), the triangle and kd-tree node counts against StatsPrint, closed forms in
float64 written here, and the statements that are refused.  CPU only; tests/test_gpu_shapes.py renders the same fixtures on the device."""
import glob
import importlib.util
import json
import lzma
import os

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import GOLDEN, film_metrics, load_golden, stat_int
from test_boundary import differing_sections

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILMS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "shapes", "*.npz")))
DESCS = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(GOLDEN, "desc_shapes", "*.xz")))
EXPECTED = ("hf_debug", "hf_direct_emitter", "loop_default_whitted", "loop_emitter_direct", "loop_level0_whitted", "loop_octa_whitted", "loop_open_debug",
            "loop_tetra_debug", "loop_umbrella_path", "nurbs_p_debug", "nurbs_pw_whitted")
TWIN_KEPT = ("hf_debug", "loop_tetra_debug", "nurbs_p_debug")
ULP = 2.0 ** -24                                         # half a unit in the last place of a float32 in [1, 2): the relative error of one rounding
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\n'


def generator():
    """tests/golden/make_shapes_golden.py, for desc_scene(): the one place that says which scene a descriptor image is of"""
    spec = importlib.util.spec_from_file_location("make_shapes_golden", os.path.join(GOLDEN, "make_shapes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parse_world(pkg, scenes, body, quiet=True):
    return pkg.ParsedScene(text=scenes.options_block(xres=16, yres=16) + 'WorldBegin\nLightSource "point"\n' + body + "WorldEnd\n", quiet=quiet)


def mesh_of(pkg, ps):
    """(verts [n, 3, 3], records) of a scene with ONE shape, in the order the mesh lists its triangles (the descriptors hold a mesh last triangle first)"""
    idx, rec, _ = pkg.shading_records(ps)
    verts = ps.tri_verts()[::-1]
    return verts, (rec[idx[::-1]] if idx is not None else None)


# ---------------------------------------------------------------- 1. descriptors
@pytest.mark.parametrize("name", [n for n in EXPECTED if n != "loop_level0_whitted"])          # the generator says why that one has no image
def test_descriptors_are_the_reference_adapters(pkg, name):
    """Committed images of what oracle/ref/hip_adapter.cpp flattened from the reference's refined shapes: vertices, normals, uvs, triangle order,
    emitter triangles.  This says whether the TESSELLATION is the reference's, whatever a kernel does with it."""
    ps = pkg.ParsedScene(text=generator().desc_scene(load_golden("shapes/" + name)["scene"]))
    assert ps.valid and ps.errors == 0, name
    mine = ps.serialize()
    ref = lzma.decompress(open(os.path.join(GOLDEN, "desc_shapes", name + ".xz"), "rb").read())
    assert mine == ref, (name, differing_sections(mine, ref))


def test_descriptors_live_when_the_reference_is_built(pkg):
    rr = g_entry.load_ref_runner()
    if not os.path.exists(os.path.join(rr.REF_DIR, "bin", "hip.so")):
        pytest.skip("oracle/_ref/bin/hip.so not on this box")
    gen = generator()
    for name in DESCS:
        text = gen.desc_scene(load_golden("shapes/" + name)["scene"])
        ref = rr.reference_descriptors(text)
        mine = pkg.ParsedScene(text=text).serialize()
        assert mine == ref, (name, differing_sections(mine, ref))


# ---------------------------------------------------------------- 2. the oracle's film of the parsed scene
@pytest.mark.parametrize("name", [n for n in EXPECTED if n.endswith(("_whitted", "_direct", "_emitter"))])
def test_oracle_film_matches_the_reference(pkg, oracle, name):
    """The strict bar of tests/gpu_checks.py (rgb and alpha within 1e-5, ray counts equal) for the CPU restatement on the host's refined mesh."""
    g = load_golden("shapes/" + name)
    ps = pkg.ParsedScene(text=g["scene"])
    assert ps.valid and ps.errors == 0
    nodes, refs, bounds, info = ps.kdtree()
    rgb, alpha, _, cnt = oracle.render(ps, nodes, refs, bounds, info=info)
    m = film_metrics(rgb, g["rgb"])
    print(name, m, float(np.abs(alpha - g["alpha"]).max()))
    assert m["maxabs"] <= 1e-5 and np.abs(alpha - g["alpha"]).max() <= 1e-5, (name, m)
    assert (cnt["closest_rays"], cnt["any_rays"], cnt["bad_samples"]) == (g["stats"]["closest_rays"], g["stats"]["any_rays"], 0)


# ---------------------------------------------------------------- 3. StatsPrint
@pytest.mark.parametrize("name", EXPECTED)
def test_triangle_and_node_counts_match_statsprint(pkg, name):
    """"Triangles created" counts every Triangle object: an emitter's shape is refined once for the primitive and once more for the AreaLight's
    ShapeSet (area.cpp:33-54), so the reference's figure is n_tris + n_light_tris -- n_tris itself where nothing emits."""
    g = load_golden("shapes/" + name)
    ps = pkg.ParsedScene(text=g["scene"])
    table = g["stats"]["stats"]
    assert ps.errors == 0 and ps.n_tris + ps.n_light_tris == int(table["Triangles created"]), (name, ps.n_tris, ps.n_light_tris, table["Triangles created"])
    assert (ps.n_light_tris > 0) == ("emitter" in name)
    nodes, _, _, _ = ps.kdtree()
    leaf = (nodes[:, 0] & 3) == 3
    for key, mine in (("Interior kd-tree nodes made", int((~leaf).sum())), ("Leaf kd-tree nodes made", int(leaf.sum()))):
        ref, exact = stat_int(table[key])
        assert exact and mine == ref, (name, key, mine, table[key])


# ---------------------------------------------------------------- 4. closed forms in float64
def test_heightfield_vertices_and_uvs(pkg, scenes):
    """Vertex x + y * nu is (x / (nu - 1), y / (nv - 1), Pz) with uv = its (x, y): one float division per coordinate, so each is within one
    rounding (2^-24 relative, and the values are at most 1) of the float64 quotient; Pz, given as float32, is kept exactly, and the identity
    CTM multiplies by 1 and adds 0.  Two triangles per cell: (v00, v10, v11), (v00, v11, v01)."""
    nu, nv = 5, 3
    z = (np.arange(nu * nv, dtype=np.float32) * np.float32(.37) - np.float32(2)).astype(np.float32)
    ps = parse_world(pkg, scenes, scenes.heightfield_text(nu, nv, z))
    assert ps.errors == 0 and ps.warnings == 0 and ps.n_tris == 2 * (nu - 1) * (nv - 1)
    verts, rec = mesh_of(pkg, ps)
    P = np.array([[x / (nu - 1), y / (nv - 1), float(z[x + y * nu])] for y in range(nv) for x in range(nu)])
    want = []
    for y in range(nv - 1):
        for x in range(nu - 1):
            a = x + y * nu
            want += [[a, a + 1, a + 1 + nu], [a, a + 1 + nu, a + nu]]
    want = np.array(want)
    assert np.abs(verts[..., :2] - P[want][..., :2]).max() <= ULP
    assert np.array_equal(verts[..., 2], P[want][..., 2].astype(np.float32))
    assert (rec["flags"] == 1).all()                                                    # RT_SHADING_UV alone: no N, no S
    assert np.abs(rec["uv"].reshape(-1, 3, 2) - P[want][..., :2]).max() <= ULP


def test_quarter_cylinder_patch_is_on_the_cylinder(pkg, scenes):
    """The rational quadratic arc with weights (1, sqrt(1/2), 1), extruded along z: every diced vertex has x^2 + y^2 = 1 and a radial normal.
    Rounding budget per homogeneous coordinate: a de Boor level is 6 roundings on values of at most 1 (alpha: a subtraction and a division,
    1 - alpha, two products, one sum), there are three levels (one in v, two in u) for the numerator and three for w: 36 roundings; the dicing
    parameter (Lerp: 3 roundings) moves the point by at most twice its error: 6; sqrt(1/2) enters as a float32: 1; the division by
    w >= sqrt(1/2) adds 1 and scales the rest by sqrt(2): (36 + 6 + 1) * sqrt(2) + 1 < 64 roundings of 2^-24.
    The normal: dPdu has components of at most 3 (factor 2 over w >= .7) from about 40 such roundings, against a speed of at least 1.4, and
    the cross product and Normalize add 6: under 128 roundings of 2^-24 in the sine of the angle to the radius."""
    s2 = np.float32(np.sqrt(.5))
    pw = [1, 0, 0, 1, s2, s2, 0, s2, 0, 1, 0, 1, 1, 0, 1, 1, s2, s2, s2, s2, 0, 1, 1, 1]
    ps = parse_world(pkg, scenes, scenes.nurbs_text(3, 3, [0, 0, 0, 1, 1, 1], 2, 2, [0, 0, 1, 1], Pw=pw))
    assert ps.errors == 0 and ps.warnings == 0 and ps.n_tris == 2 * 29 * 29
    verts, rec = mesh_of(pkg, ps)
    v = verts.reshape(-1, 3).astype(np.float64)
    r = np.hypot(v[:, 0], v[:, 1])
    print("radius error", float(np.abs(r - 1).max()))
    assert np.abs(r - 1).max() <= 64 * ULP
    assert v[:, 2].min() == 0.0 and v[:, 2].max() == 1.0 and (v[:, :2] >= -64 * ULP).all()
    assert (rec["flags"] == 3).all()                                                    # uv and N
    n = rec["n"].reshape(-1, 3).astype(np.float64)
    radial = np.stack([v[:, 0] / r, v[:, 1] / r, np.zeros_like(r)], 1)
    sine = np.linalg.norm(np.cross(n, radial), axis=1)
    print("normal: sine of the angle to the radius", float(sine.max()), "length error", float(np.abs(np.linalg.norm(n, axis=1) - 1).max()))
    assert sine.max() <= 128 * ULP and np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 4 * ULP
    assert len(set(np.sign((n * radial).sum(1)))) == 1                                  # all to the same side
    uv = rec["uv"].reshape(-1, 2).astype(np.float64)
    # v is the height; u runs along the arc: the angle is a monotone function of u from 0 to pi / 2
    assert np.abs(uv[:, 1] - v[:, 2]).max() <= 8 * ULP
    order = np.argsort(uv[:, 0], kind="stable")
    assert (np.diff(np.arctan2(v[order, 1], v[order, 0])) >= -128 * ULP).all()


def planar_grid(scenes, n=4):
    P, F = scenes.grid_mesh(n, n, 3.0)
    e1, e2, o = np.array([.8, .6, 0.0]), np.array([-.36, .48, .8]), np.array([.25, -.5, 1.0])      # an orthonormal pair: a tilted plane
    return (o + P[:, :1] * e1 + P[:, 1:2] * e2).astype(np.float32), F, np.cross(e1, e2), o


def test_planar_grid_stays_planar(pkg, scenes):
    """A regular grid in a tilted plane, two levels and the limit rule.  Every rule is an affine combination with weights that sum to 1, so
    the plane is kept up to rounding: a stage is at most 13 roundings per coordinate (valence 6: 7 products, 6 sums), three stages: 39,
    one more for the float32 control points, times sqrt(3) for the three coordinates in the distance: 70 roundings of 2^-24 * M, M = 4 the
    largest coordinate.  The tangents S, T sum up to 6 ring points with weights of at most 2, so they leave the plane by at most 6 * 2 such
    distances, against a length of about 3/4 of the original spacing 1 over four (two levels): the sine of the angle between a limit normal and
    the plane's is below 12 * 70 * 2^-24 * 4 / (3 / 16)."""
    P, F, normal, o = planar_grid(scenes)
    M = 4.0
    assert np.abs(P).max() <= M
    ps = parse_world(pkg, scenes, scenes.loopsubdiv_text(P, F, 2))
    assert ps.errors == 0 and ps.warnings == 0 and ps.n_tris == 16 * len(F)
    verts, rec = mesh_of(pkg, ps)
    dist = np.abs((verts.reshape(-1, 3).astype(np.float64) - o) @ normal)
    print("distance from the plane", float(dist.max()))
    assert dist.max() <= 70 * ULP * M
    assert (rec["flags"] == 2).all()                                                    # N alone: GetUVs' defaults
    assert np.array_equal(rec["uv"], np.tile(np.float32([0, 0, 1, 0, 1, 1]), (len(rec), 1)))
    n = rec["n"].reshape(-1, 3).astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    assert length.min() > 0
    sine = np.linalg.norm(np.cross(n, normal), axis=1) / length
    print("normals: sine of the angle to the plane's", float(sine.max()))
    assert sine.max() <= 12 * 70 * ULP * M / (3.0 / 16.0)
    assert len(set(np.sign(n @ normal))) == 1


def test_translating_the_control_mesh_translates_the_surface(pkg, scenes):
    """Octahedron of radius 1, moved by t = (8, -4, 16): its control points are exact in float32 both times.  The weights of every rule sum
    to 1 only up to rounding, and each of the 39 roundings of the three stages (see above) is now relative to |t| + 1 = 17."""
    P, F = scenes.octahedron(1.0)
    t = np.array([8.0, -4.0, 16.0])
    a, _ = mesh_of(pkg, parse_world(pkg, scenes, scenes.loopsubdiv_text(P, F, 2)))
    b, _ = mesh_of(pkg, parse_world(pkg, scenes, scenes.loopsubdiv_text(P + t, F, 2)))
    assert a.shape == b.shape == (8 * 16, 3, 3)
    err = np.abs(b.astype(np.float64) - t - a).max()
    print("translation error", float(err))
    assert err <= 40 * ULP * 17
    assert 0.2 < np.linalg.norm(a.reshape(-1, 3), axis=1).min() and np.linalg.norm(a.reshape(-1, 3), axis=1).max() < 1.0     # inside the control mesh


def test_default_levels_and_level_zero(pkg, scenes):
    P, F = scenes.octahedron(1.0)
    assert parse_world(pkg, scenes, scenes.loopsubdiv_text(P, F)).n_tris == 8 * 64      # nlevels defaults to 3
    for n in (0, -2):                                                                   # the limit surface of the control mesh itself
        ps = parse_world(pkg, scenes, scenes.loopsubdiv_text(P, F, n))
        verts, rec = mesh_of(pkg, ps)
        assert ps.errors == 0 and ps.n_tris == 8
        # valence 4: gamma = 1 / (4 + 3 / (8 * 3 / 32)) = 1 / 8, and the ring of an octahedron's vertex sums to zero: the limit is P / 2
        assert np.abs(np.abs(verts).sum(-1) - .5).max() <= 8 * ULP and (rec["flags"] == 2).all()


# ---------------------------------------------------------------- 5. refusals and parameters
OCTA_I = "0 1 2 0 2 3 0 3 4 0 4 1 5 2 1 5 3 2 5 4 3 5 1 4"
OCTA_P = "0 0 1 1 0 0 0 1 0 -1 0 0 0 -1 0 0 0 -1"
KN = '"integer nu" [3] "integer uorder" [3] "float uknots" [0 0 0 1 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1]'
P6 = '"point P" [0 0 0 1 0 1 2 0 0 0 1 0 1 1 1 2 1 0]'
REFUSED = {
    "hf_nu_only": 'Shape "heightfield" "integer nu" [2]',
    "hf_no_pz": 'Shape "heightfield" "integer nu" [2] "integer nv" [2]',
    "hf_count": 'Shape "heightfield" "integer nu" [2] "integer nv" [3] "float Pz" [0 1 2 3 4]',
    "hf_too_small": 'Shape "heightfield" "integer nu" [1] "integer nv" [3] "float Pz" [0 1 2]',
    "nurbs_no_knots": 'Shape "nurbs" "integer nu" [3] "integer uorder" [3] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] ' + P6,
    "nurbs_knot_count": 'Shape "nurbs" "integer nu" [3] "integer uorder" [3] "float uknots" [0 0 0 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] ' + P6,
    "nurbs_point_count": 'Shape "nurbs" ' + KN + ' "point P" [0 0 0 1 0 1 2 0 0 0 1 0 1 1 1]',
    "nurbs_pw_count": 'Shape "nurbs" ' + KN + ' "float Pw" [0 0 0 1 1 0 1 1 2 0 0 1 0 1 0 1 1 1 1 1]',
    "nurbs_no_order": 'Shape "nurbs" "integer nu" [3] "float uknots" [0 0 0 1 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] ' + P6,
    "nurbs_u1_outside": 'Shape "nurbs" ' + KN + ' "float u1" [1.5] ' + P6,
    "loop_index_range": 'Shape "loopsubdiv" "integer indices" [0 1 6 0 2 3] "point P" [%s]' % OCTA_P,
    "loop_three_faces_on_an_edge": 'Shape "loopsubdiv" "integer indices" [0 1 2 1 0 3 0 1 4] "point P" [0 0 0 1 0 0 0 1 0 0 -1 0 0 0 1]',
    "loop_same_winding": 'Shape "loopsubdiv" "integer indices" [0 1 2 0 1 3] "point P" [0 0 0 1 0 0 0 1 0 0 -1 0]',
    "loop_too_many_levels": 'Shape "loopsubdiv" "integer nlevels" [14] "integer indices" [%s] "point P" [%s]' % (OCTA_I, OCTA_P),      # 8 * 4^14 = 2^31
    "loop_unused_vertex": 'Shape "loopsubdiv" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0 5 5 5]',
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_malformed_statements_are_errors_and_leave_the_scene(pkg, scenes, name):
    ps = parse_world(pkg, scenes, TRI + REFUSED[name] + "\n" + TRI)
    assert ps.errors == 1 and ps.valid and ps.n_tris == 2 and ps.n_materials == 2, (name, ps.errors, ps.n_tris)


def test_patch_without_control_points_gives_no_shape(pkg, scenes):
    ps = parse_world(pkg, scenes, TRI + 'Shape "nurbs" ' + KN + "\n")                   # nurbs.cpp:321-324: return NULL, no message
    assert ps.errors == 0 and ps.valid and ps.n_tris == 1
    ps = parse_world(pkg, scenes, TRI + 'Shape "loopsubdiv" "integer indices" [0 1 2]\n')      # loopsubdiv.cpp:487
    assert ps.errors == 0 and ps.valid and ps.n_tris == 1


def test_misspelt_parameter_is_one_warning(pkg, scenes):
    ps = parse_world(pkg, scenes, 'Shape "loopsubdiv" "integer nlevel" [1] "integer indices" [%s] "point P" [%s]\n' % (OCTA_I, OCTA_P))
    assert ps.errors == 0 and ps.warnings == 1 and ps.n_tris == 8 * 64                  # ... and nlevels stays 3
    ps = parse_world(pkg, scenes, 'Shape "loopsubdiv" "integer nlevels" [1] "string scheme" ["loop"] "integer indices" [%s] "point P" [%s]\n' % (OCTA_I, OCTA_P))
    assert ps.errors == 0 and ps.warnings == 0 and ps.n_tris == 32


@pytest.mark.parametrize("shape", ['Shape "heightfield" "integer nu" [2] "integer nv" [2] "float Pz" [0 0 0 1]',
                                   'Shape "nurbs" ' + KN + " " + P6,
                                   'Shape "loopsubdiv" "integer nlevels" [1] "integer indices" [%s] "point P" [%s]' % (OCTA_I, OCTA_P)])
def test_shape_statement_material_parameters_win(pkg, scenes, shape):
    """api.cpp:361-375: TextureParams looks in the shape's parameters first -- and the shape, which did not read them, reports them unused."""
    ps = parse_world(pkg, scenes, 'Material "matte" "color Kd" [.9 .1 .1]\n' + shape + ' "color Kd" [.2 .6 .8]\n' + shape + "\n")
    assert ps.errors == 0 and ps.warnings == 1 and ps.n_materials == 2
    mats = ps.materials()
    assert np.array_equal(mats[0]["Kd"], np.float32([.2, .6, .8])) and np.array_equal(mats[1]["Kd"], np.float32([.9, .1, .1]))


def test_object_instancing_still_refuses_the_shape(pkg, scenes):
    ps = parse_world(pkg, scenes, TRI + 'ObjectBegin "o"\nShape "heightfield" "integer nu" [2] "integer nv" [2] "float Pz" [0 0 0 1]\nObjectEnd\n')
    assert ps.errors == 1 and ps.n_tris == 1


# ---------------------------------------------------------------- 6. fixtures
def test_fixtures_present():
    assert tuple(FILMS) == EXPECTED and len(FILMS) >= 10
    assert DESCS == sorted(n for n in EXPECTED if n != "loop_level0_whitted") and len(DESCS) >= 10
    for name in FILMS:
        p = os.path.join(GOLDEN, "shapes", name + ".npz")
        z = np.load(p)
        assert os.path.getsize(p) < 64 * 1024, p
        assert float(z["twin_share"]) >= 0.05, (p, float(z["twin_share"]))
        assert z["rgb"].shape == (24, 24, 3) and np.isfinite(z["rgb"]).all() and np.isfinite(z["alpha"]).all(), p
        assert json.loads(str(z["stats"]))["stderr_lines"] == (1 if name == "loop_emitter_direct" else 0), p     # area.cpp:50-52: more than 16 triangles emit
        if name in TWIN_KEPT:
            assert z["twin_rgb"].shape == z["rgb"].shape and np.isfinite(z["twin_rgb"]).all(), p
    for name in DESCS:
        assert os.path.getsize(os.path.join(GOLDEN, "desc_shapes", name + ".xz")) < 64 * 1024, name
