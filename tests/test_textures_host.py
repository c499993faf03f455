"""Host front end of the textures whose value depends on the hit alone (textures/{scale,mix,bilerp,uv,checkerboard}.cpp with the four 2-D
mappings of core/texture.cpp:63-149): the parsed table, the classes and modes that stay errors, the host evaluation (the definition the device
runs, include/pbrt_hip_texture.h) against float32 values worked out in numpy in the reference's order of operations, the per-hit material
resolve, and the descriptor images that must not move.  CPU only."""
import ctypes as C
import glob
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0] %s\n'
f32 = np.float32
NONE = '"string aamode" ["none"]'


def parse(pkg, scenes, world):
    hdr = scenes.options_block(xres=16, yres=16, integrator="whitted")
    return pkg.ParsedScene(text=hdr + 'WorldBegin\nLightSource "point" "point from" [278 500 200] "color I" [100000 100000 100000]\n' + world + "WorldEnd\n")


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def floor2int(x):
    return int(np.floor(np.float64(x)))


# ---- the parsed table ---------------------------------------------------------------------------------------------------------------------
def test_checkerboard_table_defaults_and_uv_mapping(pkg, scenes):
    ps = parse(pkg, scenes, 'Texture "c" "color" "checkerboard" %s\nMaterial "matte" "texture Kd" "c"\n' % NONE + TRI % "")
    assert ps.errors == 0 and ps.warnings == 0 and ps.has_textures()
    t = ps.textures()
    assert [x["class"] for x in t] == ["constant", "constant", "checkerboard"] and [x["name"] for x in t] == ["", "", "c"]
    assert same_bits(t[0]["value"], [1, 1, 1]) and same_bits(t[1]["value"], [0, 0, 0])                 # tex1 = 1, tex2 = 0 (checkerboard.cpp:225-226)
    c = t[2]
    assert c["type"] == "color" and (c["tex1"], c["tex2"]) == (0, 1) and c["mapping"] == "uv"
    assert (c["uscale"], c["vscale"], c["udelta"], c["vdelta"]) == (1.0, 1.0, 0.0, 0.0)
    m = ps.materials()[0]
    assert m["textured"] == {"Kd": 2} and same_bits(m["Kd"], [1, 1, 1]) and m["sigma"] == 0.0         # the literal / default stays in the descriptor


def test_mapping_parameters_and_float_classes(pkg, scenes):
    world = ('Translate 1 2 3\n'
             'Texture "b" "float" "bilerp" "string mapping" ["planar"] "vector v1" [0 0 2] "vector v2" [0 3 0] "float udelta" [.5] "float vdelta" [.25] "float v10" [4]\n'
             'Texture "s" "color" "uv" "string mapping" ["spherical"]\n'
             'Texture "y" "color" "checkerboard" "string mapping" ["cylindrical"] %s "color tex1" [.1 .2 .3]\n'
             'Texture "sc" "float" "scale" "texture tex1" "b" "float tex2" [3]\n'
             'Texture "mx" "float" "mix" "texture tex1" "sc" "texture amount" "b"\n'
             'Material "plastic" "texture roughness" "mx" "texture Kd" "s" "texture Ks" "y"\n' % NONE) + TRI % ""
    ps = parse(pkg, scenes, world)
    assert ps.errors == 0 and ps.warnings == 0
    t = {x["name"]: x for x in ps.textures() if x["name"]}
    b = t["b"]
    assert b["type"] == "float" and b["mapping"] == "planar" and same_bits(b["v1"], [0, 0, 2]) and same_bits(b["v2"], [0, 3, 0])
    assert (b["udelta"], b["vdelta"]) == (0.5, 0.25) and (b["v00"], b["v01"], b["v10"], b["v11"]) == (0.0, 1.0, 4.0, 1.0)     # bilerp.cpp:82-84 defaults
    w2t = np.eye(4, dtype=f32); w2t[:3, 3] = [-1, -2, -3]                                              # the inverse of the CTM at the statement
    assert np.array_equal(t["s"]["world_to_texture"], w2t) and t["s"]["mapping"] == "spherical"
    assert t["y"]["mapping"] == "cylindrical" and np.array_equal(t["y"]["world_to_texture"], w2t)
    tab = ps.textures()
    assert tab[t["sc"]["tex1"]]["name"] == "b" and tab[t["sc"]["tex2"]]["value"] == 3.0
    assert tab[t["mx"]["tex1"]]["name"] == "sc" and tab[t["mx"]["tex2"]]["value"] == 1.0 and tab[t["mx"]["amount"]]["name"] == "b"   # mix.cpp: tex2 defaults to 1
    m = ps.materials()[0]
    assert set(m["textured"]) == {"roughness", "Kd", "Ks"} and tab[m["textured"]["roughness"]]["name"] == "mx"
    for i, x in enumerate(tab):                                                                      # children before parents
        assert all(x[k] < i for k in ("tex1", "tex2", "amount") if k in x)


def test_shape_parameters_come_before_material_parameters(pkg, scenes):
    pre = 'Texture "a" "color" "checkerboard" %s\nTexture "b" "color" "uv"\n' % NONE
    ps = parse(pkg, scenes, pre + 'Material "matte" "texture Kd" "a"\n' + TRI % '"texture Kd" "b"' + TRI % '"color Kd" [.2 .3 .4]' + TRI % "")
    assert ps.errors == 0
    tab, mats = ps.textures(), ps.materials()
    assert tab[mats[0]["textured"]["Kd"]]["name"] == "b"                                               # the shape's texture wins
    assert tab[mats[1]["textured"]["Kd"]]["name"] == "a"        # TextureParams looks for a TEXTURE of that name first, in both sets (paramset.cpp:438-439)
    assert tab[mats[2]["textured"]["Kd"]]["name"] == "a"


def test_attribute_scoping_and_unused_parameters(pkg, scenes):
    world = ('AttributeBegin\nTexture "in" "color" "checkerboard" %s "float nosuch" [1]\nMaterial "matte" "texture Kd" "in"\n' % NONE + TRI % "" + 'AttributeEnd\n'
             'Material "matte" "texture Kd" "in"\n' + TRI % "")
    ps = parse(pkg, scenes, world)
    assert ps.warnings == 1                                                                            # ReportUnused: "nosuch"
    assert ps.errors == 1                                                                              # outside the scope the name is gone: "couldn't find"
    mats = ps.materials()
    assert mats[0]["textured"] == {"Kd": 2} and mats[1]["textured"] == {} and same_bits(mats[1]["Kd"], [1, 1, 1])


REFUSED = ['"checkerboard"',                                              # closedform is the reference's default
           '"checkerboard" "string aamode" ["closedform"]', '"checkerboard" "string aamode" ["supersample"]',
           '"checkerboard" "integer dimension" [3] %s' % NONE, '"imagemap" "string filename" ["x.exr"]',
           '"fbm"', '"wrinkled"', '"marble"', '"windy"', '"dots"']


@pytest.mark.parametrize("decl", REFUSED)
def test_refused_classes_give_one_error_and_leave_the_name_undefined(pkg, scenes, decl):
    ps = parse(pkg, scenes, 'Texture "t" "color" %s\n' % decl + TRI % "")
    assert ps.errors == 1 and ps.valid and all(x["name"] != "t" for x in ps.textures())
    # a material that names it behaves as the reference does for an unknown name: one more error, then the literal or the default
    ps2 = parse(pkg, scenes, 'Texture "t" "color" %s\nMaterial "matte" "texture Kd" "t" "color Kd" [.2 .3 .4]\n' % decl + TRI % "")
    assert ps2.errors == 2 and not ps2.has_textures()
    m = ps2.materials()[0]
    assert same_bits(m["Kd"], [.2, .3, .4]) and "textured" not in m


def test_default_aamode_message_names_closedform(pkg, scenes, capfd):
    hdr = scenes.options_block(xres=16, yres=16, integrator="whitted")
    ps = pkg.ParsedScene(text=hdr + 'WorldBegin\nTexture "t" "color" "checkerboard"\n' + TRI % "" + "WorldEnd\n", quiet=False)
    err = capfd.readouterr().err
    assert ps.errors == 1 and "closedform" in err and "none" in err


def test_bumpmap_with_a_non_constant_texture_is_an_error(pkg, scenes):
    ps = parse(pkg, scenes, 'Texture "b" "float" "checkerboard" %s\nMaterial "matte" "texture bumpmap" "b"\n' % NONE + TRI % "")
    assert ps.errors == 1 and not ps.has_textures()


# ---- host evaluation ----------------------------------------------------------------------------------------------------------------------
def test_checkerboard_values_with_negative_coordinates_and_edges(pkg, scenes):
    ps = parse(pkg, scenes, 'Texture "c" "color" "checkerboard" %s "color tex1" [.1 .2 .3] "color tex2" [.7 .8 .9] "float uscale" [4] "float vscale" [2] '
                            '"float udelta" [-1.5] "float vdelta" [.25]\n' % NONE + TRI % "")
    a, b = [.1, .2, .3], [.7, .8, .9]
    for u, v in ((.1, .1), (.9, .1), (.3, .6), (0.374999, .2), (0.375001, .2), (.5, .374999), (.5, .375001), (-.3, -.8), (0., 0.)):
        s = f32(4) * f32(u) + f32(-1.5); t = f32(2) * f32(v) + f32(.25)                                # UVMapping2D::Map texture.cpp:71-72
        want = a if (floor2int(s) + floor2int(t)) % 2 == 0 else b                                      # Floor2Int rounds towards minus infinity
        assert same_bits(ps.eval_texture("c", (0, 0, 0), u, v), want), (u, v, float(s), float(t))
    # hand-computed: u = .1 -> s = -1.1 (floor -2), v = .1 -> t = .45 (floor 0): even -> tex1;  u = .3 -> s = -.3 (floor -1): odd -> tex2
    assert same_bits(ps.eval_texture("c", (0, 0, 0), .1, .1), a) and same_bits(ps.eval_texture("c", (0, 0, 0), .3, .1), b)


def test_bilerp_uv_scale_mix_values(pkg, scenes):
    world = ('Texture "bl" "color" "bilerp" "color v00" [.9 .2 .1] "color v01" [.1 .7 .2] "color v10" [.2 .2 .9] "color v11" [.8 .8 .1] "float uscale" [2] "float vdelta" [.1]\n'
             'Texture "uvt" "color" "uv" "float uscale" [3] "float vscale" [-2]\n'
             'Texture "fb" "float" "bilerp" "float v00" [.1] "float v01" [.9] "float v10" [.7] "float v11" [.3]\n'
             'Texture "sc" "color" "scale" "texture tex1" "bl" "color tex2" [.5 .6 .9]\n'
             'Texture "mx" "color" "mix" "texture tex1" "uvt" "texture tex2" "sc" "texture amount" "fb"\n') + TRI % ""
    ps = parse(pkg, scenes, world)
    assert ps.errors == 0

    def bilerp(s, t, v00, v01, v10, v11):                                                             # bilerp.cpp: four terms, left to right, float32
        v00, v01, v10, v11 = (np.asarray(x, f32) for x in (v00, v01, v10, v11))
        one = f32(1)
        return ((((one - s) * (one - t)) * v00 + ((one - s) * t) * v01) + (s * (one - t)) * v10) + (s * t) * v11
    for u, v in ((.25, .5), (.8, .3), (-.4, 1.7)):
        u, v = f32(u), f32(v)
        s, t = f32(2) * u + f32(0), f32(1) * v + f32(.1)
        bl = bilerp(s, t, [.9, .2, .1], [.1, .7, .2], [.2, .2, .9], [.8, .8, .1])
        assert same_bits(ps.eval_texture("bl", (0, 0, 0), u, v), bl)
        s2, t2 = f32(3) * u + f32(0), f32(-2) * v + f32(0)
        uvt = np.array([s2 - f32(floor2int(s2)), t2 - f32(floor2int(t2)), 0], f32)                    # uv.cpp
        assert same_bits(ps.eval_texture("uvt", (0, 0, 0), u, v), uvt)
        fb = bilerp(u, v, .1, .9, .7, .3)
        assert f32(ps.eval_texture("fb", (0, 0, 0), u, v)) == fb
        sc = bl * np.array([.5, .6, .9], f32)                                                         # scale.cpp
        assert same_bits(ps.eval_texture("sc", (0, 0, 0), u, v), sc)
        mx = (f32(1) - fb) * uvt + fb * sc                                                            # mix.cpp, a graph of depth 3
        assert same_bits(ps.eval_texture("mx", (0, 0, 0), u, v), mx)


def test_planar_spherical_cylindrical_mappings(pkg, scenes):
    world = ('Texture "pl" "color" "uv" "string mapping" ["planar"] "vector v1" [.5 0 .25] "vector v2" [0 -.5 0] "float udelta" [.1] "float vdelta" [.2]\n'
             'Translate 1 2 3\n'
             'Texture "sp" "color" "uv" "string mapping" ["spherical"]\nTexture "cy" "color" "uv" "string mapping" ["cylindrical"]\n') + TRI % ""
    ps = parse(pkg, scenes, world)
    p = np.array([1.5, -2.25, 4], f32)
    s = f32(.1) + ((p[0] * f32(.5) + p[1] * f32(0)) + p[2] * f32(.25)); t = f32(.2) + ((p[0] * f32(0) + p[1] * f32(-.5)) + p[2] * f32(0))
    assert same_bits(ps.eval_texture("pl", p, 0, 0), [s - f32(floor2int(s)), t - f32(floor2int(t)), 0])
    q = (p - np.array([1, 2, 3], f32)).astype(np.float64); q /= np.linalg.norm(q)
    got = ps.eval_texture("sp", p, 0, 0)                                                               # libm (acosf, atan2f): a few ulp
    phi = np.arctan2(q[1], q[0]); phi = phi + 2 * np.pi if phi < 0 else phi
    assert abs(got[0] - np.arccos(q[2]) / np.pi) < 1e-6 and abs(got[1] - phi / (2 * np.pi)) < 1e-6
    got = ps.eval_texture("cy", p, 0, 0)
    tz = q[2] - np.floor(q[2])
    assert abs(got[0] - (np.pi + np.arctan2(q[1], q[0])) / (2 * np.pi)) < 1e-6 and abs(got[1] - tz) < 1e-6


def test_per_hit_resolve_is_the_host_resolve(pkg, scenes):
    """rt_material_from_params + rt_material_resolve (what the device runs per hit) give what the untextured path derives: uber's products and lobes,
    the clamps, Oren-Nayar's A and B, the Blinn exponent and its cap."""
    H = pkg.host_lib()
    P = pkg.RtMaterialParams(); P.type = 4                                                             # uber: Kd, Ks, Kr, opacity, roughness
    for k, col in enumerate(([.6, -1, .3], [.3, .3, .3], [0, 0, 0], [1, 1, 1])):
        for c in range(3):
            P.c[k][c] = col[c]
    P.f = 0.0005
    m, r = pkg.RtMaterial(), pkg.RtMaterialResolved()
    H.pbrt_host_material_resolve(C.byref(P), C.byref(m), C.byref(r))
    assert same_bits(list(m.kd), [.6, 0, .3]) and same_bits(list(m.kt), [0, 0, 0]) and list(m.kr) == [0, 0, 0]
    assert (r.has_t, r.has_r, r.has_g, r.has_kr) == (0, 1, 1, 0) and r.exponent == 1000.0            # opacity 1: no transmission lobe; 1 / .0005 capped
    P.type = 0; P.f = 120.0                                                                            # matte, sigma clamped to 90
    H.pbrt_host_material_resolve(C.byref(P), C.byref(m), C.byref(r))
    sig = f32(np.pi / 180) * f32(90); s2 = sig * sig
    assert m.sigma == 90.0 and f32(r.on_a) == f32(1) - (s2 / (f32(2) * (s2 + f32(.33)))) and f32(r.on_b) == f32(.45) * s2 / (s2 + f32(.09))
    assert C.sizeof(pkg.RtMaterial) == 64 and C.sizeof(pkg.RtMaterialResolved) == 84 and C.sizeof(pkg.RtTexture) == 168


# ---- what must not move -------------------------------------------------------------------------------------------------------------------
def test_descriptor_images_of_existing_scenes_are_unchanged(pkg):
    parent = {"plastic_whitted": "6044150839fb80d1951125c816b42add70272de79f9a50c541c793ee4519e1c3",
              "direct_spot_area": "b9e1e8fc003a80bcb82cad4a2546f75c81447be404622824f5f72055e07469f9"}
    for name, sha in parent.items():
        ps = pkg.ParsedScene(text=load_golden(name)["scene"])
        assert ps.errors == 0 and hashlib.sha256(ps.serialize()).hexdigest() == sha, name
        assert not ps.has_textures() and ps.textures() == []


def test_constant_textures_fold_and_make_no_table(pkg, scenes):
    a = parse(pkg, scenes, 'Texture "gold" "color" "constant" "color value" [.8 .6 .2]\nTexture "r" "float" "constant" "float value" [.3]\n'
                           'Material "plastic" "texture Kd" "gold" "texture roughness" "r"\n' + TRI % "")
    b = parse(pkg, scenes, 'Material "plastic" "color Kd" [.8 .6 .2] "float roughness" [.3]\n' + TRI % "")
    assert a.errors == 0 and not a.has_textures() and a.textures() == [] and "textured" not in a.materials()[0]
    assert a.serialize() == b.serialize()


def test_fixtures_present():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "textures", "*.npz")))
    assert len(paths) >= 12, paths
    for p in paths:
        assert os.path.getsize(p) < 64 * 1024, p
        z = np.load(p)
        assert float(z["flat_share"]) >= 0.05, (p, float(z["flat_share"]))
        assert z["rgb"].shape[0] in (24, 32) and np.isfinite(z["rgb"]).all()
