"""Host front end of the shinymetal and translucent materials (materials/shinymetal.cpp:43-73, materials/translucent.cpp:45-94): parameter
names, defaults, .Clamp(), named constant textures, shape parameters over material parameters, what is derived once on the host
(FresnelApproxEta core/reflection.cpp:52-56, the reflect / transmit products, the lobes present), the loud fall-back of every other unknown
material, and the descriptor images that must not move.  CPU only, through ParsedScene.materials()."""
import glob
import hashlib
import os

import numpy as np

from conftest import GOLDEN, load_golden

TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0] %s\n'
f32 = np.float32


def parse(pkg, scenes, world):
    hdr = scenes.options_block(xres=16, yres=16, integrator="whitted")
    return pkg.ParsedScene(text=hdr + 'WorldBegin\nLightSource "point" "point from" [278 500 200] "color I" [100000 100000 100000]\n' + world + "WorldEnd\n")


def one(pkg, scenes, material, shape_params="", pre=""):
    ps = parse(pkg, scenes, pre + "Material " + material + "\n" + TRI % shape_params)
    mats = ps.materials()
    assert ps.valid and len(mats) == 1 == ps.n_materials
    return ps, mats[0]


def approx_eta(fr):
    """FresnelApproxEta in float32: Clamp(0, .999), (1 + sqrt) / (1 - sqrt)"""
    r = np.clip(np.asarray(fr, f32), f32(0), f32(.999)).astype(f32)
    s = np.sqrt(r, dtype=f32)
    return ((f32(1) + s) / (f32(1) - s)).astype(f32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def test_shinymetal_defaults(pkg, scenes):
    ps, m = one(pkg, scenes, '"shinymetal"')
    assert ps.errors == 0 and ps.warnings == 0
    assert m["type"] == "shinymetal" and m["roughness"] == float(f32(.1))
    assert same_bits(m["Ks"], [1, 1, 1]) and same_bits(m["Kr"], [1, 1, 1])
    assert m["lobes"] == ["glossy_reflection", "specular_reflection"]
    assert same_bits(m["eta_Ks"], approx_eta([1, 1, 1])) and same_bits(m["eta_Kr"], approx_eta([1, 1, 1]))      # 1 is clamped to .999


def test_shinymetal_parameters_clamp_and_eta(pkg, scenes):
    ps, m = one(pkg, scenes, '"shinymetal" "color Ks" [.8 -2 .9995] "color Kr" [0 .25 7] "float roughness" [.35]')
    assert ps.errors == 0 and ps.warnings == 0
    assert same_bits(m["Ks"], [.8, 0, .9995]) and same_bits(m["Kr"], [0, .25, 7]) and m["roughness"] == float(f32(.35))      # .Clamp(): below 0 only
    assert same_bits(m["eta_Ks"], approx_eta([.8, 0, .9995])) and same_bits(m["eta_Kr"], approx_eta([0, .25, 7]))
    assert m["eta_Ks"][1] == 1.0 and m["eta_Kr"][0] == 1.0 and m["eta_Kr"][1] == 3.0                              # black: eta 1; .25: (1 + .5) / (1 - .5)
    assert m["eta_Ks"][2] == m["eta_Kr"][2] == approx_eta([.999])[0]
    assert m["lobes"] == ["glossy_reflection", "specular_reflection"]                                             # both lobes always (shinymetal.cpp:60-61)


def test_translucent_defaults(pkg, scenes):
    ps, m = one(pkg, scenes, '"translucent"')
    assert ps.errors == 0 and ps.warnings == 0
    assert m["type"] == "translucent" and m["roughness"] == float(f32(.1))
    assert same_bits(m["Kd"], [1, 1, 1]) and same_bits(m["Ks"], [1, 1, 1]) and same_bits(m["reflect"], [.5, .5, .5]) and same_bits(m["transmit"], [.5, .5, .5])
    for k in ("reflect*Kd", "transmit*Kd", "reflect*Ks", "transmit*Ks"):
        assert same_bits(m[k], [.5, .5, .5]), k
    assert m["lobes"] == ["diffuse_reflection", "diffuse_transmission", "glossy_reflection", "glossy_transmission"]


def test_translucent_parameters_and_products(pkg, scenes):
    ps, m = one(pkg, scenes, '"translucent" "color Kd" [.4 .5 -1] "color Ks" [.3 .7 .9] "color reflect" [.6 .1 2] "color transmit" [.2 .8 .3] "float roughness" [.25]')
    assert ps.errors == 0 and ps.warnings == 0
    kd, ks, r, t = (np.array(v, f32) for v in ([.4, .5, 0], [.3, .7, .9], [.6, .1, 2], [.2, .8, .3]))
    assert same_bits(m["Kd"], kd) and same_bits(m["Ks"], ks) and same_bits(m["reflect"], r) and same_bits(m["transmit"], t)
    assert same_bits(m["reflect*Kd"], r * kd) and same_bits(m["transmit*Kd"], t * kd) and same_bits(m["reflect*Ks"], r * ks) and same_bits(m["transmit*Ks"], t * ks)
    assert m["roughness"] == 0.25 and len(m["lobes"]) == 4


def test_translucent_lobe_presence(pkg, scenes):
    """translucent.cpp:56-78: a lobe exists iff its two colours are not black (the colours, not their product)."""
    D, DT, G, GT = "diffuse_reflection", "diffuse_transmission", "glossy_reflection", "glossy_transmission"
    for params, lobes in (('"color reflect" [0 0 0]', [DT, GT]), ('"color transmit" [0 0 0]', [D, G]), ('"color Kd" [0 0 0]', [G, GT]),
                          ('"color Ks" [0 0 0]', [D, DT]), ('"color reflect" [0 0 0] "color transmit" [0 0 0]', []),
                          ('"color Kd" [0 0 0] "color Ks" [0 0 0]', []), ('"color reflect" [0 0 0] "color Ks" [0 0 0]', [DT]),
                          ('"color reflect" [1 0 0] "color Kd" [0 1 0]', [D, DT, G, GT])):           # a black product is still a lobe
        ps, m = one(pkg, scenes, '"translucent" ' + params)
        assert ps.errors == 0 and ps.warnings == 0 and m["lobes"] == lobes, (params, m["lobes"])


def test_named_constant_textures_and_shape_overrides(pkg, scenes):
    pre = ('Texture "gold" "color" "constant" "color value" [.9 .7 .2]\nTexture "rough" "float" "constant" "float value" [.3]\n'
           'Texture "thin" "color" "constant" "color value" [.1 .2 .3]\n')
    ps, m = one(pkg, scenes, '"shinymetal" "texture Ks" "gold" "texture roughness" "rough" "color Kr" [.5 .5 .5]', pre=pre)
    assert ps.errors == 0 and ps.warnings == 0
    assert same_bits(m["Ks"], [.9, .7, .2]) and m["roughness"] == float(f32(.3)) and same_bits(m["eta_Ks"], approx_eta([.9, .7, .2]))
    # shape parameters come before material parameters (TextureParams, paramset.cpp:434-465)
    ps, m = one(pkg, scenes, '"shinymetal" "color Kr" [.5 .5 .5] "float roughness" [.2]', shape_params='"color Kr" [.1 .2 .3] "float roughness" [.4]')
    assert ps.errors == 0 and same_bits(m["Kr"], [.1, .2, .3]) and m["roughness"] == float(f32(.4))
    ps, m = one(pkg, scenes, '"translucent" "texture transmit" "thin" "color reflect" [.9 .9 .9]', shape_params='"color reflect" [0 0 0] "texture Kd" "gold"', pre=pre)
    assert ps.errors == 0
    assert same_bits(m["transmit"], [.1, .2, .3]) and same_bits(m["reflect"], [0, 0, 0]) and same_bits(m["Kd"], [.9, .7, .2])
    assert m["lobes"] == ["diffuse_transmission", "glossy_transmission"]


def test_misspelt_parameter_and_constant_bumpmap_warn(pkg, scenes):
    ps, m = one(pkg, scenes, '"translucent" "float rougness" [.3]')
    assert ps.errors == 0 and ps.warnings >= 1 and m["type"] == "translucent" and m["roughness"] == float(f32(.1))
    ps, m = one(pkg, scenes, '"shinymetal" "color Kd" [.3 .3 .3]')
    assert ps.errors == 0 and ps.warnings >= 1 and m["type"] == "shinymetal"
    ps, m = one(pkg, scenes, '"shinymetal" "float bumpmap" [.5]')
    assert ps.errors == 0 and ps.warnings == 1 and m["type"] == "shinymetal"


def test_other_unknown_materials_still_fall_back_loudly(pkg, scenes):
    for name in ("felt", "substrate", "Shinymetal"):
        ps, m = one(pkg, scenes, '"%s" "color Kd" [.2 .3 .4]' % name)
        assert ps.errors == 1 and m["type"] == "matte" and same_bits(m["Kd"], [.2, .3, .4]), name


def test_existing_materials_read_back(pkg, scenes):
    ps = parse(pkg, scenes, 'Material "plastic" "color Ks" [.2 .3 .4] "float roughness" [.3]\n' + TRI % "" + 'Material "glass" "float index" [1.25]\n' + TRI % "" +
               'Material "mirror"\n' + TRI % "" + 'Material "matte" "float sigma" [20]\n' + TRI % "")
    a, b, c, d = ps.materials()
    assert ps.errors == 0 and a["type"] == "plastic" and same_bits(a["Ks"], [.2, .3, .4]) and b["type"] == "glass" and b["index"] == 1.25
    assert c["type"] == "mirror" and d["type"] == "matte" and d["sigma"] == 20.0


def test_existing_descriptors_do_not_move(pkg):
    """serialize() of scenes that were there before: the SHA-256 of the image the parent commit gave."""
    parent = {"plastic_whitted": "6044150839fb80d1951125c816b42add70272de79f9a50c541c793ee4519e1c3"}
    for name, sha in parent.items():
        ps = pkg.ParsedScene(text=load_golden(name)["scene"])
        assert ps.errors == 0 and hashlib.sha256(ps.serialize()).hexdigest() == sha, name
    import ctypes as C
    assert C.sizeof(pkg.RtMaterial) == 64 and pkg.RtMaterial.ks.offset == 36 and pkg.RtMaterial.kr.offset == 52


def test_fixtures_present():
    names = sorted(glob.glob(os.path.join(GOLDEN, "materials", "*.npz")))
    assert len(names) >= 8, names
    for p in names:
        z = np.load(p)
        assert float(z["matte_share"]) >= 0.05, (p, float(z["matte_share"]))
        assert os.path.getsize(p) < 64 * 1024, p
