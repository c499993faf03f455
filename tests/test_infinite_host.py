"""Host front end of the infinite area light (lights/infinite.cpp:163-169 CreateLight, :66-82 the constructor): parameter names and defaults,
unused parameters, the radiance map that is refused loudly, the light types that stay errors, the descriptor images that must not move, and
the fixtures of tests/golden/infinite/.  CPU only, through ParsedScene.lights()."""
import ctypes as C
import glob
import hashlib
import os

import numpy as np

from conftest import GOLDEN, load_golden

f32 = np.float32
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\n'


def parse(pkg, scenes, world, **kw):
    hdr = scenes.options_block(xres=16, yres=16, integrator="whitted")
    return pkg.ParsedScene(text=hdr + "WorldBegin\n" + world + TRI + "WorldEnd\n", **kw)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def test_defaults(pkg, scenes):
    ps = parse(pkg, scenes, 'LightSource "infinite"\n')
    assert ps.valid and ps.errors == 0 and ps.warnings == 0 and ps.n_lights == 1
    (l,) = ps.lights()
    assert l["type"] == "infinite" and l["nsamples"] == 1 and same_bits(l["L"], [1, 1, 1])


def test_explicit_parameters_read_back_bit_for_bit(pkg, scenes):
    ps = parse(pkg, scenes, 'LightSource "infinite" "color L" [.2 .4 17.25] "integer nsamples" [4]\n')
    assert ps.errors == 0 and ps.warnings == 0 and ps.n_lights == 1
    (l,) = ps.lights()
    assert l["type"] == "infinite" and l["nsamples"] == 4 and same_bits(l["L"], [.2, .4, 17.25])
    # Light's constructor keeps max(1, ns) (light.h:39); L is not clamped (infinite.cpp:81)
    ps = parse(pkg, scenes, 'LightSource "infinite" "color L" [-1 0 2] "integer nsamples" [0]\n')
    (l,) = ps.lights()
    assert ps.errors == 0 and l["nsamples"] == 1 and same_bits(l["L"], [-1, 0, 2])


def test_light_to_world_transform_is_accepted_and_order_kept(pkg, scenes):
    """The transform only orients a radiance map: with a constant L the record is the same.  Lights keep the scene's order."""
    a = parse(pkg, scenes, 'LightSource "point" "point from" [1 2 3]\nLightSource "infinite" "color L" [.3 .2 .1]\n')
    b = parse(pkg, scenes, 'LightSource "point" "point from" [1 2 3]\nAttributeBegin\nRotate 40 0 1 0\nScale 2 3 4\nLightSource "infinite" "color L" [.3 .2 .1]\nAttributeEnd\n')
    assert a.errors == 0 and b.errors == 0 and a.n_lights == b.n_lights == 2
    assert [l["type"] for l in a.lights()] == ["point", "infinite"] == [l["type"] for l in b.lights()]
    assert a.serialize() == b.serialize()


def test_misspelt_parameter_warns(pkg, scenes):
    ps = parse(pkg, scenes, 'LightSource "infinite" "color Ll" [.2 .4 .6]\n')
    (l,) = ps.lights()
    assert ps.errors == 0 and ps.warnings >= 1 and same_bits(l["L"], [1, 1, 1])
    ps = parse(pkg, scenes, 'LightSource "infinite" "integer samples" [4]\n')
    assert ps.errors == 0 and ps.warnings >= 1 and ps.lights()[0]["nsamples"] == 1


def test_mapname_is_an_error_and_keeps_L(pkg, scenes):
    ps = parse(pkg, scenes, 'LightSource "infinite" "color L" [.2 .4 .6] "string mapname" ["sky.exr"] "integer nsamples" [2]\n')
    assert ps.valid and ps.errors == 1 and ps.warnings == 0 and ps.n_lights == 1
    (l,) = ps.lights()
    assert l["type"] == "infinite" and l["nsamples"] == 2 and same_bits(l["L"], [.2, .4, .6])
    ps = parse(pkg, scenes, 'LightSource "infinite" "string mapname" [""]\n')            # the empty name is the default: no map asked for
    assert ps.errors == 0 and ps.n_lights == 1


def test_other_unknown_lights_stay_errors(pkg, scenes):
    for name in ("goniometric", "projection", "infinitesample", "Infinite"):
        ps = parse(pkg, scenes, 'LightSource "%s"\n' % name)
        assert ps.errors == 1 and ps.n_lights == 0, name


def test_existing_lights_read_back(pkg, scenes):
    ps = parse(pkg, scenes, 'LightSource "point" "point from" [1 2 3] "color I" [4 5 6]\nLightSource "distant" "point from" [0 2 0] "point to" [0 0 0] "color L" [.5 .5 .25]\n'
               'LightSource "spot" "color I" [7 8 9]\n')
    a, b, c = ps.lights()
    assert ps.errors == 0 and a["type"] == "point" and same_bits(a["I"], [4, 5, 6]) and same_bits(a["from"], [1, 2, 3])
    assert b["type"] == "distant" and same_bits(b["L"], [.5, .5, .25]) and same_bits(b["dir"], [0, 1, 0]) and c["type"] == "spot" and same_bits(c["I"], [7, 8, 9])


def test_existing_descriptors_do_not_move(pkg):
    """RtLight keeps its size and offsets, and serialize() of scenes that were there before gives the SHA-256 of the image the parent commit gave."""
    L = pkg.RtLight
    assert C.sizeof(L) == 108
    offs = dict(type=0, color=4, pos=16, n_samples=28, first_tri=32, n_tris=36, reverse_orientation=40, flip_normal=44, dir=48, world_to_light=60,
                cos_total_width=96, cos_falloff_start=100, quadric_plus1=104)
    for n, o in offs.items():
        assert getattr(L, n).offset == o, n
    parent = {"direct_spot_area": "b9e1e8fc003a80bcb82cad4a2546f75c81447be404622824f5f72055e07469f9",
              "whitted_spot_distant": "48605c0e3a09f3afbca8b207b01bd56aa22a016caa4b91c27f7cbca72ad4acf9",
              "direct_one_point_and_area": "678446067ec657c8d14ed6ef361ca73c0f8396f5ad0bb84a528f4295c5ec53c8"}
    for name, sha in parent.items():
        ps = pkg.ParsedScene(text=load_golden(name)["scene"])
        assert ps.errors == 0 and hashlib.sha256(ps.serialize()).hexdigest() == sha, name


def test_fixtures_present_and_parse():
    names = sorted(glob.glob(os.path.join(GOLDEN, "infinite", "*.npz")))
    assert len(names) >= 10, names
    for p in names:
        z = np.load(p)
        if os.path.basename(p) != "inf_black.npz":
            assert float(z["dark_share"]) >= 0.05, (p, float(z["dark_share"]))
        assert os.path.getsize(p) < 64 * 1024, p
        assert z["rgb"].shape[0] in (16, 24, 32) and np.isfinite(z["rgb"]).all()


def test_fixture_scenes_parse_without_errors(pkg):
    for p in sorted(glob.glob(os.path.join(GOLDEN, "infinite", "*.npz"))):
        name = os.path.basename(p)[:-4]
        ps = pkg.ParsedScene(text=load_golden("infinite/" + name)["scene"])
        assert ps.valid and ps.errors == 0 and sum(l["type"] == "infinite" for l in ps.lights()) == 1, name
