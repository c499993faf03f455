"""Textured material parameters on the device (checkerboard / bilerp / uv / scale / mix with the uv, planar, spherical and cylindrical mappings,
evaluated and resolved per hit by the EXT kernels), against the unmodified reference: the fixtures of tests/golden/textures/
(tests/golden/make_textures_golden.py), the scene without its textures as a different film, the per-hit resolve against the host's, the kernel
flavours and both scene-creation paths against each other, and rt_scene_set_textures' refusals.
Bars are those of tests/gpu_checks.py: Whitted / DirectLighting on triangle-only scenes with uv or planar mapping the strict one; path tracing,
the bidirectional integrator, a quadric, a spherical / cylindrical mapping or a textured sigma the loose one."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import film_metrics, load_golden
from gpu_checks import PIPELINE_ENVS, assert_flavours_agree, assert_prebuilt_agrees, check_bar, check_counts, fixture_names, need_gpu, render_both

pytestmark = pytest.mark.gpu

TEXTURES = fixture_names("textures")
PATH, BIDIR = 2, 3
NONE = '"string aamode" ["none"]'
PANEL = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [60 20 300 500 20 300 500 460 420 60 460 420]\n'
POINT = 'LightSource "point" "point from" [278 300 100] "color I" [90000 85000 70000]\n'


def loose_bar(scene_text, integrator):
    return (integrator in (PATH, BIDIR) or re.search(r'Shape "(sphere|disk|cylinder|cone|paraboloid|hyperboloid)"', scene_text) is not None or
            re.search(r'"string mapping" \["(spherical|cylindrical)"\]', scene_text) is not None or '"texture sigma"' in scene_text)


def flat(text):
    """the scene without its textures: the Texture statements removed, the textured parameters back at their literals or defaults"""
    text = re.sub(r'^Texture [^\n]*\n', '', text, flags=re.M)
    return re.sub(r'\s*"texture \w+" "\w+"', '', text)


def test_fixtures_present():
    assert len(TEXTURES) >= 12, TEXTURES


@pytest.mark.parametrize("name", TEXTURES)
def test_textured_film_matches_reference_fixture(pkg, name):
    need_gpu(pkg)
    g = load_golden("textures/" + name)
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    assert ps.has_textures() and any(m["textured"] for m in ps.materials())
    loose = loose_bar(g["scene"], ps.integrator)
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], loose)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], loose)
    check_counts(name, cnt, g["stats"], loose)


def test_the_scene_without_its_textures_is_another_film(pkg):
    need_gpu(pkg)
    for name in ("chk_default_uv_direct_all_grid_ld", "planar_walls_direct_one"):
        g = load_golden("textures/" + name)
        text = flat(g["scene"])
        assert "Texture" not in text and '"texture' not in text
        rgb, _, _, _ = pkg.render_text(text)
        assert film_metrics(rgb, g["rgb"])["maxabs"] > 1e-3, name


# ---- the per-hit resolve equals the host's: a checkerboard whose two sub-textures are the same constant has that value at every hit, and is not folded on the host
RESOLVE = {   # material -> [(parameter, "color" | "float", value)]
    "matte": [("Kd", "color", ".6 .5 .4"), ("sigma", "float", "30")],
    "mirror": [("Kr", "color", ".8 .7 .9")],
    "glass": [("Kr", "color", ".9 .8 .9"), ("Kt", "color", ".8 .9 .7"), ("index", "float", "1.4")],
    "plastic": [("Kd", "color", ".5 .3 .6"), ("Ks", "color", ".4 .4 .3"), ("roughness", "float", ".15")],
    "uber": [("Kd", "color", ".5 .4 .3"), ("Ks", "color", ".3 .3 .3"), ("Kr", "color", ".2 .1 .2"), ("opacity", "color", ".7 .6 .8"), ("roughness", "float", ".2")],
    "shinymetal": [("Ks", "color", ".8 .6 .3"), ("Kr", "color", ".5 .6 .7"), ("roughness", "float", ".12")],
    "translucent": [("Kd", "color", ".6 .7 .4"), ("Ks", "color", ".3 .2 .3"), ("reflect", "color", ".4 .5 .4"), ("transmit", "color", ".6 .5 .6"), ("roughness", "float", ".18")],
}


@pytest.mark.parametrize("integrator", ["whitted", "directlighting"])
@pytest.mark.parametrize("material", sorted(RESOLVE))
def test_per_hit_resolve_equals_host_resolve(pkg, scenes, material, integrator):
    need_gpu(pkg)
    params = RESOLVE[material]
    tex = "".join('Texture "t_%s" "%s" "checkerboard" "%s tex1" [%s] "%s tex2" [%s] %s "float uscale" [5] "float vscale" [4]\n' % (p, t, t, v, t, v, NONE) for p, t, v in params)
    mat_tex = 'Material "%s" %s\n' % (material, " ".join('"texture %s" "t_%s"' % (p, p) for p, t, v in params))
    mat_lit = 'Material "%s" %s\n' % (material, " ".join('"%s %s" [%s]' % (t, p, v) for p, t, v in params))
    films = []
    for body in (tex + mat_tex, mat_lit):
        text = scenes.cornell_scene(xres=24, yres=24, integrator=integrator, keyed=True, count=True,
                                    world_kwargs=dict(extra=POINT + "AttributeBegin\n" + body + PANEL + "AttributeEnd\n"))
        ps = pkg.ParsedScene(text=text)
        assert ps.errors == 0 and ps.has_textures() == (body is not mat_lit)
        ds = pkg.DeviceScene(ps)
        ds.render()
        films.append((ds.film_accum(), ds.counters()))
        ds.close()
    (a, ca), (b, cb) = films
    assert ca["closest_rays"] == cb["closest_rays"] and ca["any_rays"] == cb["any_rays"], (ca, cb)
    print(material, integrator, "max difference", float(np.abs(a - b).max()))
    if material == "matte":                                     # the issue's exception: Oren-Nayar's A and B are derived on the device
        assert float(np.abs(a - b).max()) <= 1e-5
    else:
        assert np.array_equal(a, b), float(np.abs(a - b).max())


FLAVOUR_CASES = ["nested_mix_plastic_direct", "uber_opacity_path", "glass_checker_whitted", "shiny_medium_direct"]


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_texture_kernel_flavours_give_the_same_film(pkg, name):
    """Counting twins, timed kernels (both occupancy flavours) and the queue pipeline (per ray, and with 512 slots so that every slot is
    refilled many times; by path vertex where the frame takes that form) give the bit-identical film, and the counting twins the same
    ray counts."""
    need_gpu(pkg)
    ds = pkg.DeviceScene(pkg.ParsedScene(text=load_golden("textures/" + name)["scene"]))
    assert_flavours_agree(ds, name, PIPELINE_ENVS)
    ds.close()


@pytest.mark.parametrize("name", ["nested_mix_plastic_direct", "spherical_sphere_path", "kd_bidirectional"])
def test_prebuilt_scene_renders_the_textures(pkg, name):
    """rt_scene_create_prebuilt (the multi-rank path) gives the film of rt_scene_create."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("textures/" + name)["scene"])
    a = pkg.DeviceScene(ps)
    a.render()
    ref = a.film_accum()
    a.close()
    assert_prebuilt_agrees(pkg, ps, ref).close()


# ---- rt_scene_set_textures refuses bad input ------------------------------------------------------------------------------------------------
def table(pkg, ps):
    """A valid table for the scene's first material (matte: slot 0 = Kd): two constants and a checkerboard, and the scene's own material records."""
    nodes = (pkg.RtTexture * 3)()
    for i, col in enumerate(((.8, .2, .2), (.2, .3, .8))):
        nodes[i].kind = 0; nodes[i].is_color = 1
        for c in range(3):
            nodes[i].child[c] = -1; nodes[i].value[c] = col[c]
    nodes[2].kind = 5; nodes[2].is_color = 1; nodes[2].mapping = 0
    nodes[2].child[0] = 0; nodes[2].child[1] = 1; nodes[2].child[2] = -1
    nodes[2].map[0] = 5.0; nodes[2].map[1] = 4.0
    _, _, src, n = ps.texture_table()
    mats = (pkg.RtMaterialTextures * n)()
    C.memmove(mats, src, C.sizeof(pkg.RtMaterialTextures) * n)
    mats[0].tex[0] = 2
    return nodes, mats, n


def test_set_textures_refuses_bad_input(pkg, scenes):
    need_gpu(pkg)
    L = pkg.hip_lib()
    text = scenes.cornell_scene(xres=16, yres=16, integrator="whitted", keyed=True, count=True)
    ps = pkg.ParsedScene(text=text)
    assert not ps.has_textures()
    err = lambda: L.rt_last_error().decode()
    EINVAL, ESTATE = -1, -3

    ds = pkg.DeviceScene(ps)
    nodes, mats, n = table(pkg, ps)
    assert L.rt_scene_set_textures(ds._s, None, 3, mats, n) == EINVAL and "null" in err()                       # a null table
    nodes[2].child[1] = 7
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n) == EINVAL and "out of range" in err()              # a child index out of range
    nodes[2].child[1] = 2
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n) == EINVAL and "cycle" in err()                     # a node that is its own child
    nodes[2].child[1] = 1; nodes[2].kind = 9
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n) == EINVAL and "unknown texture kind" in err()      # an unknown kind
    nodes[2].kind = 5
    mats[0].tex[0] = 3
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n) == EINVAL and "texture index out of range" in err()
    mats[0].tex[0] = 2
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n - 1) == EINVAL and "number of materials" in err()
    # none of the refused calls launched or changed anything: no ray has been counted, and the scene renders the film and the counters of a scene
    # that never saw them, bit for bit; after that frame the call is out of order
    assert all(v == 0 for v in ds.counters().values())
    ds.render()
    plain, plain_cnt = ds.film_accum(), ds.counters()
    fresh = pkg.DeviceScene(ps)
    fresh.render()
    assert np.array_equal(fresh.film_accum(), plain) and fresh.counters() == plain_cnt
    fresh.close()
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n) == ESTATE and "rendered" in err()                  # a call after rt_render
    ds.close()

    ds = pkg.DeviceScene(ps)
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n) == 0
    assert L.rt_scene_set_textures(ds._s, nodes, 3, mats, n) == ESTATE and "already" in err()                   # a second call
    ds.render()                                                                                                 # a valid table still renders: the first wall is checkered now
    tex = ds.film_accum()
    ds.close()
    assert np.isfinite(tex).all() and float(np.abs(tex - plain).max()) > 1e-3
