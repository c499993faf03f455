"""The shinymetal and translucent materials on the device (FresnelConductor lobes; BRDFToBTDF diffuse and glossy transmission), against the
unmodified reference: the fixtures of tests/golden/materials/ (tests/golden/make_materials_golden.py), light through a translucent sheet,
the matte fall-back as a different film, the kernel flavours and both scene-creation paths against each other, one live frame when
oracle/_ref travelled with the tree, and rt_scene_create's refusal of an unknown material type.
Bars are those of tests/gpu_checks.py: Whitted / DirectLighting on triangle-only scenes the strict one, path tracing and frames with a quadric
the loose one."""
import json
import re

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import film_metrics, load_golden
from gpu_checks import PIPELINE_ENVS, assert_flavours_agree, assert_prebuilt_agrees, check_bar, check_counts, fixture_names, need_gpu, render_both

pytestmark = pytest.mark.gpu

MATERIALS = fixture_names("materials")
PATH = 2
T_ONLY_SHEET = '"translucent" "color reflect" [0 0 0] "color transmit" [.8 .8 .8] "float roughness" [.2]'


def loose_bar(scene_text, integrator):
    """path tracing, or a quadric in the frame (device libm in the geometry): the 99.5 % bar"""
    return integrator == PATH or re.search(r'Shape "(sphere|disk|cylinder|cone|paraboloid|hyperboloid)"', scene_text) is not None


def as_matte(text):
    return re.sub(r'Material "(shinymetal|translucent)"', 'Material "matte"', text)


def test_fixtures_present():
    assert len(MATERIALS) >= 8, MATERIALS


@pytest.mark.parametrize("name", MATERIALS)
def test_material_film_matches_reference_fixture(pkg, name):
    need_gpu(pkg)
    g = load_golden("materials/" + name)
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    assert any(m["type"] in ("shinymetal", "translucent") for m in ps.materials())
    loose = loose_bar(g["scene"], ps.integrator)
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], loose)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], loose)
    check_counts(name, cnt, g["stats"], loose)


def test_the_matte_fall_back_is_another_film(pkg):
    """What the host did before it knew the material (an error and "matte") does not pass for the fixture."""
    need_gpu(pkg)
    for name in ("shiny_panel_direct_one", "transl_sheet_direct_weighted"):
        g = load_golden("materials/" + name)
        rgb, _, _, _ = pkg.render_text(as_matte(g["scene"]))
        assert film_metrics(rgb, g["rgb"])["maxabs"] > 1e-3, name


@pytest.mark.parametrize("name", ["sheet_whitted", "sheet_path"])
def test_light_comes_through_a_translucent_sheet(pkg, name):
    """A sheet with transmission lobes only spans the box below the area light; the camera sees its underside.  The reference's films with the
    translucent sheet and with a matte one are both in the fixture; the device is held to both, and the light that reached the far side is
    asserted on the device's own films: Whitted, the rows that show the underside (8-11, columns 8-23; reference .47-1.18 against exactly 0);
    path tracing, the floor below the sheet (rows 26-28, columns 10-21; reference .143 against .00094, a factor of 150)."""
    need_gpu(pkg)
    g = load_golden("materials/" + name)
    assert T_ONLY_SHEET in g["scene"]
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    mps, mrgb, malpha, mcnt, mtrgb, mtalpha = render_both(pkg, as_matte(g["scene"]))
    loose = ps.integrator == PATH
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], loose)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], loose)
    check_counts(name, cnt, g["stats"], loose)
    check_bar(name + " matte", mrgb, malpha, g["matte_rgb"], g["matte_alpha"], loose)
    check_bar(name + " matte timed", mtrgb, mtalpha, g["matte_rgb"], g["matte_alpha"], loose)
    check_counts(name + " matte", mcnt, json.loads(str(g["matte_stats"])), loose)
    for film, mfilm in ((rgb, mrgb), (trgb, mtrgb)):
        if ps.integrator == PATH:
            floor, mfloor = float(film[26:29, 10:22].mean()), float(mfilm[26:29, 10:22].mean())
            print(name, "floor block", floor, "matte", mfloor)
            assert mfloor > 0 and floor >= 50 * mfloor, (floor, mfloor)
        else:
            for r in range(8, 12):
                under, munder = float(film[r, 8:24].mean()), float(np.abs(mfilm[r, 8:24]).max())
                print(name, "row", r, under, "matte", munder)
                assert munder == 0.0 and under > .4, (r, under, munder)


FLAVOUR_CASES = ["shiny_mesh_direct_all_grid_ld", "shiny_mesh_path", "sheet_whitted", "transl_closed_mesh_path_ld", "mix_glass_plastic_path", "sheet_medium_direct"]


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_material_kernel_flavours_give_the_same_film(pkg, name):
    """Counting twins, timed kernels (both occupancy flavours) and the queue pipeline (per ray, and with 512 slots so that every slot is
    refilled many times; by path vertex where the frame takes that form) give the bit-identical film, and the counting twins the same
    ray counts."""
    need_gpu(pkg)
    ds = pkg.DeviceScene(pkg.ParsedScene(text=load_golden("materials/" + name)["scene"]))
    assert_flavours_agree(ds, name, PIPELINE_ENVS)
    ds.close()


@pytest.mark.parametrize("name", ["shiny_sphere_whitted", "transl_sheet_direct_weighted", "transl_closed_mesh_path_ld", "mix_glass_plastic_path"])
def test_prebuilt_scene_renders_the_materials(pkg, name):
    """rt_scene_create_prebuilt (the multi-rank path) gives the film of rt_scene_create."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("materials/" + name)["scene"])
    a = pkg.DeviceScene(ps)
    a.render()
    ref = a.film_accum()
    a.close()
    assert_prebuilt_agrees(pkg, ps, ref).close()


def test_unknown_material_type_is_refused(pkg, scenes):
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(xres=8, yres=8))
    tab = pkg.host_lib().pbrt_host_materials(ps.scene_desc)
    L = pkg.hip_lib()
    keep = tab[0].type
    try:
        for bad in (7, -1):
            tab[0].type = bad
            with pytest.raises(pkg.RtError) as e:
                pkg.DeviceScene(ps)
            assert "unknown material type" in str(e.value) and "rt error -1" in str(e.value), str(e.value)      # RT_EINVAL
    finally:
        tab[0].type = keep
    pkg.DeviceScene(ps).close()


def test_live_reference_materials_frame(pkg, scenes):
    """When oracle/_ref travelled with the tree: a 96 x 96 DirectLighting frame, a 2 k-triangle soup, a shinymetal mesh and a translucent panel, live."""
    need_gpu(pkg)
    extra = ('AttributeBegin\nTranslate 170 120 330\nMaterial "shinymetal" "color Ks" [.8 .6 .3] "color Kr" [.7 .7 .7] "float roughness" [.15]\n' +
             scenes.smooth_mesh_text(radius=100.0) + 'AttributeEnd\nAttributeBegin\nMaterial "translucent" "color Kd" [.5 .7 .4] "float roughness" [.2]\n'
             'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [300 20 250 520 20 350 520 400 420 300 400 320]\nAttributeEnd\n')
    text = scenes.cornell_scene(xres=96, yres=96, integrator="directlighting", xsamples=1, ysamples=1, soup_tris=2000, keyed=True, count=True, seed=3,
                                world_kwargs=dict(extra=extra))
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(text, keyed=True)
    except FileNotFoundError:
        pytest.skip("oracle/_ref not on this box")
    rgb, alpha, cnt, _ = pkg.render_text(text)
    check_bar("live", rgb, alpha, ref_rgb, ref_alpha, False)
    assert cnt["closest_rays"] == st["closest_rays"] and cnt["any_rays"] == st["any_rays"]
