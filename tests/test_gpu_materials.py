"""The shinymetal and translucent materials on the device (FresnelConductor lobes; BRDFToBTDF diffuse and glossy transmission), against the
unmodified reference: the fixtures of tests/golden/materials/ (tests/golden/make_materials_golden.py), light through a translucent sheet,
the matte fall-back as a different film, the kernel flavours and both scene-creation paths against each other, one live frame when
oracle/_ref travelled with the tree, and rt_scene_create's refusal of an unknown material type.
Bars are those of tests/test_gpu_parity.py: Whitted / DirectLighting on triangle-only scenes every pixel within 1e-5 (colour and alpha) with
equal ray counts; path tracing and frames with a quadric >= 99.5 % of the pixels with per-pixel L2 < 1e-4 and mean L2 < 1e-4, ray counts
within max(4, 2e-4 * closest_rays)."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import GOLDEN, film_metrics, load_golden, stat_int

pytestmark = pytest.mark.gpu

MATERIALS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "materials", "*.npz")))
PATH = 2
T_ONLY_SHEET = '"translucent" "color reflect" [0 0 0] "color transmit" [.8 .8 .8] "float roughness" [.2]'


def need_gpu(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")


def loose_bar(scene_text, integrator):
    """path tracing, or a quadric in the frame (device libm in the geometry): the 99.5 % bar"""
    return integrator == PATH or re.search(r'Shape "(sphere|disk|cylinder|cone|paraboloid|hyperboloid)"', scene_text) is not None


def check_bar(name, rgb, alpha, ref_rgb, ref_alpha, loose):
    m = film_metrics(rgb, ref_rgb)
    print(name, "loose" if loose else "strict", m, "alpha maxabs %.3g" % float(np.abs(alpha - ref_alpha).max()))
    assert np.isfinite(rgb).all(), name
    if loose:
        assert m["frac"] >= 0.995 and m["mean_l2"] < 1e-4, (name, m)
        assert (np.abs(alpha - ref_alpha) > 1e-5).mean() <= 0.005, name
    else:
        assert m["maxabs"] <= 1e-5, (name, m)
        assert float(np.abs(alpha - ref_alpha).max()) <= 1e-5, name
    return m


def check_counts(name, cnt, st, loose):
    print(name, "device", cnt["closest_rays"], cnt["any_rays"], "reference", st["closest_rays"], st["any_rays"])
    tol = max(4, int(2e-4 * st["closest_rays"])) if loose else 0
    assert abs(cnt["closest_rays"] - st["closest_rays"]) <= tol and abs(cnt["any_rays"] - st["any_rays"]) <= tol, (name, cnt, st["closest_rays"], st["any_rays"])
    cam, exact = stat_int(st["stats"]["Camera Rays Traced"])          # StatsPrint writes 17424 as "17.4k": equal where it is exact, else equal as printed
    assert (cnt["camera_rays"] == cam if exact else abs(cnt["camera_rays"] - cam) <= .0005 * cam + 50) and cnt["bad_samples"] == 0, (cnt["camera_rays"], cam)


def render_both(pkg, text):
    """counting kernels (film + counters) and timed kernels of one scene text"""
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    ds.set_counting(False); ds.clear_film(); ds.render()
    trgb, talpha = ds.film()
    ds.close()
    return ps, rgb, alpha, cnt, trgb, talpha


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
def test_material_kernel_flavours_give_the_same_film(pkg, name, monkeypatch):
    """Counting twins, timed kernels (both occupancy flavours) and the queue pipeline (per ray, and with 512 slots so that every slot is
    refilled many times; by path vertex where the frame takes that form) give the bit-identical film, and the pipeline's counting twin the
    same ray counts."""
    need_gpu(pkg)
    g = load_golden("materials/" + name)
    ps = pkg.ParsedScene(text=g["scene"])
    ds = pkg.DeviceScene(ps)
    monkeypatch.setenv("PBRT_HIP_PIPELINE", "0")
    ds.render()
    ref = ds.film_accum()
    cnt_ref = ds.counters()
    for occ in ("0", "1"):
        monkeypatch.setenv("PBRT_HIP_HIGH_OCC", occ)
        ds.set_counting(False); ds.clear_film(); ds.render()
        got = ds.film_accum()
        assert np.array_equal(got, ref), (name, occ, float(np.abs(got - ref).max()))
    monkeypatch.delenv("PBRT_HIP_HIGH_OCC")
    for env in (dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="0"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="1"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_SLOTS="512")):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            for counting in (False, True):
                ds.set_counting(counting); ds.reset_counters(); ds.clear_film(); ds.render()
                assert ds.last_stats()["pipeline"] == 1
                got = ds.film_accum()
                assert np.array_equal(got, ref), (name, env, counting, float(np.abs(got - ref).max()))
                if counting:
                    c = ds.counters()
                    for k in ("camera_rays", "closest_rays", "any_rays", "nodes_visited", "leaf_refs", "tri_tests", "bad_samples"):
                        assert c[k] == cnt_ref[k], (name, env, k, c[k], cnt_ref[k])
    ds.close()


@pytest.mark.parametrize("name", ["shiny_sphere_whitted", "transl_sheet_direct_weighted", "transl_closed_mesh_path_ld", "mix_glass_plastic_path"])
def test_prebuilt_scene_renders_the_materials(pkg, name):
    """rt_scene_create_prebuilt (the multi-rank path) gives the film of rt_scene_create."""
    need_gpu(pkg)
    g = load_golden("materials/" + name)
    ps = pkg.ParsedScene(text=g["scene"])
    a = pkg.DeviceScene(ps)
    a.render()
    ref = a.film_accum()
    nodes, refs = a.accel_arrays()
    info = a.accel_info()
    a.close()
    b = pkg.DeviceScene(ps, prebuilt=(nodes, refs, info))
    b.render()
    got = b.film_accum()
    b.close()
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())


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
