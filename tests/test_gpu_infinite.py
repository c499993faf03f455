"""The infinite area light (LightSource "infinite", lights/infinite.cpp, constant radiance) on the device against the unmodified reference: the
fixtures of tests/golden/infinite/ (tests/golden/make_infinite_golden.py), the exact empty-world frames, the scene without the light as a
different film, the kernel flavours, a two-shard split and both scene-creation paths against each other, the refusals, and one live frame
when oracle/_ref travelled with the tree.
Bars: every direction this light samples passes through the device's sinf / cosf / sqrtf, so the fixture frames are held
to the loose bar -- >= 99.5 % of the pixels with per-pixel L2 < 1e-4 and mean L2 < 1e-4, alpha off on <= 0.5 % of the pixels, ray counts within
max(4, 2e-4 * n), camera rays exact.  The empty-world frames involve no libm: every pixel within 1e-5, alpha 1 everywhere, no shadow rays."""
import re

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import film_metrics, load_golden
from gpu_checks import (PIPELINE_ENVS, assert_flavours_agree, assert_prebuilt_agrees, assert_two_shards_agree, check_bar, check_counts, differing_share,
                        fixture_names, need_gpu, render_both)

pytestmark = pytest.mark.gpu

ALL = fixture_names("infinite")
EXACT = ["inf_empty_whitted", "inf_empty_direct"]
LOOSE = [n for n in ALL if n not in EXACT]
INF_RE = re.compile(r'^LightSource "infinite".*\n', re.M)


def without_light(text):
    out, n = INF_RE.subn("", text)
    assert n == 1
    return out


def test_fixtures_present():
    assert len(LOOSE) >= 8 and all(n in ALL for n in EXACT), ALL


@pytest.mark.parametrize("name", LOOSE)
def test_infinite_film_matches_reference_fixture(pkg, name):
    need_gpu(pkg)
    g = load_golden("infinite/" + name)
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    assert any(l["type"] == "infinite" for l in ps.lights())
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], True)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], True)
    check_counts(name, cnt, g["stats"], True)


@pytest.mark.parametrize("name", EXACT)
def test_empty_world_is_the_sky_exactly(pkg, name):
    """Nothing but LightSource "infinite" "color L" [.2 .4 .6]: every camera ray leaves the scene and returns L (whitted.cpp:52-58,
    directlighting.cpp:186-191), alpha 1; no libm is involved, so the strict bar holds; no shadow ray is ever cast."""
    need_gpu(pkg)
    g = load_golden("infinite/" + name)
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], False)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], False)
    check_counts(name, cnt, g["stats"], False)
    assert cnt["any_rays"] == 0
    for film, a in ((rgb, alpha), (trgb, talpha)):
        assert float(np.abs(film - np.array([.2, .4, .6], np.float32)).max()) <= 1e-5       # L up to the film's filter normalisation
        assert float(a.min()) == 1.0 and float(a.max()) == 1.0


@pytest.mark.parametrize("name", [n for n in LOOSE if n != "inf_black"])
def test_the_scene_without_the_light_is_another_film(pkg, name):
    """What the host did before it knew the light (an error, no light) does not pass for the fixture."""
    need_gpu(pkg)
    g = load_golden("infinite/" + name)
    assert float(g["dark_share"]) >= 0.05
    rgb, _, _, _ = pkg.render_text(without_light(g["scene"]))
    share = differing_share(rgb, g["rgb"])
    print(name, "differs on", share)
    assert share >= 0.05, (name, share)


def test_black_infinite_light_still_counts_as_a_light(pkg):
    """L = 0: misses keep alpha 0 and radiance 0, but the light takes its share of UniformSampleOneLight -- the film and the ray counts are not
    those of the scene without it (the reference's film of that scene is in the fixture)."""
    need_gpu(pkg)
    g = load_golden("infinite/inf_black")
    ps, rgb, alpha, cnt, _, _ = render_both(pkg, g["scene"])
    assert float(alpha.min()) == 0.0                                        # the open front of the box: rays that leave the scene
    drgb, _, dcnt, _ = pkg.render_text(without_light(g["scene"]))
    check_bar("inf_black dark", drgb, alpha, g["dark_rgb"], alpha, True)
    assert film_metrics(rgb, drgb)["maxabs"] > 1e-3 and cnt["any_rays"] != dcnt["any_rays"]
    assert np.array_equal(rgb[alpha == 0.0], np.zeros_like(rgb[alpha == 0.0]))


FLAVOUR_CASES = ["inf_path", "inf_direct_all_ns4_grid_ld", "inf_medium_single_direct"]


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_infinite_kernel_flavours_give_the_same_film(pkg, name):
    """Counting twins, timed kernels (both occupancy flavours) and the queue pipeline (per ray, by path vertex where the frame takes that form, and
    with 512 slots so that every slot is refilled many times) give the bit-identical film, and the counting twins the same ray counts."""
    need_gpu(pkg)
    ds = pkg.DeviceScene(pkg.ParsedScene(text=load_golden("infinite/" + name)["scene"]))
    assert_flavours_agree(ds, name, PIPELINE_ENVS)
    ds.close()


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_two_shards_and_prebuilt_scene_give_the_same_film(pkg, name):
    """Two shards of 8 x 8-pixel tiles, summed, and rt_scene_create_prebuilt (the multi-rank path) give the film of one rt_scene_create frame."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("infinite/" + name)["scene"])
    a = pkg.DeviceScene(ps)
    a.render()
    ref, cnt_ref = a.film_accum(), a.counters()
    a.close()
    b = assert_prebuilt_agrees(pkg, ps, ref, cnt_ref)
    assert_two_shards_agree(ps, b, ref, cnt_ref)          # (the box filter of these frames)
    b.close()


def test_weighted_with_an_infinite_light_is_refused(pkg, scenes):
    """the light draws a random number per estimate, which the survey of WeightedSampleOneLight does not model; rt_render says so
    before launching anything, and the same scene renders with strategy "one"."""
    need_gpu(pkg)
    inf = 'LightSource "infinite" "color L" [.5 .6 .8]\nLightSource "distant" "point from" [0 1 0] "point to" [0 0 0]\n'
    kw = dict(xres=8, yres=8, integrator="directlighting", xsamples=1, ysamples=1, world_kwargs=dict(point_light=True, area_light=False, extra=inf))
    ps = pkg.ParsedScene(text=scenes.cornell_scene(integrator_params='"string strategy" ["weighted"]', **kw))
    assert ps.errors == 0 and ps.n_lights == 3
    ds = pkg.DeviceScene(ps)
    with pytest.raises(pkg.RtError) as e:
        ds.render()
    assert "weighted" in str(e.value) and "infinite" in str(e.value) and "rt error -1" in str(e.value), str(e.value)
    ds.close()
    rgb, alpha, cnt, _ = pkg.render_text(scenes.cornell_scene(integrator_params='"string strategy" ["one"]', **kw))
    assert np.isfinite(rgb).all() and rgb.max() > 0


def test_unknown_light_type_is_refused(pkg, scenes):
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(xres=8, yres=8, world_kwargs=dict(point_light=True)))
    tab = pkg.host_lib().pbrt_host_lights(ps.scene_desc)
    k = [i for i in range(ps.n_lights) if tab[i].type == 0][0]
    try:
        for bad in (5, -1):
            tab[k].type = bad
            with pytest.raises(pkg.RtError) as e:
                pkg.DeviceScene(ps)
            assert "unknown light type" in str(e.value) and "rt error -1" in str(e.value), str(e.value)      # RT_EINVAL
        tab[k].type = 4                                                                                      # the same record as an infinite light: accepted
        pkg.DeviceScene(ps).close()
    finally:
        tab[k].type = 0
    pkg.DeviceScene(ps).close()


def test_live_reference_infinite_frame(pkg, scenes):
    """When oracle/_ref travelled with the tree: a 48 x 48 DirectLighting frame of the Cornell box with a 2 k-triangle soup, its emitter and the sky, live."""
    need_gpu(pkg)
    text = scenes.cornell_scene(xres=48, yres=48, integrator="directlighting", xsamples=1, ysamples=1, soup_tris=2000, keyed=True, count=True, seed=3,
                                world_kwargs=dict(extra='LightSource "infinite" "color L" [.6 .7 .9] "integer nsamples" [2]\n'))
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(text, keyed=True)
    except FileNotFoundError:
        pytest.skip("oracle/_ref not on this box")
    rgb, alpha, cnt, _ = pkg.render_text(text)
    check_bar("live", rgb, alpha, ref_rgb, ref_alpha, True)
    check_counts("live", cnt, st, True)
