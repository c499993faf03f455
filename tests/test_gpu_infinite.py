"""The infinite area light (LightSource "infinite", lights/infinite.cpp, constant radiance) on the device against the unmodified reference: the
fixtures of tests/golden/infinite/ (tests/golden/make_infinite_golden.py), the exact empty-world frames, the scene without the light as a
different film, the kernel flavours, a two-shard split and both scene-creation paths against each other, the refusals, and one live frame
when oracle/_ref travelled with the tree.
Bars: every direction this light samples passes through the device's sinf / cosf / sqrtf, so the fixture frames are held
to the loose bar -- >= 99.5 % of the pixels with per-pixel L2 < 1e-4 and mean L2 < 1e-4, alpha off on <= 0.5 % of the pixels, ray counts within
max(4, 2e-4 * n), camera rays exact.  The empty-world frames involve no libm: every pixel within 1e-5, alpha 1 everywhere, no shadow rays."""
import glob
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import GOLDEN, film_metrics, load_golden, stat_int

pytestmark = pytest.mark.gpu

ALL = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "infinite", "*.npz")))
EXACT = ["inf_empty_whitted", "inf_empty_direct"]
LOOSE = [n for n in ALL if n not in EXACT]
INF_RE = re.compile(r'^LightSource "infinite".*\n', re.M)


def need_gpu(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")


def check_bar(name, rgb, alpha, ref_rgb, ref_alpha, loose):
    m = film_metrics(rgb, ref_rgb)
    print(name, "loose" if loose else "strict", m, "alpha maxabs %.3g off on %.4f" % (float(np.abs(alpha - ref_alpha).max()), float((np.abs(alpha - ref_alpha) > 1e-5).mean())))
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
    tol_c = max(4, int(2e-4 * st["closest_rays"])) if loose else 0
    tol_a = max(4, int(2e-4 * st["any_rays"])) if loose else 0
    assert abs(cnt["closest_rays"] - st["closest_rays"]) <= tol_c and abs(cnt["any_rays"] - st["any_rays"]) <= tol_a, (name, cnt, st["closest_rays"], st["any_rays"])
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
    share = float((np.sqrt(((rgb.astype(np.float64) - g["rgb"]) ** 2).sum(-1)) > 1e-3).mean())
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
def test_infinite_kernel_flavours_give_the_same_film(pkg, name, monkeypatch):
    """Counting twins, timed kernels (both occupancy flavours) and the queue pipeline (per ray, by path vertex where the frame takes that form, and
    with 512 slots so that every slot is refilled many times) give the bit-identical film, and the pipeline's counting twin the same ray counts."""
    need_gpu(pkg)
    g = load_golden("infinite/" + name)
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


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_two_shards_and_prebuilt_scene_give_the_same_film(pkg, name):
    """Two shards of 8 x 8-pixel tiles, summed, and rt_scene_create_prebuilt (the multi-rank path) give the film of one rt_scene_create frame."""
    need_gpu(pkg)
    g = load_golden("infinite/" + name)
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
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    cnt_ref = None
    b.reset_counters(); b.clear_film(); b.render(); cnt_ref = b.counters()
    b.reset_counters(); b.clear_film()
    for shard in range(2):                                  # both shards into one film, as the ranks' films are summed
        ps.set_shard(shard, 2, (8, 8))
        b.render()
    parts = b.film_accum(); cnt = b.counters()
    ps.set_shard(0, 1, 64)
    b.close()
    # the box filter of these frames gives every sample to the one pixel it lies in, and a tile holds whole pixels: a pixel's sum is formed by one shard
    assert np.array_equal(parts, ref), float(np.abs(parts - ref).max())
    for k in ("camera_rays", "closest_rays", "any_rays"):
        assert cnt[k] == cnt_ref[k], (k, cnt[k], cnt_ref[k])


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
