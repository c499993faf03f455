"""Density media on the device (DensityRegion with ExponentialDensity / VolumeGrid, rt_scene_set_density), against the unmodified
reference: the fixtures of tests/golden/density/ (tests/golden/make_density_golden.py), one live frame when oracle/_ref travelled with
the tree, the kernel flavours and both scene-creation paths against each other, and rt_render's refusal of a march that cannot advance.
Bars are those of tests/test_gpu_parity.py: Whitted / DirectLighting every pixel within 1e-5; path >= 99.5 % of the pixels with
per-pixel L2 < 1e-4 and mean L2 < 1e-4; ray counts equal to the reference's."""
import glob
import os

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import GOLDEN, film_metrics, load_golden

pytestmark = pytest.mark.gpu

DENSITY = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "density", "*.npz")))
PATH = 2


def need_gpu(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")


def check_bar(name, rgb, alpha, ref_rgb, ref_alpha, integrator):
    m = film_metrics(rgb, ref_rgb)
    assert np.isfinite(rgb).all(), name
    if integrator == PATH:
        assert m["frac"] >= 0.995 and m["mean_l2"] < 1e-4, (name, m)
    else:
        assert m["maxabs"] <= 1e-5, (name, m)
        assert float(np.abs(alpha - ref_alpha).max()) <= 1e-5, name
    return m


def test_fixtures_present():
    assert len(DENSITY) >= 7, DENSITY


@pytest.mark.parametrize("name", DENSITY)
def test_density_film_matches_reference_fixture(pkg, name):
    need_gpu(pkg)
    g = load_golden("density/" + name)
    ps = pkg.ParsedScene(text=g["scene"])
    assert ps.valid and ps.volume()["density"] is not None
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    ds.set_counting(False); ds.clear_film(); ds.render()           # the timed kernels, against the reference directly
    trgb, talpha = ds.film()
    ds.close()
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], ps.integrator)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], ps.integrator)
    st = g["stats"]
    assert cnt["closest_rays"] == st["closest_rays"] and cnt["any_rays"] == st["any_rays"], (name, cnt, st["closest_rays"], st["any_rays"])
    assert cnt["camera_rays"] == int(st["stats"]["Camera Rays Traced"]) and cnt["bad_samples"] == 0


def test_density_without_the_region_differs(pkg):
    """The fixtures see the medium: the same frame with the region's density ignored (a homogeneous region of the same constants) is another film."""
    need_gpu(pkg)
    g = load_golden("density/dens_grid_single_direct_grid")
    import re
    text = re.sub(r'Volume "volumegrid" [^\n]*', 'Volume "homogeneous" "point p0" [30 20 40] "point p1" [520 500 530] "color sigma_a" [.002 .0025 .003] '
                  '"color sigma_s" [.003 .003 .0025]', g["scene"])
    rgb, _, _, _ = pkg.render_text(text)
    assert film_metrics(rgb, g["rgb"])["maxabs"] > 1e-3


@pytest.mark.parametrize("name", ["dens_exp_single_whitted", "dens_grid_single_direct_grid", "dens_grid_xform_path", "dens_exp_emission_path",
                                  "dens_grid_emission_whitted_ld"])
def test_density_kernel_flavours_give_the_same_film(pkg, name, monkeypatch):
    """Counting twins, timed kernels (both occupancy flavours) and the queue pipeline (per ray, and with 512 slots so that every slot is
    refilled many times) give the bit-identical film, and the pipeline's counting twin the same ray counts."""
    need_gpu(pkg)
    g = load_golden("density/" + name)
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
    for env in (dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="0"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_SLOTS="512")):
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


@pytest.mark.parametrize("name", ["dens_exp_xform_updir_direct_ld", "dens_grid_xform_path"])
def test_prebuilt_scene_takes_the_density_region(pkg, name):
    """rt_scene_create_prebuilt (the multi-rank path) + rt_scene_set_density gives the film of rt_scene_create."""
    need_gpu(pkg)
    g = load_golden("density/" + name)
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


def test_set_density_is_refused_out_of_order(pkg, scenes):
    need_gpu(pkg)
    import ctypes as C
    g = load_golden("density/dens_exp_single_whitted")
    ps = pkg.ParsedScene(text=g["scene"])
    ds = pkg.DeviceScene(ps)                                         # applies the region once
    L = pkg.hip_lib()
    assert L.rt_scene_set_density(ds._s, ps.density_desc()) == -3 and b"already" in L.rt_last_error()
    ds.close()
    plain = pkg.ParsedScene(text=scenes.cornell_scene(xres=8, yres=8))
    ds = pkg.DeviceScene(plain)
    assert L.rt_scene_set_density(ds._s, ps.density_desc()) == -1 and b"no medium" in L.rt_last_error()
    assert L.rt_scene_set_density(ds._s, None) == -1
    ds.close()
    ps2 = pkg.ParsedScene(text=g["scene"].replace('Volume "exponential"', 'Volume "homogeneous"'))
    ds = pkg.DeviceScene(ps2)
    ds.render()
    assert L.rt_scene_set_density(ds._s, ps.density_desc()) == -3 and b"rendered" in L.rt_last_error()
    ds.close()


def test_march_that_cannot_advance_is_refused_before_any_launch(pkg):
    """A camera 3e8 units away: at such t, t + .5 * stepsize == t in float32 -- DensityRegion::Tau's loop would never end."""
    need_gpu(pkg)
    g = load_golden("density/dens_exp_single_whitted")
    text = g["scene"].replace("LookAt 278 273 -800", "LookAt 278 273 -300000000").replace('"float stepsize" [50]', '"float stepsize" [20]')
    assert "-300000000" in text and '"float stepsize" [20]' in text
    ps = pkg.ParsedScene(text=text)
    ds = pkg.DeviceScene(ps)
    ds.bind_film(); ds.clear_film(); ds.reset_counters()
    with pytest.raises(pkg.RtError) as e:
        ds.render()
    assert "would not advance" in str(e.value)
    assert not ds.film_accum().any() and ds.counters()["camera_rays"] == 0
    # the same frame at a sane distance renders
    ds.close()
    ok = pkg.ParsedScene(text=text.replace("LookAt 278 273 -300000000", "LookAt 278 273 -800"))
    ds = pkg.DeviceScene(ok)
    ds.render()
    assert ds.counters()["camera_rays"] > 0
    ds.close()


def test_live_reference_density_frame(pkg, scenes):
    """When oracle/_ref travelled with the tree: a 96 x 96 frame, a 2 k-triangle soup, a 32^3 grid, single scattering, live."""
    need_gpu(pkg)
    rng = np.random.default_rng(5)
    vals = " ".join("%.9g" % v for v in np.round(rng.random(32 ** 3) * 2.0, 3).astype(np.float32))
    vol = ('AttributeBegin\nTranslate 278 0 280\nRotate 15 0 1 0\nVolume "volumegrid" "integer nx" [32] "integer ny" [32] "integer nz" [32] '
           '"point p0" [-250 5 -250] "point p1" [250 540 250] "color sigma_a" [.002 .002 .002] "color sigma_s" [.003 .003 .003] "float g" [.2] '
           '"float density" [%s]\nAttributeEnd\n' % vals)
    text = scenes.cornell_scene(xres=96, yres=96, integrator="directlighting", xsamples=1, ysamples=1, soup_tris=2000, keyed=True, count=True, seed=3,
                                volume_integrator='"single" "float stepsize" [40]', world_kwargs=dict(extra=vol))
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(text, keyed=True)
    except FileNotFoundError:
        pytest.skip("oracle/_ref not on this box")
    rgb, alpha, cnt, _ = pkg.render_text(text)
    check_bar("live", rgb, alpha, ref_rgb, ref_alpha, 1)
    assert cnt["closest_rays"] == st["closest_rays"] and cnt["any_rays"] == st["any_rays"]
