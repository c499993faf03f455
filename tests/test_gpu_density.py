"""Density media on the device (DensityRegion with ExponentialDensity / VolumeGrid, rt_scene_set_density), against the unmodified
reference: the fixtures of tests/golden/density/ (tests/golden/make_density_golden.py), one live frame when oracle/_ref travelled with
the tree, the kernel flavours and both scene-creation paths against each other, and rt_render's refusal of a march that cannot advance.
Bars are those of tests/gpu_checks.py: Whitted / DirectLighting the strict one, path the loose one; ray counts equal to the reference's
under both."""
import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import film_metrics, load_golden
from gpu_checks import PIPELINE_ENVS, assert_flavours_agree, assert_prebuilt_agrees, check_bar, check_counts, fixture_names, need_gpu, render_both

pytestmark = pytest.mark.gpu

DENSITY = fixture_names("density")
PATH = 2


def test_fixtures_present():
    assert len(DENSITY) >= 7, DENSITY


@pytest.mark.parametrize("name", DENSITY)
def test_density_film_matches_reference_fixture(pkg, name):
    need_gpu(pkg)
    g = load_golden("density/" + name)
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])           # (the timed kernels too against the reference directly)
    assert ps.volume()["density"] is not None
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], ps.integrator == PATH)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], ps.integrator == PATH)
    check_counts(name, cnt, g["stats"], False)                                  # exact also under path tracing


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
def test_density_kernel_flavours_give_the_same_film(pkg, name):
    """Counting twins, timed kernels (both occupancy flavours) and the queue pipeline (per ray, and with 512 slots so that every slot is
    refilled many times; the by-vertex setting changes nothing for a frame with a medium) give the bit-identical film, and the counting
    twins the same ray counts."""
    need_gpu(pkg)
    ds = pkg.DeviceScene(pkg.ParsedScene(text=load_golden("density/" + name)["scene"]))
    assert_flavours_agree(ds, name, PIPELINE_ENVS)
    ds.close()


@pytest.mark.parametrize("name", ["dens_exp_xform_updir_direct_ld", "dens_grid_xform_path"])
def test_prebuilt_scene_takes_the_density_region(pkg, name):
    """rt_scene_create_prebuilt (the multi-rank path) + rt_scene_set_density gives the film of rt_scene_create."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("density/" + name)["scene"])
    a = pkg.DeviceScene(ps)
    a.render()
    ref = a.film_accum()
    a.close()
    assert_prebuilt_agrees(pkg, ps, ref).close()


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
    check_bar("live", rgb, alpha, ref_rgb, ref_alpha, False)
    assert cnt["closest_rays"] == st["closest_rays"] and cnt["any_rays"] == st["any_rays"]
