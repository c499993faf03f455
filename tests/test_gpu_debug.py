"""The debug integrator (SurfaceIntegrator "debug", integrators/debug.cpp) on the device against the unmodified reference: the fixtures of
tests/golden/debug/ (tests/golden/make_debug_golden.py), their wrong twins as different films, the kernel flavours, rt_scene_create_prebuilt and a
two-shard split against one frame, a scene without lights, alpha on the misses, the hit channel against another integrator's alpha, the refusal.
Bars: the triangle fixtures and the one in a medium are held to the strict bar -- every pixel's rgb and alpha within 1e-5, ray
counts equal --, the quadric fixture, whose (u, v) and normals pass through the device's libm, to the loose one.  No allow-list."""
import re

import numpy as np
import pytest

from conftest import load_golden
from gpu_checks import (PIPELINE_ENVS, assert_flavours_agree, assert_prebuilt_agrees, assert_two_shards_agree, check_bar, check_counts,
                        differing_share, fixture_names, need_gpu, render_both)

pytestmark = pytest.mark.gpu

ALL = fixture_names("debug")
LOOSE = ("debug_quadrics_grid",)                       # sphere / disk / cylinder: atan2f, acosf, sqrtf
WIDE_FILTER = ("debug_lens_gauss_crop",)               # a Gaussian filter wider than a pixel: two shards add to one pixel, in another order
TWIN_KEPT = ("debug_default_uv", "debug_normals_mesh", "debug_quadrics_grid")
DEBUG_RE = re.compile(r'^SurfaceIntegrator "debug"[^\n]*\n', re.M)


def as_whitted(text):
    out, n = DEBUG_RE.subn('SurfaceIntegrator "whitted" "integer maxdepth" [5]\n', text)
    assert n == 1
    return out


def with_channels(text, red, green, blue):
    out, n = DEBUG_RE.subn('SurfaceIntegrator "debug" "string red" ["%s"] "string green" ["%s"] "string blue" ["%s"]\n' % (red, green, blue), text)
    assert n == 1
    return out


def test_fixtures_present():
    assert len(ALL) == 8, ALL


@pytest.mark.parametrize("name", ALL)
def test_debug_film_matches_reference_fixture(pkg, name):
    """Counting twin (film + ray counts) and timed kernel against the reference's film."""
    need_gpu(pkg)
    g = load_golden("debug/" + name)
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    assert ps.integrator == pkg.RT_INTEGRATOR_DEBUG
    loose = name in LOOSE
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], loose)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], loose)
    check_counts(name, cnt, g["stats"], loose)
    assert cnt["any_rays"] == 0 and cnt["closest_rays"] == cnt["camera_rays"]              # one camera ray per sample and nothing else


@pytest.mark.parametrize("name", ALL)
def test_flavours_prebuilt_scene_and_two_shards_agree(pkg, name):
    """Timed kernel and counting twin under both PBRT_HIP_HIGH_OCC settings and under PBRT_HIP_PIPELINE=1 -- a debug frame always runs its own
    megakernel, pipeline == 0 --, rt_scene_create_prebuilt, and two shards of 8 x 8 tiles summed: the film and the counters of one frame."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("debug/" + name)["scene"])
    ds = pkg.DeviceScene(ps)
    ref, cnt_ref = assert_flavours_agree(ds, name, PIPELINE_ENVS, expect_pipeline=0)
    ds.close()
    b = assert_prebuilt_agrees(pkg, ps, ref, cnt_ref)
    assert_two_shards_agree(ps, b, ref, cnt_ref, exact=name not in WIDE_FILTER)
    b.close()


@pytest.mark.parametrize("name", TWIN_KEPT)
def test_the_twin_film_is_another_film(pkg, name):
    """The device's film is as far from the reference's film of the wrong twin (channels exchanged / the geometric normal for the shading normal)
    as the fixture's own film is."""
    need_gpu(pkg)
    g = load_golden("debug/" + name)
    assert float(g["twin_share"]) >= 0.05
    rgb, _, _, _ = pkg.render_text(g["scene"])
    share = differing_share(rgb, g["twin_rgb"])
    print(name, "differs from its twin", str(g["twin"]), "on", share)
    assert share >= 0.05, (name, share)


def test_scene_without_lights_renders_the_same_film(pkg):
    """The integrator reads no light: fixture 1's scene without its light gives the bit-identical accumulators."""
    need_gpu(pkg)
    text = load_golden("debug/debug_default_uv")["scene"]
    dark, n = re.subn(r'^LightSource [^\n]*\n', "", text, flags=re.M)
    assert n == 1
    films = []
    for t in (text, dark):
        ps = pkg.ParsedScene(text=t)
        assert ps.valid and ps.errors == 0 and ps.n_lights == (1 if t is text else 0)
        ds = pkg.DeviceScene(ps)
        ds.render()
        films.append(ds.film_accum())
        ds.close()
    assert np.isfinite(films[1]).all() and films[1][:3].max() > 0
    assert np.array_equal(films[0], films[1])


def test_alpha_is_one_on_the_misses_too(pkg):
    """debug.cpp:69.  The same scene under "whitted" has alpha below 0.5 on the empty half: the scene does have misses."""
    need_gpu(pkg)
    g = load_golden("debug/debug_one_zero")
    _, alpha, _, _ = pkg.render_text(g["scene"])
    assert np.abs(alpha - 1.0).max() <= 1e-5, float(np.abs(alpha - 1.0).max())
    _, walpha, _, _ = pkg.render_text(as_whitted(g["scene"]))
    print("whitted: pixels with alpha < 0.5:", float((walpha < 0.5).mean()))
    assert float((walpha < 0.5).mean()) >= 0.25


def test_hit_channel_is_the_coverage_of_another_integrator(pkg, scenes):
    """Device against device, without jitter (no integrator's draws move the image samples): the `hit` channel of a debug frame is the alpha of the
    whitted frame of the same scene, and the hit-dependent channels are 0 where it is 0."""
    need_gpu(pkg)
    world = load_golden("debug/debug_normals_mesh")["scene"]
    world = world[world.index("WorldBegin"):]
    kw = dict(xres=24, yres=24, xsamples=2, ysamples=2, jitter=False)
    rgb, alpha, _, _ = pkg.render_text(scenes.options_block(integrator="debug", integrator_params='"string red" ["hit"] "string green" ["snz"] "string blue" ["u"]', **kw) + world)
    _, walpha, _, _ = pkg.render_text(scenes.options_block(integrator="whitted", **kw) + world)
    assert 0.05 < float((walpha < 0.5).mean()) < 0.95                                   # covered and empty pixels both occur
    assert np.abs(rgb[..., 0] - walpha).max() <= 1e-5, float(np.abs(rgb[..., 0] - walpha).max())
    assert np.abs(alpha - 1.0).max() <= 1e-5
    assert np.abs(rgb[walpha == 0.0]).max() <= 1e-5


def test_refusal_of_an_unknown_channel_code(pkg):
    """A channel code of 11 in the descriptor is refused by rt_render (RT_EINVAL) before anything is launched; restored, the frame renders."""
    need_gpu(pkg)
    g = load_golden("debug/debug_one_zero")
    ps = pkg.ParsedScene(text=g["scene"])
    ds = pkg.DeviceScene(ps)
    rd = ps.render_struct()
    good = rd.strategy
    assert good == (pkg.RT_DEBUG_ONE | pkg.RT_DEBUG_ZERO << 8 | pkg.RT_DEBUG_SNY << 16)
    try:
        for bad in ((good & ~0xff) | 11, (good & ~0xff00) | 11 << 8, (good & ~0xff0000) | 11 << 16, good | 1 << 24):
            rd.strategy = bad
            with pytest.raises(pkg.RtError) as e:
                ds.render()
            assert "rt error -1" in str(e.value) and "debug" in str(e.value), str(e.value)
    finally:
        rd.strategy = good
    ds.render()
    rgb, alpha = ds.film()
    ds.close()
    check_bar("restored", rgb, alpha, g["rgb"], g["alpha"], False)
