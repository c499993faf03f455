"""The bidirectional integrator (SurfaceIntegrator "bidirectional", integrators/bidirectional.cpp) on the device against the unmodified reference:
the fixtures of tests/golden/bidir/ (tests/golden/make_bidir_golden.py), the same scenes under "path" as different films, the kernel flavours,
a two-shard split and both scene-creation paths against each other, another seed, the refusals, and one live frame when oracle/_ref travelled
with the tree.
Bars: every direction here passes through the device's sinf / cosf / sqrtf, so every fixture is held to the loose bar --
>= 99.5 % of the pixels with per-pixel L2 < 1e-4 and mean L2 < 1e-4, alpha off on <= 0.5 % of the pixels, ray counts within max(4, 2e-4 * n),
camera rays exact, no bad samples.  There is no strict-bar case and no allow-list."""
import ctypes as C
import re

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import film_metrics, load_golden
from gpu_checks import assert_prebuilt_agrees, assert_two_shards_agree, check_bar, check_counts, differing_share, fixture_names, need_gpu

pytestmark = pytest.mark.gpu

ALL = fixture_names("bidir")
BIDIR_RE = re.compile(r'^SurfaceIntegrator "bidirectional"[^\n]*\n', re.M)


def as_path(text):
    out, n = BIDIR_RE.subn('SurfaceIntegrator "path" \n', text)
    assert n == 1
    return out


def with_seed(text, seed):
    out, n = re.subn(r'"integer seed" \[\d+\]', '"integer seed" [%d]' % seed, text)
    assert n == 1
    return out


def with_accel(text, name):
    out, n = re.subn(r'\["(kdtree|grid)"\]', '["%s"]' % name, text)
    assert n == 1
    return out


def test_fixtures_present():
    assert len(ALL) >= 8, ALL


@pytest.mark.parametrize("name", ALL)
def test_bidir_film_matches_reference_fixture(pkg, name):
    """Counting twin (film + ray counts) and timed kernel against the reference's film."""
    need_gpu(pkg)
    g = load_golden("bidir/" + name)
    ps = pkg.ParsedScene(text=g["scene"])
    assert ps.valid and ps.errors == 0 and ps.integrator == 3
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    assert ds.last_stats()["pipeline"] == 0
    ds.set_counting(False); ds.clear_film(); ds.render()
    trgb, talpha = ds.film()
    ds.close()
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], True)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], True)
    check_counts(name, cnt, g["stats"], True)


@pytest.mark.parametrize("name", ALL)
def test_the_path_film_is_another_film(pkg, name):
    """The same scene under SurfaceIntegrator "path" does not pass for the fixture."""
    need_gpu(pkg)
    g = load_golden("bidir/" + name)
    assert float(g["path_share"]) >= 0.05
    rgb, _, _, _ = pkg.render_text(as_path(g["scene"]))
    share = differing_share(rgb, g["rgb"])
    print(name, "differs on", share)
    assert share >= 0.05, (name, share)


def test_half_empty_frame_has_alpha_zero_pixels(pkg):
    need_gpu(pkg)
    g = load_golden("bidir/bidir_half_empty")
    rgb, alpha, _, _ = pkg.render_text(g["scene"])
    assert float((alpha == 0.0).mean()) >= 0.25 and float((alpha == 1.0).mean()) >= 0.1        # empty pixels and covered ones both occur
    assert np.array_equal(rgb[alpha == 0.0], np.zeros_like(rgb[alpha == 0.0]))


FLAVOUR_CASES = ["bidir_cornell", "bidir_soup_ext_random", "bidir_spot_distant_grid_ld"]
# fixtures whose film is bit-identical under the other accelerator.  The reference's own films of the two box scenes differ between its kd-tree and its grid
# (111 and 55 of 576 pixels, largest difference 0.0122, other ray counts; the device's grid film of bidir_cornell shows the same largest difference), so
# identity is asserted where the reference has it; the grid kernels match the reference's grid run ray for ray on bidir_spot_distant_grid_ld
ACCEL_IDENTICAL = ["bidir_spot_distant_grid_ld"]


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_bidir_kernel_flavours_give_the_same_film(pkg, name, monkeypatch):
    """Counting twin, timed kernel, two renders in a row and PBRT_HIP_PIPELINE=1 (which this integrator answers in its megakernel form) give the
    bit-identical film; the other accelerator's two kernels agree with each other, and with this film where the fixture allows (ACCEL_IDENTICAL)."""
    need_gpu(pkg)
    g = load_golden("bidir/" + name)
    ps = pkg.ParsedScene(text=g["scene"])
    ds = pkg.DeviceScene(ps)
    ds.render()
    ref = ds.film_accum()
    cnt_ref = ds.counters()
    ds.reset_counters(); ds.clear_film(); ds.render()
    assert np.array_equal(ds.film_accum(), ref)
    cnt = ds.counters()
    for k in ("camera_rays", "closest_rays", "any_rays", "bad_samples"):
        assert cnt[k] == cnt_ref[k], (name, k, cnt[k], cnt_ref[k])
    ds.set_counting(False); ds.clear_film(); ds.render()
    got = ds.film_accum()
    assert np.array_equal(got, ref), (name, float(np.abs(got - ref).max()))
    monkeypatch.setenv("PBRT_HIP_PIPELINE", "1")
    for counting in (False, True):
        ds.set_counting(counting); ds.clear_film(); ds.render()
        assert ds.last_stats()["pipeline"] == 0
        got = ds.film_accum()
        assert np.array_equal(got, ref), (name, counting, float(np.abs(got - ref).max()))
    monkeypatch.delenv("PBRT_HIP_PIPELINE")
    ds.close()
    other = "kdtree" if "grid" in name else "grid"
    po = pkg.ParsedScene(text=with_accel(g["scene"], other))
    do = pkg.DeviceScene(po)
    do.render()
    oref = do.film_accum()
    do.set_counting(False); do.clear_film(); do.render()
    got = do.film_accum()
    do.close()
    assert np.array_equal(got, oref), (name, other, float(np.abs(got - oref).max()))           # the other accelerator's counting twin and timed kernel
    differ = int((np.abs(oref - ref).max(axis=0) > 0).sum())
    print(name, other, "pixels that differ from the fixture's accelerator:", differ)
    if name in ACCEL_IDENTICAL:
        assert differ == 0, (name, other, differ)


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_two_shards_and_prebuilt_scene_give_the_same_film(pkg, name):
    """Two shards of 8 x 8-pixel tiles, summed, and rt_scene_create_prebuilt (the multi-rank path) give the film of one rt_scene_create frame."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("bidir/" + name)["scene"])
    a = pkg.DeviceScene(ps)
    a.render()
    ref, cnt_ref = a.film_accum(), a.counters()
    a.close()
    b = assert_prebuilt_agrees(pkg, ps, ref, cnt_ref)
    assert_two_shards_agree(ps, b, ref, cnt_ref)          # (the box filter of these frames)
    b.close()


def test_samples_read_back(pkg):
    """DeviceScene.samples(): one record per camera sample, finite, alpha 0 or 1."""
    need_gpu(pkg)
    g = load_golden("bidir/bidir_half_empty")
    ps = pkg.ParsedScene(text=g["scene"])
    ds = pkg.DeviceScene(ps)
    ds.render()
    s = ds.samples()
    ds.close()
    assert s.shape == (ps.n_camera_samples, 8) and np.isfinite(s).all()
    assert set(np.unique(s[:, 3])) == {0.0, 1.0}
    assert np.array_equal(s[s[:, 3] == 0.0][:, :3], np.zeros((int((s[:, 3] == 0.0).sum()), 3), np.float32))


def test_another_seed_is_another_film(pkg):
    need_gpu(pkg)
    g = load_golden("bidir/bidir_cornell")
    a, _, _, _ = pkg.render_text(g["scene"])
    b, _, _, _ = pkg.render_text(with_seed(g["scene"], 5))
    assert np.isfinite(b).all() and film_metrics(a, b)["maxabs"] > 1e-3


def test_refusals(pkg, scenes):
    """A participating medium, a scene without lights and an integrator value above 3 are refused by rt_render (RT_EINVAL) before anything is launched;
    the same scenes render under "path"."""
    need_gpu(pkg)
    kw = dict(xres=8, yres=8, xsamples=1, ysamples=1)
    cases = [(dict(world_kwargs=dict(volume='"float g" [.2]'), volume_integrator='"single" "float stepsize" [60]'), ("medium",)),
             (dict(world_kwargs=dict(area_light=False)), ("light",))]
    for extra, words in cases:
        ps = pkg.ParsedScene(text=scenes.cornell_scene(integrator="bidirectional", **kw, **extra))
        assert ps.valid and ps.errors == 0 and ps.integrator == 3
        ds = pkg.DeviceScene(ps)
        with pytest.raises(pkg.RtError) as e:
            ds.render()
        assert "rt error -1" in str(e.value) and "bidirectional" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
        ds.close()
    rgb, _, _, _ = pkg.render_text(scenes.cornell_scene(integrator="path", **kw, **cases[0][0]))
    assert np.isfinite(rgb).all() and rgb.max() > 0
    rgb, _, _, _ = pkg.render_text(scenes.cornell_scene(integrator="path", **kw, **cases[1][0]))       # no light: a finite (black) film
    assert np.isfinite(rgb).all()
    # an integrator value the library does not know
    ps = pkg.ParsedScene(text=scenes.cornell_scene(integrator="bidirectional", **kw))
    ds = pkg.DeviceScene(ps)
    field = np.ctypeslib.as_array(C.cast(ps.render_desc, C.POINTER(C.c_int32)), shape=(1,))      # RtRenderDesc.integrator
    assert field[0] == 3
    field[0] = 4
    try:
        with pytest.raises(pkg.RtError) as e:
            ds.render()
        assert "rt error -1" in str(e.value) and "unknown integrator" in str(e.value), str(e.value)
    finally:
        field[0] = 3
    ds.render()
    rgb, _ = ds.film()
    ds.close()
    assert np.isfinite(rgb).all() and rgb.max() > 0


def test_live_reference_bidir_frame(pkg, scenes):
    """When oracle/_ref travelled with the tree: a 48 x 48 frame of the Cornell box with a 2 k-triangle soup, its emitter and a point light, live."""
    need_gpu(pkg)
    text = scenes.cornell_scene(xres=48, yres=48, integrator="bidirectional", xsamples=1, ysamples=1, soup_tris=2000, keyed=True, count=True, seed=3,
                                world_kwargs=dict(point_light=True))
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(text, keyed=True)
    except FileNotFoundError:
        pytest.skip("oracle/_ref not on this box")
    rgb, alpha, cnt, _ = pkg.render_text(text)
    check_bar("live", rgb, alpha, ref_rgb, ref_alpha, True)
    check_counts("live", cnt, st, True)
