"""The checks that the tests/test_gpu_<feature>.py files share: the bars that decide whether a device film and its ray counts agree with the
reference's, and the comparisons of the kernel flavours, of rt_scene_create_prebuilt and of a two-shard split against one
frame.  Written once, so that a bar is tightened in one place; tests/test_gpu_checks_host.py pins the bars without a device.
  strict: every pixel's rgb and alpha within 1e-5, closest_rays / any_rays equal;
  loose:  >= 99.5 % of the pixels with per-pixel L2 < 1e-4 and mean L2 < 1e-4, alpha off by more than 1e-5 on <= 0.5 % of the pixels, each
          ray count within max(4, 2e-4 * n) of its own reference count;
  both:   rgb and alpha finite, camera rays equal (as exactly as StatsPrint wrote them), no bad samples."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, film_metrics, stat_int

COUNTER_KEYS = ("camera_rays", "closest_rays", "any_rays", "nodes_visited", "leaf_refs", "tri_tests", "bad_samples")
# the queue pipeline per ray, by path vertex (where the frame takes that form), and with 512 slots so that every slot is refilled many times
PIPELINE_ENVS = (dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="0"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="1"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_SLOTS="512"))


def need_gpu(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")


def fixture_names(subdir):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, subdir, "*.npz")))


def render_both(pkg, text):
    """counting twin (film + counters), then the timed kernel (film), of one scene text"""
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


def bar_metrics(rgb, alpha, ref_rgb, ref_alpha):
    """film_metrics of the colour, and alpha's largest difference and the share of the pixels where it is off by more than 1e-5"""
    m = film_metrics(rgb, ref_rgb)
    da = np.abs(alpha - ref_alpha)
    m.update(alpha_maxabs=float(da.max()), alpha_off=float((da > 1e-5).mean()))
    return m


def check_bar(name, rgb, alpha, ref_rgb, ref_alpha, loose):
    m = bar_metrics(rgb, alpha, ref_rgb, ref_alpha)
    print(name, "loose" if loose else "strict", m)
    assert np.isfinite(rgb).all() and np.isfinite(alpha).all(), name
    if loose:
        assert m["frac"] >= 0.995 and m["mean_l2"] < 1e-4, (name, m)
        assert m["alpha_off"] <= 0.005, (name, m)
    else:
        assert m["maxabs"] <= 1e-5 and m["alpha_maxabs"] <= 1e-5, (name, m)
    return m


def check_counts(name, cnt, st, loose):
    print(name, "device", cnt["closest_rays"], cnt["any_rays"], "reference", st["closest_rays"], st["any_rays"])
    for k in ("closest_rays", "any_rays"):
        tol = max(4, int(2e-4 * st[k])) if loose else 0
        assert abs(cnt[k] - st[k]) <= tol, (name, k, cnt[k], st[k], tol)
    cam, exact = stat_int(st["stats"]["Camera Rays Traced"])          # StatsPrint writes 17424 as "17.4k": equal where it is exact, else equal as printed
    assert (cnt["camera_rays"] == cam if exact else abs(cnt["camera_rays"] - cam) <= .0005 * cam + 50), (name, cnt["camera_rays"], cam)
    assert cnt["bad_samples"] == 0, name


def differing_share(rgb, ref_rgb):
    """the share of the pixels more than 1e-3 (L2) away from the fixture: what "another film" is measured by"""
    return float((np.sqrt(((rgb.astype(np.float64) - ref_rgb) ** 2).sum(-1)) > 1e-3).mean())


def _same_counters(c, cnt_ref, keys, *what):
    assert [c[k] for k in keys] == [cnt_ref[k] for k in keys], what + (c, cnt_ref)


def _timed_and_counting_agree(ds, ref, cnt_ref, expect_pipeline, *what):
    for counting in (False, True):
        ds.set_counting(counting); ds.reset_counters(); ds.clear_film(); ds.render()
        if expect_pipeline is not None:                     # after each render: last_stats() speaks of the last one only
            assert ds.last_stats()["pipeline"] == expect_pipeline, what + (counting,)
        got = ds.film_accum()
        assert np.array_equal(got, ref), what + (counting, float(np.abs(got - ref).max()))
        if counting:
            _same_counters(ds.counters(), cnt_ref, COUNTER_KEYS, *what)


def assert_flavours_agree(ds, name, pipeline_envs, expect_pipeline=1):
    """On a freshly opened DeviceScene: the megakernel's counting twin gives the film and the counters; the timed kernel and the counting twin
    of both occupancy flavours, and of the queue pipeline under each of pipeline_envs, give the bit-identical film_accum(), the counting runs
    the same counters.  expect_pipeline: what last_stats()["pipeline"] is after every render under a pipeline_envs setting (None: not asserted).
    Returns (film, counters); the environment is as it was."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PBRT_HIP_PIPELINE", "0")
        ds.render()
        assert ds.last_stats()["pipeline"] == 0, name
        ref = ds.film_accum()
        cnt_ref = ds.counters()
        for occ in ("0", "1"):
            mp.setenv("PBRT_HIP_HIGH_OCC", occ)
            _timed_and_counting_agree(ds, ref, cnt_ref, 0, name, "PBRT_HIP_HIGH_OCC=" + occ)
        mp.delenv("PBRT_HIP_HIGH_OCC")
        for env in pipeline_envs:
            with pytest.MonkeyPatch.context() as inner:
                for k, v in env.items():
                    inner.setenv(k, v)
                _timed_and_counting_agree(ds, ref, cnt_ref, expect_pipeline, name, env)
    return ref, cnt_ref


def assert_prebuilt_agrees(pkg, ps, ref, cnt_ref=None):
    """rt_scene_create_prebuilt (the multi-rank path), on the accelerator of an rt_scene_create scene, gives the film ref (and, where given,
    the counters cnt_ref).  Returns the prebuilt scene, open."""
    a = pkg.DeviceScene(ps)
    nodes, refs = a.accel_arrays()
    info = a.accel_info()
    a.close()
    b = pkg.DeviceScene(ps, prebuilt=(nodes, refs, info))
    b.render()
    got = b.film_accum()
    assert np.array_equal(got, ref), ("prebuilt", float(np.abs(got - ref).max()))
    if cnt_ref is not None:
        _same_counters(b.counters(), cnt_ref, COUNTER_KEYS, "prebuilt")
    return b


def assert_two_shards_agree(ps, b, ref, cnt_ref, exact=True):
    """Two shards of 8 x 8-pixel tiles rendered into one film, as the ranks' films are summed, give the film and the ray counts of one frame.
    exact: the box filter gives every sample to the one pixel it lies in, and a tile holds whole pixels, so a pixel's sum is formed by one
    shard; under a wider filter both shards add to a pixel, in another order."""
    b.reset_counters(); b.clear_film()
    try:
        for shard in range(2):
            ps.set_shard(shard, 2, (8, 8))
            b.render()
        parts, cnt = b.film_accum(), b.counters()
    finally:
        ps.set_shard(0, 1, 64)
    if exact:
        assert np.array_equal(parts, ref), ("shards", float(np.abs(parts - ref).max()))
    else:
        assert np.allclose(parts, ref, rtol=2e-5, atol=2e-6), ("shards", float(np.abs(parts - ref).max()))
    _same_counters(cnt, cnt_ref, ("camera_rays", "closest_rays", "any_rays", "bad_samples"), "shards")
