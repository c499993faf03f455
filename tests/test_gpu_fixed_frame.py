"""The kernels compiled for a fixed frame (rt_fixed_frame.h, rt_mega_f.hip: stratified sampler with n == 1 requests, pinhole perspective / orthographic
camera, one shard handed out in pixel blocks) against the generic kernels they are the twins of.  The fixed kernel keeps the expressions the generic one
runs for such a frame, so the bar is equality of bits: film, alpha, sample records and counters of a frame equal those of the same frame rendered with
PBRT_HIP_FIXED_FRAME=0, and last_stats()["fixed_frame"] says which family ran.  Frames with one disqualifier each must run the generic kernel.
Scene: the Cornell box with a 3000-triangle soup (large enough for the high-occupancy kernels), 70 x 45 pixels at 2 x 2 samples: neither side is a
multiple of the 32-pixel work block, so clipped blocks run on both edges; 64 does not divide the 72 x 47 x 4 samples, so the last chunk is short; pixel 0,
whose strata come from the sampler constructor's stream, is inside the frame."""
import numpy as np
import pytest

from gpu_checks import COUNTER_KEYS, need_gpu

SOUP = 3000
BASE = dict(soup_tris=SOUP, xres=70, yres=45, xsamples=2, ysamples=2, jitter=True, pixel_filter="box")
ORTHO = 'Camera "orthographic" "float screenwindow" [-300 300 -200 200]'
ENVCAM = 'Camera "environment"'
PLASTIC = ('AttributeBegin\n  Material "plastic" "color Kd" [.4 .4 .5] "color Ks" [.3 .3 .3] "float roughness" [.1]\n'
           '  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [150 1 150 400 1 150 400 1 400 150 1 400]\nAttributeEnd\n')

VARIANTS = {
    "direct_all": dict(integrator="directlighting", integrator_params='"string strategy" ["all"]'),
    "direct_one": dict(integrator="directlighting", integrator_params='"string strategy" ["one"]'),
    "whitted": dict(integrator="whitted", soup_materials=True, world_kwargs=dict(point_light=True)),
    "path5": dict(integrator="path", maxdepth=5, soup_materials=True),
    "direct_all_unjittered": dict(integrator="directlighting", integrator_params='"string strategy" ["all"]', jitter=False),
    "direct_all_ortho": dict(integrator="directlighting", integrator_params='"string strategy" ["all"]', camera=ORTHO),
}
CASES = [(v, a) for v in ("direct_all", "direct_one", "whitted", "path5") for a in ("kdtree", "grid")] + \
        [("direct_all_unjittered", "kdtree"), ("direct_all_ortho", "kdtree")]

DIRECT = dict(integrator="directlighting", integrator_params='"string strategy" ["all"]')
# one disqualifier each; env: knobs of the frame, shard / counting: how it is rendered
REFUSED = {
    "lowdiscrepancy": dict(DIRECT, sampler="lowdiscrepancy", pixelsamples=4),
    "random": dict(DIRECT, sampler="random"),
    "light_nsamples_4": dict(DIRECT, world_kwargs=dict(light_nsamples=4)),
    "lens": dict(DIRECT, lensradius=4.0, focaldistance=900.0),
    "environment_camera": dict(DIRECT, camera=ENVCAM),
    "two_shards": dict(DIRECT, shards=2),
    "counting": dict(DIRECT, counting=True),
    "ext": dict(DIRECT, world_kwargs=dict(extra=PLASTIC)),
    "medium": dict(DIRECT, volume_integrator='"emission" "float stepsize" [40]', world_kwargs=dict(volume='"color Le" [.002 .001 .001]'), env=dict(PBRT_HIP_PIPELINE="0")),
    "tiny_scene": dict(DIRECT, soup_tris=0),
}


def _text(scenes, kw):
    kw = dict(BASE, **kw)
    camera = kw.pop("camera", None)
    for k in ("shards", "counting", "env"):
        kw.pop(k, None)
    text = scenes.cornell_scene(**kw)
    if camera is not None:
        head, sep, rest = text.partition('Camera "perspective"')
        assert sep
        text = head + camera + rest[rest.index("\n"):]
    return text


def _frame(ds, ps, shards=1):
    """one frame into a cleared film: (5-plane accumulator, rgb, alpha, sample records, counters, stats of the last launch)"""
    ds.reset_counters(); ds.clear_film()
    try:
        for shard in range(shards):
            if shards > 1:
                ps.set_shard(shard, shards, (8, 8))
            ds.render()
    finally:
        if shards > 1:
            ps.set_shard(0, 1, 64)
    rgb, alpha = ds.film()
    return ds.film_accum(), rgb, alpha, ds.samples() if shards == 1 else None, ds.counters(), ds.last_stats()


def _assert_same(name, a, b):
    for what, x, y in zip(("accum", "rgb", "alpha", "samples"), a[:4], b[:4]):
        if x is None:
            continue
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, what, float(np.abs(x - y).max()))
    assert [a[4][k] for k in COUNTER_KEYS] == [b[4][k] for k in COUNTER_KEYS], (name, a[4], b[4])


@pytest.mark.gpu
@pytest.mark.parametrize("variant,accel", CASES)
def test_fixed_kernel_equals_generic(pkg, scenes, variant, accel):
    need_gpu(pkg)
    name = "%s / %s" % (variant, accel)
    ps = pkg.ParsedScene(text=_text(scenes, dict(VARIANTS[variant], accelerator=accel)))
    assert ps.valid and ps.errors == 0 and ps.spp == 4
    assert ps.n_camera_samples % 64 != 0 and ps.sample_extent[0] <= 0 and ps.sample_extent[2] <= 0, name
    ds = pkg.DeviceScene(ps)
    try:
        ds.bind_film()
        ds.set_counting(False)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PBRT_HIP_PIPELINE", "0")
            fixed = _frame(ds, ps)
            assert fixed[5]["pipeline"] == 0 and fixed[5]["fixed_frame"] == 1, (name, "the fixed kernel did not run", fixed[5])
            mp.setenv("PBRT_HIP_FIXED_FRAME", "0")
            generic = _frame(ds, ps)
            assert generic[5]["pipeline"] == 0 and generic[5]["fixed_frame"] == 0, (name, generic[5])
            mp.setenv("PBRT_HIP_FIXED_FRAME", "1")            # (the knob cannot force the fixed kernel onto a frame: it only allows it)
            again = _frame(ds, ps)
            assert again[5]["fixed_frame"] == 1, (name, again[5])
        assert np.isfinite(fixed[0]).all() and fixed[1].any() and fixed[2].any(), name
        _assert_same(name, fixed, generic)
        _assert_same(name + " (second frame)", again, generic)
        # ... and the counting twin, which no frame takes the fixed kernel for, draws the same film and counts its rays
        ds.set_counting(True)
        counted = _frame(ds, ps)
        assert counted[5]["fixed_frame"] == 0, name
        assert counted[4]["camera_rays"] == ps.n_camera_samples and counted[4]["bad_samples"] == 0, (name, counted[4])
        for k in range(4):
            assert np.array_equal(counted[k], fixed[k]), (name, "counting twin", k)
    finally:
        ds.close(); ps.close()


@pytest.mark.gpu
@pytest.mark.parametrize("why", sorted(REFUSED))
def test_disqualified_frame_runs_generic_kernel(pkg, scenes, why):
    need_gpu(pkg)
    kw = REFUSED[why]
    ps = pkg.ParsedScene(text=_text(scenes, kw))
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    try:
        ds.bind_film()
        ds.set_counting(bool(kw.get("counting", False)))
        with pytest.MonkeyPatch.context() as mp:
            for k, v in kw.get("env", {}).items():
                mp.setenv(k, v)
            free = _frame(ds, ps, kw.get("shards", 1))
            assert free[5]["fixed_frame"] == 0, (why, "a disqualified frame ran the fixed kernel", free[5])
            mp.setenv("PBRT_HIP_FIXED_FRAME", "0")
            held = _frame(ds, ps, kw.get("shards", 1))
            assert held[5]["fixed_frame"] == 0, (why, held[5])
            mp.setenv("PBRT_HIP_FIXED_FRAME", "1")
            asked = _frame(ds, ps, kw.get("shards", 1))
            assert asked[5]["fixed_frame"] == 0, (why, "the knob forced the fixed kernel onto a disqualified frame", asked[5])
        assert np.isfinite(free[0]).all() and free[1].any(), why
        _assert_same(why, free, held)
        _assert_same(why + " (knob at 1)", asked, held)
    finally:
        ds.close(); ps.close()
