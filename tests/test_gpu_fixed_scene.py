"""The scene twins of the fixed-frame kernels (rt_fixed_frame.h fixed::Scene, rt_mega_fs{d,p}.hip: compiled for a scene with one light and, a second axis,
for a material table without a specular lobe) against the kernels they are the twins of.  A scene twin keeps the expressions the less specialised kernel
runs for such a scene, so the bar is equality of bits: accumulator, rgb, alpha, sample records and counters of a frame equal those of the same frame
rendered on a scene created under PBRT_HIP_FIXED_SCENE=0 (the fixed-frame kernel; the knob is a fact of the scene, read when it is created), with
PBRT_HIP_FIXED_FRAME=0 (the generic kernel) and by the counting twin, and last_stats()["fixed_scene"] / ["fixed_frame"] say which kernel ran.  Scenes
with one disqualifier each must run the less specialised kernel.
The frame is that of tests/test_gpu_fixed_frame.py: the Cornell box with a 3000-triangle soup, 70 x 45 pixels at 2 x 2 samples -- clipped work blocks on
both edges, a short last chunk, pixel 0 inside the frame -- and the ceiling light in view, so camera rays hit the emitter."""
import numpy as np
import pytest

from gpu_checks import COUNTER_KEYS, need_gpu

SOUP = 3000
BASE = dict(soup_tris=SOUP, xres=70, yres=45, xsamples=2, ysamples=2, jitter=True, pixel_filter="box")
ONE_LIGHT, NO_SPECULAR = 1, 2                     # the bits of RtRenderStats::fixed_scene
BOTH = ONE_LIGHT | NO_SPECULAR

ALL = '"string strategy" ["all"]'
ONE = '"string strategy" ["one"]'
# an emitter of ONE triangle (ShapeSet::Sample draws no random number for it), facing down from the ceiling
ONE_TRI_EMITTER = ('AttributeBegin\n  AreaLightSource "area" "color L" [17 12 4] "integer nsamples" [1]\n  Material "matte" "color Kd" [0 0 0]\n'
                   '  Shape "trianglemesh" "integer indices" [0 1 2] "point P" [343 548.7 227 343 548.7 332 213 548.7 332]\nAttributeEnd\n')
PLASTIC = ('AttributeBegin\n  Material "plastic" "color Kd" [.4 .4 .5] "color Ks" [.3 .3 .3] "float roughness" [.1]\n'
           '  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [150 1 150 400 1 150 400 1 400 150 1 400]\nAttributeEnd\n')

# name -> (scene keywords, the axes of the twin that must run).  The Cornell light is an emitter of two triangles: ShapeSet::Sample draws for it.
VARIANTS = {
    "direct_all_d0": (dict(integrator="directlighting", integrator_params=ALL, maxdepth=0), BOTH),
    "direct_all_d5": (dict(integrator="directlighting", integrator_params=ALL, maxdepth=5), BOTH),
    "direct_one_d0": (dict(integrator="directlighting", integrator_params=ONE, maxdepth=0), BOTH),
    "direct_one_d5": (dict(integrator="directlighting", integrator_params=ONE, maxdepth=5), BOTH),
    "path5": (dict(integrator="path", maxdepth=5), BOTH),                  # RandomFloat() draws beyond depth 3: a wrong counter shows
    "direct_all_one_tri": (dict(integrator="directlighting", integrator_params=ALL, maxdepth=5, world_kwargs=dict(area_light=False, extra=ONE_TRI_EMITTER)), BOTH),
    "path5_one_tri": (dict(integrator="path", maxdepth=5, world_kwargs=dict(area_light=False, extra=ONE_TRI_EMITTER)), BOTH),
    "direct_all_point": (dict(integrator="directlighting", integrator_params=ALL, maxdepth=5, world_kwargs=dict(point_light=True, area_light=False)), BOTH),
    "direct_one_point": (dict(integrator="directlighting", integrator_params=ONE, maxdepth=5, world_kwargs=dict(point_light=True, area_light=False)), BOTH),
    "path5_point": (dict(integrator="path", maxdepth=5, world_kwargs=dict(point_light=True, area_light=False)), BOTH),
    # glass and mirror in the soup: one light holds, "no specular lobe" does not, and the specular recursion must still be right
    "direct_all_d5_materials": (dict(integrator="directlighting", integrator_params=ALL, maxdepth=5, soup_materials=True), ONE_LIGHT),
    "direct_one_d5_materials": (dict(integrator="directlighting", integrator_params=ONE, maxdepth=5, soup_materials=True), ONE_LIGHT),
    "path5_materials": (dict(integrator="path", maxdepth=5, soup_materials=True), ONE_LIGHT),
}
CASES = [(v, a) for v in ("direct_all_d0", "direct_all_d5", "direct_one_d0", "direct_one_d5", "path5", "direct_all_d5_materials", "path5_materials") for a in ("kdtree", "grid")] + \
        [(v, "kdtree") for v in ("direct_all_one_tri", "path5_one_tri", "direct_all_point", "direct_one_point", "path5_point", "direct_one_d5_materials")]

DIRECT = dict(integrator="directlighting", integrator_params=ALL, maxdepth=5)
# one disqualifier each -> (scene keywords, fixed_scene that must be reported, fixed_frame that must be reported)
REFUSED = {
    "two_lights": (dict(DIRECT, world_kwargs=dict(point_light=True)), 0, 1),
    "two_lights_path": (dict(integrator="path", maxdepth=5, world_kwargs=dict(point_light=True)), 0, 1),
    "mirror": (dict(DIRECT, world_kwargs=dict(mirror_quad=True)), ONE_LIGHT, 1),
    "glass_blob": (dict(DIRECT, glass_blob=True), ONE_LIGHT, 1),
    "glass_blob_path": (dict(integrator="path", maxdepth=5, glass_blob=True), ONE_LIGHT, 1),
    "whitted": (dict(integrator="whitted", maxdepth=5), 0, 1),
    "ext": (dict(DIRECT, world_kwargs=dict(extra=PLASTIC)), 0, 0),
    "counting": (dict(DIRECT, counting=True), 0, 0),
    "medium": (dict(DIRECT, volume_integrator='"emission" "float stepsize" [40]', world_kwargs=dict(volume='"color Le" [.002 .001 .001]'), env=dict(PBRT_HIP_PIPELINE="0")), 0, 0),
}


def _text(scenes, kw):
    kw = dict(BASE, **kw)
    for k in ("counting", "env"):
        kw.pop(k, None)
    if kw.pop("glass_blob", False):
        kw["world_kwargs"] = dict(kw.get("world_kwargs", {}), glass_sphere_tris=scenes.icosphere((185, 165, 169), 80.0, 1))
    return scenes.cornell_scene(**kw)


def _frame(ds):
    """one frame into a cleared film: (5-plane accumulator, rgb, alpha, sample records, counters, stats of the last launch)"""
    ds.reset_counters(); ds.clear_film()
    ds.render()
    rgb, alpha = ds.film()
    return ds.film_accum(), rgb, alpha, ds.samples(), ds.counters(), ds.last_stats()


def _frame_on_new_scene(pkg, ps, knob, counting=False, env=None):
    """the frame on a scene of its own, created (and rendered) with PBRT_HIP_FIXED_SCENE=knob"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PBRT_HIP_PIPELINE", "0")
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        mp.setenv("PBRT_HIP_FIXED_SCENE", knob)
        ds = pkg.DeviceScene(ps)
        try:
            ds.bind_film()
            ds.set_counting(counting)
            return _frame(ds)
        finally:
            ds.close()


def _assert_same(name, a, b):
    for what, x, y in zip(("accum", "rgb", "alpha", "samples"), a[:4], b[:4]):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, what, float(np.abs(x - y).max()))
    assert [a[4][k] for k in COUNTER_KEYS] == [b[4][k] for k in COUNTER_KEYS], (name, a[4], b[4])


def test_stats_report_the_scene_axes(pkg):
    fields = [n for n, _ in pkg.RtRenderStats._fields_]
    assert fields[-2:] == ["fixed_frame", "fixed_scene"]                      # appended: fixed_frame stays where it was
    assert "rt_mega_fsd.hip" in pkg.HIP_UNITS and "rt_mega_fsp.hip" in pkg.HIP_UNITS


@pytest.mark.gpu
@pytest.mark.parametrize("variant,accel", CASES)
def test_scene_twin_equals_less_specialised_kernels(pkg, scenes, variant, accel):
    need_gpu(pkg)
    name = "%s / %s" % (variant, accel)
    kw, axes = VARIANTS[variant]
    ps = pkg.ParsedScene(text=_text(scenes, dict(kw, accelerator=accel)))
    assert ps.valid and ps.errors == 0 and ps.spp == 4
    assert ps.n_camera_samples % 64 != 0 and ps.sample_extent[0] <= 0 and ps.sample_extent[2] <= 0, name
    ds = pkg.DeviceScene(ps)
    try:
        ds.bind_film()
        ds.set_counting(False)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PBRT_HIP_PIPELINE", "0")
            twin = _frame(ds)
            assert twin[5]["pipeline"] == 0 and twin[5]["fixed_frame"] == 1 and twin[5]["fixed_scene"] == axes, (name, "the scene twin did not run", twin[5])
            mp.setenv("PBRT_HIP_FIXED_SCENE", "0")            # (read at scene create: it changes nothing on a scene that exists)
            again = _frame(ds)                                # ... a second frame on the same scene
            assert again[5]["fixed_frame"] == 1 and again[5]["fixed_scene"] == axes, (name, again[5])
            mp.delenv("PBRT_HIP_FIXED_SCENE")
            mp.setenv("PBRT_HIP_FIXED_FRAME", "0")
            generic = _frame(ds)
            assert generic[5]["pipeline"] == 0 and generic[5]["fixed_frame"] == 0 and generic[5]["fixed_scene"] == 0, (name, generic[5])
        frame_only = _frame_on_new_scene(pkg, ps, "0")
        assert frame_only[5]["fixed_frame"] == 1 and frame_only[5]["fixed_scene"] == 0, (name, frame_only[5])
        allowed = _frame_on_new_scene(pkg, ps, "1")           # (the knob only allows the twin)
        assert allowed[5]["fixed_frame"] == 1 and allowed[5]["fixed_scene"] == axes, (name, allowed[5])
        assert np.isfinite(twin[0]).all() and twin[1].any() and twin[2].any(), name
        _assert_same(name + " (against the fixed-frame kernel)", twin, frame_only)
        _assert_same(name + " (a scene created with the knob at 1)", allowed, twin)
        _assert_same(name + " (against the generic kernel)", twin, generic)
        _assert_same(name + " (second frame)", again, twin)
        # ... and the counting twin, which no frame takes a specialised kernel for, draws the same film and counts its rays
        ds.set_counting(True)
        counted = _frame(ds)
        assert counted[5]["fixed_frame"] == 0 and counted[5]["fixed_scene"] == 0, name
        assert counted[4]["camera_rays"] == ps.n_camera_samples and counted[4]["bad_samples"] == 0, (name, counted[4])
        for k in range(4):
            assert np.array_equal(counted[k], twin[k]), (name, "counting twin", k)
    finally:
        ds.close(); ps.close()


@pytest.mark.gpu
@pytest.mark.parametrize("why", sorted(REFUSED))
def test_disqualified_scene_runs_less_specialised_kernel(pkg, scenes, why):
    need_gpu(pkg)
    kw, want_scene, want_frame = REFUSED[why]
    ps = pkg.ParsedScene(text=_text(scenes, kw))
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    try:
        ds.bind_film()
        ds.set_counting(bool(kw.get("counting", False)))
        with pytest.MonkeyPatch.context() as mp:
            for k, v in kw.get("env", {}).items():
                mp.setenv(k, v)
            free = _frame(ds)
            assert free[5]["fixed_scene"] == want_scene and free[5]["fixed_frame"] == want_frame, (why, "a disqualified scene ran a twin it must not", free[5])
            mp.setenv("PBRT_HIP_FIXED_FRAME", "0")
            generic = _frame(ds)
            assert generic[5]["fixed_scene"] == 0 and generic[5]["fixed_frame"] == 0, (why, generic[5])
        counting, env = bool(kw.get("counting", False)), kw.get("env", {})
        held = _frame_on_new_scene(pkg, ps, "0", counting, env)
        assert held[5]["fixed_scene"] == 0 and held[5]["fixed_frame"] == want_frame, (why, held[5])
        for value in ("1", "3"):
            asked = _frame_on_new_scene(pkg, ps, value, counting, env)
            assert asked[5]["fixed_scene"] == want_scene and asked[5]["fixed_frame"] == want_frame, (why, "the knob forced a twin onto a disqualified scene", asked[5])
            _assert_same(why + " (knob at %s)" % value, asked, held)
        assert np.isfinite(free[0]).all() and free[1].any(), why
        _assert_same(why, free, held)
        _assert_same(why + " (against the generic kernel)", free, generic)
    finally:
        ds.close(); ps.close()
