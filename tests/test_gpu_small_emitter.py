"""The small-emitter path of the scene twins (rt_shade.h emitter_pair, area_sample_point_small, area_light_pdf_small: an emitter of one or two triangles
is sampled from its records in scalar registers, the pdf loop unrolled) and their matte BSDF forms, against the kernels they are the twins of.  The twin
keeps every expression of the less specialised kernels, so the bar is equality of bits: accumulator, rgb, alpha, sample records and counters of a frame
equal those of the same frame on a scene created under PBRT_HIP_FIXED_SCENE=0 (the fixed-frame kernel), with PBRT_HIP_FIXED_FRAME=0 (the generic
kernel) and by the counting twin; last_stats() says the twin for one light and an all-matte table ran.  The less specialised kernels are the yardstick
(tests/test_gpu_parity.py and the per-sample checks pin them to the reference); tests/test_gpu_fixed_scene.py holds the Cornell quad and a one-triangle
emitter to the same bar.
The frame is that of tests/test_gpu_fixed_scene.py: the Cornell box with a 3000-triangle soup, 70 x 45 pixels at 2 x 2 samples, the emitter in view.
The emitters, all in the ceiling's plane and facing down:
  unequal    a quad split 20 : 1 -- the large triangle first, so ShapeSet::Sample's `ls < cdf0` takes both sides within one wave
  overlap    two coplanar triangles that share an edge and overlap: most pdf rays hit both, "the last one hit wins" and its thit decide the film
  reversed   the Cornell quad wound the other way under ReverseOrientation: Triangle::Sample's normal is flipped back down
  three      three triangles: the twin's loops, beside the new branch"""
import numpy as np
import pytest

from gpu_checks import COUNTER_KEYS, need_gpu

SOUP = 3000
BASE = dict(soup_tris=SOUP, xres=70, yres=45, xsamples=2, ysamples=2, jitter=True, pixel_filter="box")
BOTH = 3                                          # RtRenderStats::fixed_scene: one light | no specular lobe

ALL = '"string strategy" ["all"]'
ONE = '"string strategy" ["one"]'


def _emitter(indices, points, before=""):
    return ('AttributeBegin\n  AreaLightSource "area" "color L" [17 12 4] "integer nsamples" [1]\n  Material "matte" "color Kd" [0 0 0]\n%s'
            '  Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\nAttributeEnd\n' % (before, indices, points))


QUAD = "343 548.7 227 343 548.7 332 213 548.7 332 213 548.7 227"
EMITTERS = {
    # areas 6825 and 341.25: the cdf of the first triangle is 20 / 21
    "unequal": _emitter("0 1 2 0 2 3", "343 548.7 227 343 548.7 332 213 548.7 332 336.5 548.7 227"),
    "overlap": _emitter("0 1 2 0 1 3", QUAD),
    "reversed": _emitter("0 2 1 0 3 2", QUAD, before="  ReverseOrientation\n"),
    "three": _emitter("0 1 2 0 2 3 0 3 4", QUAD + " 213 548.7 200"),
}
INTEGRATORS = {
    "direct_all": dict(integrator="directlighting", integrator_params=ALL, maxdepth=5),
    "direct_one": dict(integrator="directlighting", integrator_params=ONE, maxdepth=5),
    "path5": dict(integrator="path", maxdepth=5),
}
CASES = [(e, i, "kdtree") for e in EMITTERS for i in INTEGRATORS] + [("unequal", i, "grid") for i in INTEGRATORS]


def _frame(ds):
    """one frame into a cleared film: (5-plane accumulator, rgb, alpha, sample records, counters, stats of the last launch)"""
    ds.reset_counters(); ds.clear_film()
    ds.render()
    rgb, alpha = ds.film()
    return ds.film_accum(), rgb, alpha, ds.samples(), ds.counters(), ds.last_stats()


def _frame_without_scene_twin(pkg, ps):
    """the frame on a scene of its own, created (and rendered) with PBRT_HIP_FIXED_SCENE=0"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PBRT_HIP_PIPELINE", "0")
        mp.setenv("PBRT_HIP_FIXED_SCENE", "0")
        ds = pkg.DeviceScene(ps)
        try:
            ds.bind_film()
            ds.set_counting(False)
            return _frame(ds)
        finally:
            ds.close()


def _assert_same(name, a, b):
    for what, x, y in zip(("accum", "rgb", "alpha", "samples"), a[:4], b[:4]):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, what, float(np.abs(x - y).max()))
    assert [a[4][k] for k in COUNTER_KEYS] == [b[4][k] for k in COUNTER_KEYS], (name, a[4], b[4])


@pytest.mark.gpu
@pytest.mark.parametrize("emitter,integ,accel", CASES)
def test_small_emitter_twin_equals_less_specialised_kernels(pkg, scenes, emitter, integ, accel):
    need_gpu(pkg)
    name = "%s / %s / %s" % (emitter, integ, accel)
    kw = dict(BASE, accelerator=accel, world_kwargs=dict(area_light=False, extra=EMITTERS[emitter]), **INTEGRATORS[integ])
    ps = pkg.ParsedScene(text=scenes.cornell_scene(**kw))
    assert ps.valid and ps.errors == 0 and ps.spp == 4
    assert ps.n_camera_samples % 64 != 0, name
    ds = pkg.DeviceScene(ps)
    try:
        ds.bind_film()
        ds.set_counting(False)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PBRT_HIP_PIPELINE", "0")
            twin = _frame(ds)
            assert twin[5]["pipeline"] == 0 and twin[5]["fixed_frame"] == 1 and twin[5]["fixed_scene"] == BOTH, (name, "the scene twin did not run", twin[5])
            mp.setenv("PBRT_HIP_FIXED_FRAME", "0")
            generic = _frame(ds)
            assert generic[5]["pipeline"] == 0 and generic[5]["fixed_frame"] == 0 and generic[5]["fixed_scene"] == 0, (name, generic[5])
        frame_only = _frame_without_scene_twin(pkg, ps)
        assert frame_only[5]["fixed_frame"] == 1 and frame_only[5]["fixed_scene"] == 0, (name, frame_only[5])
        assert np.isfinite(twin[0]).all() and twin[1].any() and twin[2].any(), name
        # the emitter lights the box: a frame that is black but for the emitter itself would compare nothing
        assert (twin[1].sum(axis=2) > 0).mean() > 0.5, (name, "most of the frame is black")
        _assert_same(name + " (against the fixed-frame kernel)", twin, frame_only)
        _assert_same(name + " (against the generic kernel)", twin, generic)
        ds.set_counting(True)
        counted = _frame(ds)
        assert counted[5]["fixed_frame"] == 0 and counted[5]["fixed_scene"] == 0, name
        assert counted[4]["camera_rays"] == ps.n_camera_samples and counted[4]["bad_samples"] == 0, (name, counted[4])
        for k in range(4):
            assert np.array_equal(counted[k], twin[k]), (name, "counting twin", k)
    finally:
        ds.close(); ps.close()
