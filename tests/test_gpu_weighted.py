"""DirectLighting with strategy "weighted": WeightedSampleOneLight (transport.cpp:71-122) on the device (pbrt-v1_amd/csrc/hip/rt_weighted.h).

The strategy is a recurrence over EVERY shading point of the frame in program order, so one wrong estimate anywhere changes the light choices of the
rest of the frame.  The five reference films tests/golden/weighted_*.npz (1, 2, 3, 4 and 6 lights; delta, quadric and two-triangle emitters; glass and
mirror recursion; stratified and low-discrepancy samplers) are covered by test_gpu_parity.py::test_device_film_matches_reference_golden.  Here:
larger seeded frames against the oracle (whose "weighted" is pinned by those five films, tests/test_oracle_golden.py), the timed kernels against
their counting twins, both forms of the recurrence kernel (40 lights in lanes, 70 in LDS tables), a medium, the grid, the frames the device refuses."""
import numpy as np
import pytest
from gpu_checks import need_gpu
from test_gpu_parity import check_film

pytestmark = pytest.mark.gpu

SPOT = 'LightSource "spot" "point from" [278 540 100] "point to" [200 0 330] "color I" [600000 500000 400000] "float coneangle" [35] "float conedeltaangle" [12]\n'
DISTANT = 'LightSource "distant" "point from" [0.3 1 -0.8] "point to" [0 0 0] "color L" [1.5 1.6 2.0]\n'
EMITTER2 = ('AttributeBegin\nAreaLightSource "area" "color L" [3 6 12]\nMaterial "matte" "color Kd" [0 0 0]\n'
            'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [20 150 100  20 150 300  20 350 300  20 350 100]\nAttributeEnd\n')
W = '"string strategy" ["weighted"]'


def many_points(n, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        p = rng.uniform((40, 60, 40), (510, 520, 500)); c = rng.uniform(20000, 160000, 3)
        out.append('LightSource "point" "point from" [%.1f %.1f %.1f] "color I" [%.0f %.0f %.0f]\n' % (*p, *c))
    return "".join(out)


CASES = {
    "delta3_soup_materials": dict(xres=96, yres=96, xsamples=2, ysamples=2, jitter=True, soup_tris=3000, soup_materials=True,
                                  world_kwargs=dict(point_light=True, area_light=False, extra=SPOT + DISTANT, mirror_quad=True)),
    "two_mesh_emitters_soup": dict(xres=128, yres=96, xsamples=2, ysamples=1, jitter=True, soup_tris=20000, pixel_filter="mitchell",
                                   world_kwargs=dict(extra=EMITTER2)),
    "forty_points_ld": dict(xres=64, yres=64, sampler="lowdiscrepancy", pixelsamples=4, soup_tris=500, soup_materials=True,
                            world_kwargs=dict(area_light=False, extra=many_points(40))),
    "seventy_points": dict(xres=48, yres=48, xsamples=2, ysamples=1, jitter=True, soup_tris=300, soup_materials=True,              # > 64 lights: the recurrence's LDS form
                           world_kwargs=dict(area_light=False, extra=many_points(70, 11))),
    "delta4_soup200k_256": dict(xres=256, yres=256, xsamples=2, ysamples=2, jitter=True, soup_tris=200000, soup_materials=True,      # 0.4 M shading points: many LDS chunks, every scan block
                                world_kwargs=dict(point_light=True, area_light=False, extra=SPOT + DISTANT + many_points(1, 2))),
    "grid_four_lights": dict(xres=64, yres=64, xsamples=2, ysamples=1, accelerator="grid", soup_tris=2000,
                             world_kwargs=dict(point_light=True, area_light=False, extra=SPOT + DISTANT + many_points(1, 9), mirror_quad=True)),
    # lights of mixed RNG use (round 5): the two-triangle ceiling emitter draws its triangle, the point / spot / distant lights draw nothing; mirror and
    # soup glass give samples of several shading points, so the emitter's draw sits at k = 0 .. j draws further depending on the lights chosen before
    "mixed_emitter_and_deltas": dict(xres=72, yres=72, xsamples=2, ysamples=2, jitter=True, soup_tris=2500, soup_materials=True, maxdepth=4,
                                     world_kwargs=dict(point_light=True, extra=SPOT + DISTANT, mirror_quad=True)),
    "mixed_two_emitters_ld": dict(xres=64, yres=48, sampler="lowdiscrepancy", pixelsamples=4, soup_tris=1500, soup_materials=True, maxdepth=5,
                                  world_kwargs=dict(point_light=True, extra=EMITTER2 + many_points(2, 17), mirror_quad=True)),
    "medium_two_points": dict(xres=32, yres=32, xsamples=2, ysamples=1, jitter=True, volume_integrator='"single" "float stepsize" [80]',
                              world_kwargs=dict(volume='"float g" [.3]', point_light=True, area_light=False, extra=many_points(1, 3), mirror_quad=True)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_weighted_frame_matches_the_oracle(pkg, scenes, oracle, case):
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(keyed=True, integrator="directlighting", integrator_params=W, **CASES[case]))
    assert ps.valid and ps.render_view()["strategy"] == 2
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film(); acc = ds.film_accum(); cnt = ds.counters(); st = ds.last_stats()
    nodes, refs = ds.accel_arrays(); info = ds.accel_info(); bounds = np.array(list(info.bounds), np.float32)
    orgb, oalpha, _, ocnt = oracle.render(ps, nodes, refs, bounds, info=info)
    check_film("weighted:" + case, rgb, alpha, orgb, oalpha, ps.integrator)
    # Scene::Render's rays only: the count and survey passes are not counted.  With an emitter in the scene the BSDF-sampled MIS ray's direction goes
    # through the device's sinf / cosf (ConcentricSampleDisk): a last-bit difference from glibc moves a handful of node visits per frame under ANY
    # strategy (this frame: 5 of 2.7 M with "one", 8 of 3.9 M with "all") and the last bit of some estimates -- which "weighted" feeds into its
    # recurrence: the weights then differ in the last bits too (per pixel <= 5e-7 here), and a light choice flips only if a sample falls within that
    # of a CDF step.
    emitters = ps.n_light_tris > 0
    for k in ("camera_rays", "closest_rays", "any_rays", "nodes_visited", "leaf_refs", "tri_tests"):
        slack = 16 if emitters and k in ("nodes_visited", "leaf_refs", "tri_tests") else 0
        assert abs(cnt[k] - ocnt[k]) <= slack, (k, cnt[k], ocnt[k])
    assert st["pipeline"] == 0 and st["weighted_points"] > 0.5 * cnt["camera_rays"] and all(m > 0 for m in st["weighted_ms"])
    # the same frame again, and from the timed kernels: bit-identical (the recurrence is deterministic, and so is everything around it)
    ds.clear_film(); ds.reset_counters(); ds.render()
    assert np.array_equal(ds.film_accum(), acc) and ds.counters() == cnt
    ds.set_counting(False); ds.clear_film(); ds.render()
    assert np.array_equal(ds.film_accum(), acc), "the timed weighted kernels differ from their counting twins"
    assert ds.last_stats()["weighted_points"] == st["weighted_points"]
    ds.close()


def test_weighted_against_the_live_reference_when_present(pkg, scenes):
    """The compiled reference travels to the GPU box (oracle/_ref): one "weighted" frame that is in no fixture, rendered by both, live -- the device
    against the reference itself, the oracle not in the loop.  Delta lights only: every estimate is bit-reproducible, so the recurrences cannot part."""
    need_gpu(pkg)
    import __graft_entry__ as g_entry
    text = scenes.cornell_scene(xres=80, yres=64, xsamples=2, ysamples=2, jitter=True, soup_tris=6000, soup_materials=True, keyed=True, count=True, seed=23,
                                integrator="directlighting", integrator_params=W, maxdepth=4,
                                world_kwargs=dict(point_light=True, area_light=False, extra=SPOT + DISTANT + many_points(2, 31), mirror_quad=True))
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(text, keyed=True)
    except FileNotFoundError:
        pytest.skip("oracle/_ref not on this box")
    rgb, alpha, cnt, _ = pkg.render_text(text)
    check_film("weighted:live", rgb, alpha, ref_rgb, ref_alpha, 1)
    assert cnt["closest_rays"] == st["closest_rays"] and cnt["any_rays"] == st["any_rays"]


def test_weighted_is_the_references_estimator_including_its_scale(pkg, scenes):
    """What the reference computes, not what one might expect of it: SampleStep1d's pdf (mc.cpp:51) is a DENSITY over [0, 1) -- a light is chosen with
    probability pdf / nLights -- and transport.cpp:118 divides the estimate by that density, so a converged "weighted" image is the direct lighting
    divided by nLights (the golden films say the same).  The device reproduces the reference: 1 / 3 of strategy "one" with three lights, block by block."""
    need_gpu(pkg)
    kw = dict(xres=48, yres=48, xsamples=6, ysamples=6, jitter=True, keyed=True, integrator="directlighting",
              world_kwargs=dict(point_light=True, area_light=False, extra=SPOT + DISTANT))
    films = {}
    for strat in ("weighted", "one"):
        rgb, alpha, cnt, _ = pkg.render_text(scenes.cornell_scene(integrator_params='"string strategy" ["%s"]' % strat, **kw))
        films[strat] = rgb
    w3 = 3.0 * films["weighted"]
    assert abs(w3.mean() - films["one"].mean()) < 0.03 * films["one"].mean(), (float(w3.mean()), float(films["one"].mean()))
    blk = lambda a: a.reshape(6, 8, 6, 8, 3).mean((1, 3))
    assert np.abs(blk(w3) - blk(films["one"])).max() < 0.25 * blk(films["one"]).max()


def test_weighted_without_lights_and_with_one(pkg, scenes):
    """No lights: WeightedSampleOneLight is never called (directlighting.cpp:106) -- the film of strategy "one".  One light: the CDF has one
    step, every weight is 1 -- again the film of "one" (nLights * Ld with nLights = 1), whatever the recurrence does."""
    need_gpu(pkg)
    for wk in (dict(area_light=False, mirror_quad=True), dict(mirror_quad=True)):
        kw = dict(xres=32, yres=32, xsamples=2, ysamples=1, jitter=True, keyed=True, integrator="directlighting", world_kwargs=wk)
        a, aa, ca, _ = pkg.render_text(scenes.cornell_scene(integrator_params=W, **kw))
        b, ba, cb, _ = pkg.render_text(scenes.cornell_scene(integrator_params='"string strategy" ["one"]', **kw))
        assert np.array_equal(a, b) and np.array_equal(aa, ba) and ca == cb, wk


def test_frames_the_weighted_recurrence_cannot_serve_are_refused(pkg, scenes):
    need_gpu(pkg)
    kw = dict(xres=16, yres=16, keyed=True, integrator="directlighting", integrator_params=W)
    # (a point light next to the two-triangle ceiling emitter -- lights of mixed RNG use -- was refused until round 5: now CASES["mixed_*"] and the
    # reference film weighted_cornell_plus_point)
    # a participating medium with the two-triangle emitter: Scene::Transmittance draws per unoccluded ray, so the survey and the frame pass
    # would hand ShapeSet::Sample different random numbers at a sample's second shading point (here: behind the mirror)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(volume_integrator='"single" "float stepsize" [60]', world_kwargs=dict(volume='"float g" [0]', mirror_quad=True), **kw))
    assert ps.valid
    ds = pkg.DeviceScene(ps)
    with pytest.raises(pkg.RtError) as e:
        ds.render()
    assert "medium" in str(e.value) and "weighted" in str(e.value)
    ds.close()
    # more than one shard: the recurrence spans the frame
    ps = pkg.ParsedScene(text=scenes.cornell_scene(**kw))
    ps.set_shard(0, 2, 64)
    ds = pkg.DeviceScene(ps)
    with pytest.raises(pkg.RtError) as e:
        ds.render()
    assert "one shard" in str(e.value)
    ds.close()
