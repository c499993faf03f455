"""rt_last_render_stats speaks of the last timed launch and of nothing before it (include/pbrt_hip.h: weighted_points / weighted_ms are "zeros otherwise",
iterations is 0 for one kernel).  rt_trace_closest is a timed launch of one trace kernel: after it the stats hold that kernel's time and no field of the
frame that ran before -- a "weighted" frame's shading points and pass times, the queue pipeline's iterations and slots, the fixed-frame flags.
Scene: the keyed Cornell box with a point light, 16 x 16 pixels of one sample; the fixed-frame case adds the 3000-triangle soup and the settings
tests/test_gpu_fixed_frame.py qualifies with.  (That a radiance query, which is not a timed launch, leaves the stats alone: tests/test_gpu_radiance.py.)"""
import pytest

from gpu_checks import PIPELINE_ENVS, need_gpu

BASE = dict(xres=16, yres=16, xsamples=1, ysamples=1, keyed=True, world_kwargs=dict(point_light=True))
# scene options, the frame's knobs, whether the scene counts, and what the frame's own stats must say (so that no case passes vacuously)
FRAMES = {
    "weighted": (dict(integrator="directlighting", integrator_params='"string strategy" ["weighted"]'), {}, True,
                 lambda st: st["weighted_points"] > 0 and st["pipeline"] == 0),
    "pipeline": (dict(integrator="path"), PIPELINE_ENVS[0], True,
                 lambda st: st["pipeline"] == 1 and st["iterations"] > 0 and st["slots"] > 0),
    "fixed_frame": (dict(integrator="directlighting", integrator_params='"string strategy" ["all"]', soup_tris=3000, jitter=True, pixel_filter="box"),
                    dict(PBRT_HIP_PIPELINE="0"), False,
                    lambda st: st["fixed_frame"] == 1 and st["pipeline"] == 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_a_trace_call_leaves_nothing_of_the_frame_before_it_in_the_stats(pkg, scenes, frame):
    need_gpu(pkg)
    opts, env, counting, ran = FRAMES[frame]
    ps = pkg.ParsedScene(text=scenes.cornell_scene(**dict(BASE, **opts)))
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    try:
        ds.set_counting(counting)
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            ds.render()
        before = ds.last_stats()
        assert ran(before), (frame, before)
        assert ds.last_stats() == before, frame
        assert len(ds.trace_closest(ds.camera_rays(0, 64))) == 64
        st = ds.last_stats()
        assert st["weighted_points"] == 0 and st["weighted_ms"] == [0.0] * 5, (frame, st)
        assert st["pipeline"] == 0 and st["iterations"] == 0 and st["timed_iterations"] == 0 and st["slots"] == 0, (frame, st)
        assert st["fixed_frame"] == 0 and st["fixed_scene"] == 0, (frame, st)
        assert st["trace_ms"] == st["render_ms"], (frame, st)
        assert ds.last_stats() == st, frame
    finally:
        ds.close()
