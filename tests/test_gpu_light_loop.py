"""How a lane leaves the direct-lighting loop (rt_integrate.h: UniformSampleAllLights' last estimate performs the loop's exit statements itself,
all_lights_done, instead of going back through ST_DIRECT_NEXT in another pass).  Cornell plus a 3 000-triangle soup of matte, glass and mirror
triangles (the specular recursion re-enters the loop at every level) at 64 x 48 @ 4 spp, under DirectLighting "all" and "one" and under Whitted,
with one, two and three lights (area; + point; + spot) and 1 and 4 samples on the area light.  Per frame the counting twin gives the film and the
ray counts; the timed kernel and the counting twin of both occupancy flavours and of the queue pipeline (whose shade kernel runs the same
advance_pass) give the bit-identical film and the same counts.  tests/golden holds no film of these frames: the reference's films of the loop
(direct_all_ns4_spp4, direct_spot_area, direct_one_point_and_area, ...) are compared by tests/test_gpu_parity.py."""
import numpy as np
import pytest

from gpu_checks import PIPELINE_ENVS, assert_flavours_agree, need_gpu

SPOT = ('LightSource "spot" "point from" [278 540 100] "point to" [200 0 330] "color I" [600000 500000 400000] "float coneangle" [35] '
        '"float conedeltaangle" [12]\n')
LIGHTS = {1: dict(), 2: dict(point_light=True), 3: dict(point_light=True, extra=SPOT)}
INTEGRATORS = {
    "direct_all": dict(integrator="directlighting", integrator_params='"string strategy" ["all"]'),
    "direct_one": dict(integrator="directlighting", integrator_params='"string strategy" ["one"]'),
    "whitted": dict(integrator="whitted"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("integ", sorted(INTEGRATORS))
def test_light_loop_exit_keeps_every_flavour_bit_identical(pkg, scenes, integ):
    need_gpu(pkg)
    films = {}
    for n_lights, world in sorted(LIGHTS.items()):
        for ns in (1, 4):
            name = "%s, %d lights, nsamples %d" % (integ, n_lights, ns)
            text = scenes.cornell_scene(soup_tris=3000, soup_materials=True, xres=64, yres=48, xsamples=2, ysamples=2, jitter=True, maxdepth=5,
                                        world_kwargs=dict(light_nsamples=ns, **world), **INTEGRATORS[integ])
            ps = pkg.ParsedScene(text=text)
            assert ps.valid and ps.errors == 0, name
            ds = pkg.DeviceScene(ps)
            try:
                ref, cnt = assert_flavours_agree(ds, name, PIPELINE_ENVS)
            finally:
                ds.close()
            assert np.isfinite(ref).all() and ref[:3].max() > 0, name
            assert cnt["camera_rays"] == ps.n_camera_samples and cnt["bad_samples"] == 0, (name, cnt)
            assert cnt["any_rays"] > 0, (name, cnt)                      # shadow rays: the loop ran
            films[(n_lights, ns)] = ref
            ps.close()
    # every further light is in the loop: it changes the film
    for ns in (1, 4):
        assert not np.array_equal(films[(1, ns)], films[(2, ns)]) and not np.array_equal(films[(2, ns)], films[(3, ns)]), (integ, ns)
