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


@pytest.mark.gpu
def test_the_scene_keeps_its_lights_sample_counts_on_the_host(pkg, scenes):
    """DirectLighting "all" lays out three sample requests per light from the lights' sample counts.  The scene keeps them on the host from the loop that
    fills the uploaded records (SceneFacts::light_samples, rt_frame_plan.h): a frame reads nothing back.  Seen from outside: the counts set the shadow
    rays of a frame, a light of 65536 samples is refused by "all" with the request table's message before anything is launched, and "one", which asks
    for one sample whatever the light says, renders the same scene."""
    need_gpu(pkg)
    rays = {}
    for ns in (1, 3, 65536):
        kw = dict(xres=8, yres=8, xsamples=1, ysamples=1, jitter=False, keyed=True, count=True, world_kwargs=dict(light_nsamples=ns))
        ps = pkg.ParsedScene(text=scenes.cornell_scene(**kw, **INTEGRATORS["direct_all"]))
        assert ps.valid and ps.errors == 0 and ps.lights()[0]["nsamples"] == ns
        ds = pkg.DeviceScene(ps)
        try:
            if ns == 65536:
                with pytest.raises(pkg.RtError, match="more than 65535 samples per light"):
                    ds.render()
                assert ds.counters()["camera_rays"] == 0                   # nothing was launched
            else:
                ds.render()
                rays[ns] = ds.counters()
                assert rays[ns]["camera_rays"] == ps.n_camera_samples and rays[ns]["bad_samples"] == 0
        finally:
            ds.close()
        ps.close()
        if ns == 65536:
            ps = pkg.ParsedScene(text=scenes.cornell_scene(**kw, **INTEGRATORS["direct_one"]))
            ds = pkg.DeviceScene(ps)
            try:
                ds.render()
                assert ds.counters()["camera_rays"] == ps.n_camera_samples
            finally:
                ds.close()
            ps.close()
    # matte surfaces only: a camera ray has at most one shading point, and an estimate casts at most one shadow ray -- one sample per light cannot
    # cast more shadow rays than there are camera rays, three samples do (most points see the light) and cannot cast more than three times as many
    n = rays[1]["camera_rays"]
    assert n == rays[3]["camera_rays"] and 0 < rays[1]["any_rays"] <= n < rays[3]["any_rays"] <= 3 * n, rays
