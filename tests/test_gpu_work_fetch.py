"""The megakernel's work fetch (rt_render_kernel.h: a wave takes the sample list in chunks of 64 from its band's counter; rt_integrate.h
tile_order_to_sample / setup_sample / sample_write: divisions by frame constants through rt_fastdiv.h) on single-shard DirectLighting frames at the
smallest sizes where the block arithmetic and the chunk claim can go wrong: extents that are no multiple of the 32-pixel work block, totals that are
no multiple of the 64-sample chunk, fewer samples than one wave, a crop window -- with the XCD bands of the work list forced on and off.  Per frame:
the timed kernel's film is the counting twin's bit for bit, camera_rays is the frame's sample count, and rt_samples_read returns every sample once, in
its own pixel and stratum (each kernel renders into a scene of its own, whose sample buffer starts zero-filled: a record nobody wrote is at the origin)."""
import numpy as np
import pytest

from gpu_checks import need_gpu

SPP = {1: (1, 1), 4: (2, 2), 6: (3, 2), 16: (4, 4)}
FRAMES = {
    "1x1": dict(xres=1, yres=1, pixel_filter="box"),
    "33x33": dict(xres=33, yres=33, pixel_filter="box"),
    "70x45": dict(xres=70, yres=45, pixel_filter="box"),
    "97x31": dict(xres=97, yres=31, pixel_filter="box"),
    "crop": dict(xres=90, yres=70, pixel_filter="mitchell", crop=(0.21, 0.83, 0.13, 0.9)),      # (the filter's reach puts the extent's corner off the film's)
}


def _render(pkg, ps, counting):
    ds = pkg.DeviceScene(ps)
    try:
        ds.set_counting(counting)
        ds.render()
        assert ds.last_stats()["pipeline"] == 0
        return ds.film_accum(), ds.counters(), ds.samples()
    finally:
        ds.close()


def _check_samples(name, ps, rec, xs, ys):
    """every record lies in the pixel and the stratum its index names, and no two records are one sample"""
    x0, x1, y0, y1 = ps.sample_extent
    w, spp = x1 - x0, xs * ys
    n = np.arange(ps.n_camera_samples)
    assert rec.shape[0] == n.size, name
    pixel, s = n // spp, n % spp
    px, py = x0 + pixel % w, y0 + pixel // w
    ix, iy = rec[:, 4].astype(np.float64), rec[:, 5].astype(np.float64)
    assert np.isfinite(rec).all(), name
    # jittered stratified samples: pixel + (stratum + [0, 1)) / strata, strictly inside the pixel's square (a zero-filled record is at (0, 0): outside
    # every stratum but the first of the pixel at the origin, where the jitter is not 0 either)
    fx, fy = (ix - px) * xs - s % xs, (iy - py) * ys - s // xs
    ok = (fx >= -1e-4) & (fx <= 1 + 1e-4) & (fy >= -1e-4) & (fy <= 1 + 1e-4) & ((ix != 0) | (iy != 0))
    assert ok.all(), (name, "records out of place", int((~ok).sum()), n[~ok][:8].tolist())
    assert np.unique(rec[:, 4:6], axis=0).shape[0] == n.size, (name, "duplicated records")


@pytest.mark.gpu
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_every_sample_fetched_once(pkg, scenes, frame):
    need_gpu(pkg)
    for spp, (xs, ys) in sorted(SPP.items()):
        text = scenes.cornell_scene(integrator="directlighting", xsamples=xs, ysamples=ys, jitter=True, **FRAMES[frame])
        ps = pkg.ParsedScene(text=text)
        assert ps.valid and ps.errors == 0 and ps.spp == spp
        if frame != "crop":                                  # (the sample extent is a pixel larger each way: the box filter's reach)
            assert "%dx%d" % (ps.width, ps.height) == frame
        for bands in ("0", "1"):
            name = "%s @ %d spp, PBRT_HIP_XCD_BANDS=%s" % (frame, spp, bands)
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("PBRT_HIP_XCD_BANDS", bands)
                mp.setenv("PBRT_HIP_PIPELINE", "0")
                ref, cnt, rec = _render(pkg, ps, True)
                film, _, trec = _render(pkg, ps, False)
            assert cnt["camera_rays"] == ps.n_camera_samples, (name, cnt)
            assert cnt["bad_samples"] == 0, (name, cnt)
            assert np.array_equal(film, ref), (name, float(np.abs(film - ref).max()))
            assert np.array_equal(trec, rec), (name, "sample records of the timed kernel and its counting twin differ")
            _check_samples(name, ps, rec, xs, ys)
            _check_samples(name, ps, trec, xs, ys)
        ps.close()
