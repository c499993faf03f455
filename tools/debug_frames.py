"""Time the debug integrator's frame on the 1 M-triangle scene against the cheapest frame the device had before it.

    python tools/debug_frames.py [--frames debug,whitted_dark] [--steps K] [--warmup W] [--res N] [--spp-side S] [--channels nx,ny,nz]

The scene is the Cornell box plus the 1 M-triangle matte soup of bench.py's workloads, N x N pixels (default 1024) at S x S jittered samples
(default 2 x 2).  `debug`: SurfaceIntegrator "debug" with the given channels (one camera ray per sample, the hit's frame, no light, no BSDF);
`whitted_dark`: SurfaceIntegrator "whitted" on the same scene with every light removed -- one camera ray per sample and no shadow rays, the frame
a library without the debug integrator comes closest with.  Each frame is rendered once with the counting kernels (the ray count) and then with
the timed kernels; one JSON line per frame gives the GPU milliseconds of every step (rt_last_render_stats: the whole frame and the render kernel
alone), their medians and Mrays/s at the median.  To compare with another build of the device library, run it once per library
(PBRT_HIP_TUNE=1 PBRT_HIP_LIB_PATH=<libpbrt_hip_NAME.so>) alternately in one session, as tools/material_frames.py is."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def frame_text(scenes, kind, tris, res, side, channels):
    kw = dict(xres=res, yres=res, xsamples=side, ysamples=side, jitter=True, soup_tris=tris)
    if kind == "debug":
        params = '"string red" ["%s"] "string green" ["%s"] "string blue" ["%s"]' % tuple(channels)
        return scenes.cornell_scene(integrator="debug", integrator_params=params, **kw)
    if kind == "whitted_dark":
        return scenes.cornell_scene(integrator="whitted", maxdepth=5, world_kwargs=dict(area_light=False), **kw)
    raise SystemExit("unknown frame " + kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="debug,whitted_dark")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp-side", type=int, default=2)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--channels", default="nx,ny,nz")
    args = ap.parse_args()
    pkg = g.load_package()
    from pbrt_v1_amd import scenes
    for kind in args.frames.split(","):
        t0 = time.time()
        ps = pkg.ParsedScene(text=frame_text(scenes, kind, args.tris, args.res, args.spp_side, args.channels.split(",")))
        assert ps.valid and ps.errors == 0, kind
        ds = pkg.DeviceScene(ps)
        setup_s = time.time() - t0
        ds.bind_film()
        ds.render()                                      # counting kernels: the frame's rays
        cnt = ds.counters()
        rays = cnt["closest_rays"] + cnt["any_rays"]
        ds.set_counting(False)
        for _ in range(args.warmup):
            ds.clear_film(); ds.render()
        ms, kernel_ms = [], []
        for _ in range(args.steps):
            ds.clear_film(); ds.render()
            st = ds.last_stats()
            ms.append(round(st["total_ms"], 3)); kernel_ms.append(round(st["render_ms"], 3))
        rgb, alpha = ds.film()
        ds.close()
        med = statistics.median(ms)
        print(json.dumps({"frame": kind, "lib": os.path.basename(pkg.HIP_LIB), "ms": ms, "median_ms": med, "kernel_ms": kernel_ms,
                          "median_kernel_ms": statistics.median(kernel_ms), "camera_rays": cnt["camera_rays"], "rays": rays,
                          "mrays_per_s": round(rays / med / 1e3, 1), "setup_s": round(setup_s, 1), "film_mean": float(rgb.mean()),
                          "alpha_mean": float(alpha.mean()), "finite": bool(np.isfinite(rgb).all())}), flush=True)


if __name__ == "__main__":
    main()
