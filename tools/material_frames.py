"""Time a 1 M-triangle path-traced frame with glossy materials on the soup (shinymetal and translucent).

    python tools/material_frames.py [--frames plastic,mixed] [--steps K] [--warmup W] [--res N] [--spp-side S]

The frame is the Cornell box plus the 1 M-triangle soup of bench.py's workloads, path tracing (maxdepth 5), N x N pixels (default 1024)
at S x S jittered samples (default 2 x 2).  `plastic`: every soup triangle is plastic (the EXT kernels with the materials they had before);
`plastic_checker`: the same with a checkered Kd; `mixed`: the soup's triangles cycle through shinymetal, translucent and matte (triangle index modulo 3); `plastic_infinite`: the plastic frame with
the box's emitter replaced by an infinite light.  Each frame is rendered once with
the counting kernels (the ray count) and then with the timed kernels; one JSON line per frame gives the GPU milliseconds of every step
(rt_last_render_stats), their median and Mrays/s at the median.  To compare two builds of the device library, run it once per library
(PBRT_HIP_TUNE=1 PBRT_HIP_LIB_PATH=<libpbrt_hip_NAME.so>, tools/build_variant.py) alternately in one session."""
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

MATERIALS = {
    "plastic": ['Material "plastic" "color Kd" [.5 .45 .4] "color Ks" [.4 .4 .4] "float roughness" [.15]'],
    # the plastic frame with Kd from a checkerboard over every triangle's default uvs: evaluated and resolved per hit
    "plastic_checker": ['Texture "chk" "color" "checkerboard" "color tex1" [.5 .45 .4] "color tex2" [.2 .3 .5] "string aamode" ["none"] "float uscale" [4] "float vscale" [4]\n'
                        '  Material "plastic" "texture Kd" "chk" "color Ks" [.4 .4 .4] "float roughness" [.15]'],
    "mixed": ['Material "shinymetal" "color Ks" [.8 .7 .4] "color Kr" [.7 .7 .7] "float roughness" [.15]',
              'Material "translucent" "color Kd" [.6 .7 .5] "color Ks" [.3 .3 .3] "float roughness" [.15]',
              'Material "matte" "color Kd" [.6 .55 .5]'],
}


def frame_text(scenes, kind, soup, res, side):
    mats = MATERIALS["plastic" if kind == "plastic_infinite" else kind]
    cls = np.arange(soup.shape[0]) % len(mats)
    blocks = "".join("AttributeBegin # soup %d\n  %s\n  %sAttributeEnd\n" % (i, m, scenes.soup_shape_text(soup[cls == i])) for i, m in enumerate(mats))
    return scenes.options_block(xres=res, yres=res, integrator="path", maxdepth=5, xsamples=side, ysamples=side, jitter=True) + \
        (scenes.cornell_world(area_light=False, extra='LightSource "infinite" "color L" [.8 .9 1]\n' + blocks) if kind == "plastic_infinite" else scenes.cornell_world(extra=blocks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="plastic,mixed")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp-side", type=int, default=2)
    ap.add_argument("--tris", type=int, default=1000000)
    args = ap.parse_args()
    pkg = g.load_package()
    from pbrt_v1_amd import scenes
    soup = scenes.lcg_soup(args.tris)
    for kind in args.frames.split(","):
        t0 = time.time()
        ps = pkg.ParsedScene(text=frame_text(scenes, kind, soup, args.res, args.spp_side))
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
        ms = []
        for _ in range(args.steps):
            ds.clear_film(); ds.render()
            ms.append(round(ds.last_stats()["total_ms"], 2))
        rgb, _ = ds.film()
        ds.close()
        med = statistics.median(ms)
        print(json.dumps({"frame": kind, "lib": os.path.basename(pkg.HIP_LIB), "ms": ms, "median_ms": med, "rays": rays, "mrays_per_s": round(rays / med / 1e3, 1),
                          "setup_s": round(setup_s, 1), "film_mean": float(rgb.mean()), "finite": bool(np.isfinite(rgb).all())}), flush=True)


if __name__ == "__main__":
    main()
