"""Cost of a radiance query (rt_radiance_device) against the render kernel of the same frame, on bench.py's headline scene (C3: the
Cornell box plus a 1 M-triangle soup, DirectLighting, 1920 x 1080 at 16 samples per pixel) and on the 1 M-triangle path frame (1024 x 1024 at 16
samples per pixel, maxdepth 5).

    python tools/radiance_query_rate.py [--steps K] [--warmup W] [--tris N] [--frames c3,path]

Per frame two scenes are opened: the frame as bench.py states it, whose render() takes the headline kernel (high occupancy, fixed frame), and the
same frame with one plastic quad on the floor, which makes render() take the kernel with the EXT shading set at natural allocation -- the
YARDSTICK: the code a query runs, with the camera as ray source and the sample buffer as sink.  In one process, alternating per step:
  render()                          kernel time from rt_last_render_stats (render_ms: the render kernel alone, without the film gather)
  radiance(camera_rays_device)      events on the scene's stream around the call (the query records none of its own: it is not a frame)
on both scenes, the frame's own rays as the query's rays.  One JSON line: the times of every step, the medians, the query's time relative to the
yardstick kernel and to the headline kernel, and whether the query returned the frame's records bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the device library is loaded: one HIP runtime serves torch and the library, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PBRT_HIP_TUNE", "1")
import __graft_entry__ as g  # noqa: E402

PLASTIC = ('AttributeBegin\n  Material "plastic" "color Kd" [.4 .4 .5] "color Ks" [.3 .3 .3] "float roughness" [.1]\n'
           '  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [150 1 150 400 1 150 400 1 400 150 1 400]\nAttributeEnd\n')
FRAMES = {"c3": dict(xres=1920, yres=1080, integrator="directlighting", xsamples=4, ysamples=4, jitter=True, pixel_filter="mitchell"),
          "path": dict(xres=1024, yres=1024, integrator="path", maxdepth=5, xsamples=4, ysamples=4, jitter=True, pixel_filter="mitchell")}


def timed_query(ds, stream, rays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):                    # torch's current stream = the scene's: the wrapper then orders nothing
        e0.record()
        out = ds.radiance(rays)
        e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frames", default="c3,path")
    args = ap.parse_args()
    pkg = g.load_package()
    from pbrt_v1_amd import scenes
    res = {"tool": "radiance_query_rate", "lib": os.path.basename(pkg.HIP_LIB), "code_id": pkg.code_id(), "tris": args.tris, "frames": {}}
    for frame in args.frames.split(","):
        t0 = time.time()
        opened = {}
        for which, wk in (("headline", {}), ("ext", dict(extra=PLASTIC))):
            ps = pkg.ParsedScene(text=scenes.cornell_scene(soup_tris=args.tris, world_kwargs=wk, **FRAMES[frame]))
            assert ps.valid and ps.errors == 0
            ds = pkg.DeviceScene(ps)
            ds.bind_film(); ds.set_counting(False)
            dev = torch.device("cuda", torch.cuda.current_device())
            _, mine = ds._scene_stream(torch, dev)
            stream = mine if mine is not None else torch.cuda.current_stream(dev)
            opened[which] = (ps, ds, stream, ds.camera_rays_device(0, ps.n_camera_samples))
        rec = {"samples": opened["ext"][0].n_camera_samples, "setup_s": round(time.time() - t0, 1)}
        ms = {k: [] for k in ("headline_render", "headline_query", "ext_render", "ext_query")}
        stats = {}
        for step in range(args.warmup + args.steps):
            for which, (ps, ds, stream, rays) in opened.items():     # alternating: every kernel once per step
                ds.clear_film()
                ds.render()
                st = ds.last_stats()
                out, q_ms = timed_query(ds, stream, rays)
                if step >= args.warmup:
                    ms[which + "_render"].append(round(st["render_ms"], 3)); ms[which + "_query"].append(round(q_ms, 3))
                if step == 0:
                    stats[which] = {"pipeline": st["pipeline"], "fixed_frame": st["fixed_frame"],
                                    "query_equals_the_frames_records": bool(np.array_equal(out.cpu().numpy().view(np.uint32), ds.samples()[:, :4].copy().view(np.uint32)))}
                del out
        for _, ds, _, _ in opened.values():
            ds.close()
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec.update(ms=ms, median_ms=med, render=stats,
                   query_over_yardstick=round(med["ext_query"] / med["ext_render"], 4),
                   query_over_headline=round(med["headline_query"] / med["headline_render"], 4),
                   msamples_per_s=round(rec["samples"] / med["ext_query"] / 1e3, 1))
        res["frames"][frame] = rec
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
