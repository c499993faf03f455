"""Rate of ray queries on rays that live in device memory, on the scene of bench.py's headline workload (C3: the Cornell box
plus a 1 M-triangle soup, 1920 x 1080 at 16 samples per pixel).

    python tools/ray_query_rate.py [--steps K] [--warmup W] [--tris N] [--max-rays M] [--counting]

The frame's camera rays are generated on the device (DeviceScene.camera_rays_device) and then, alternating in one process,
  (a) intersect(fields=())          rt_trace_closest_device: hits only
  (b) intersect(all six fields)     ... plus rt_hit_geometry_device
  (c) occluded                      rt_trace_any_device
  (d) trace_closest                 the host-array entry point on the same rays copied to the host (repack, upload, trace, download)
are timed: (a) - (c) with events on torch's current stream around the call (the wrappers order the scene's stream inside them) and by the
wall clock around call + synchronize, (d) by the wall clock (its cost is on the host).  One JSON line: per query the times of every step, the
median and Mrays/s at the median.  --max-rays M takes the first M camera rays only (0, the default: the whole frame)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  (before the device library is loaded: one HIP runtime serves torch and the library, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--max-rays", type=int, default=0)
    ap.add_argument("--counting", action="store_true", help="leave the counting twin of the trace kernel on (default: the timed kernel)")
    args = ap.parse_args()
    pkg = g.load_package()
    from pbrt_v1_amd import scenes
    t0 = time.time()
    ps = pkg.ParsedScene(text=scenes.cornell_scene(xres=1920, yres=1080, integrator="directlighting", xsamples=4, ysamples=4, jitter=True,
                                                   pixel_filter="mitchell", soup_tris=args.tris))
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    setup_s = time.time() - t0
    ds.set_counting(args.counting)
    n = ps.n_camera_samples if args.max_rays <= 0 else min(args.max_rays, ps.n_camera_samples)
    rays = ds.camera_rays_device(0, n)
    torch.cuda.synchronize()
    host_rays = rays.cpu().numpy().view(pkg.RAY_DTYPE).reshape(n)
    all_fields = pkg.HIT_FIELDS
    queries = {"a_hits_only": lambda: ds.intersect(rays, fields=()), "b_all_fields": lambda: ds.intersect(rays, fields=all_fields),
               "c_occluded": lambda: ds.occluded(rays), "d_host_arrays": lambda: ds.trace_closest(host_rays)}
    ev_ms = {k: [] for k in queries}
    wall_ms = {k: [] for k in queries}
    hits = None
    for step in range(args.warmup + args.steps):
        for k, q in queries.items():                   # alternating: every query once per step
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record()
            out = q()
            e1.record()
            torch.cuda.synchronize()
            w1 = time.perf_counter()
            if step >= args.warmup:
                wall_ms[k].append(round((w1 - w0) * 1e3, 3))
                if k != "d_host_arrays":
                    ev_ms[k].append(round(e0.elapsed_time(e1), 3))
            if k == "a_hits_only":
                hits = int((out["prim"] >= 0).sum().item())
            del out
    ds.close()
    res = {"tool": "ray_query_rate", "lib": os.path.basename(pkg.HIP_LIB), "code_id": pkg.code_id(), "tris": args.tris, "rays": n, "hits": hits,
           "counting": bool(args.counting), "setup_s": round(setup_s, 1), "queries": {}}
    for k in queries:
        timed = ev_ms[k] if ev_ms[k] else wall_ms[k]
        med = statistics.median(timed)
        res["queries"][k] = {"timed_by": "events" if ev_ms[k] else "wall clock", "event_ms": ev_ms[k], "wall_ms": wall_ms[k], "median_ms": med,
                             "mrays_per_s": round(n / med / 1e3, 1), "wall_median_ms": statistics.median(wall_ms[k]),
                             "wall_mrays_per_s": round(n / statistics.median(wall_ms[k]) / 1e3, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
