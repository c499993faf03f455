"""Cost of a film add (rt_film_add_device) against the film gather of the same frame, on bench.py's headline scene (C3: the Cornell
box plus a 1 M-triangle soup, DirectLighting, 1920 x 1080 at 16 samples per pixel) and on the Cornell path frame (C2: 1024 x 1024 at 64 samples per
pixel, maxdepth 5).

    python tools/film_add_rate.py [--steps K] [--warmup W] [--tris N] [--frames c3,c2] [--chunk M]

In one process, alternating per step:
  render()                              gather_ms of rt_last_render_stats: the frame's own film gather -- the YARDSTICK, existing code
  add_samples(L)                        the whole frame's radiances, events on the scene's stream around the call (an add records none of its own)
  add_samples(L[a:a + M], first=a)      one chunk of M samples from the middle of the frame
with L = radiance(camera_rays_device(0, N)), the frame's own radiances, made once.  One JSON line: the times of every step, the medians, the add's
time relative to the frame's gather, the chunk's time beside its share of the gather, and whether the add gave the frame's film bit for bit."""
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

FRAMES = {"c3": (True, dict(xres=1920, yres=1080, integrator="directlighting", xsamples=4, ysamples=4, jitter=True, pixel_filter="mitchell")),
          "c3_box": (True, dict(xres=1920, yres=1080, integrator="directlighting", xsamples=4, ysamples=4, jitter=True, pixel_filter="box")),
          "c2": (False, dict(xres=1024, yres=1024, integrator="path", maxdepth=5, xsamples=8, ysamples=8, jitter=True, pixel_filter="mitchell"))}


def timed_add(ds, stream, L, first=0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):                    # torch's current stream = the scene's: the wrapper then orders nothing
        e0.record()
        ds.add_samples(L, first=first)
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frames", default="c3,c2")
    ap.add_argument("--chunk", type=int, default=1 << 20)
    args = ap.parse_args()
    pkg = g.load_package()
    from pbrt_v1_amd import scenes
    res = {"tool": "film_add_rate", "lib": os.path.basename(pkg.HIP_LIB), "code_id": pkg.code_id(), "tris": args.tris, "frames": {}}
    for frame in args.frames.split(","):
        t0 = time.time()
        soup, opts = FRAMES[frame]
        ps = pkg.ParsedScene(text=scenes.cornell_scene(soup_tris=args.tris if soup else 0, **opts))
        assert ps.valid and ps.errors == 0
        ds = pkg.DeviceScene(ps)
        ds.bind_film(); ds.set_counting(False)
        dev = torch.device("cuda", torch.cuda.current_device())
        _, mine = ds._scene_stream(torch, dev)
        stream = mine if mine is not None else torch.cuda.current_stream(dev)
        n = ps.n_camera_samples
        L = ds.radiance(ds.camera_rays_device(0, n))
        torch.cuda.synchronize()
        m = min(args.chunk, n)
        a = (n - m) // 2
        chunk = L[a:a + m].contiguous()
        rec = {"samples": n, "chunk_samples": m, "setup_s": round(time.time() - t0, 1)}
        ms = {"gather": [], "add": [], "chunk": []}
        for step in range(args.warmup + args.steps):
            ds.clear_film()
            ds.render()
            st = ds.last_stats()
            if step == 0:
                film = ds.film_accum()
            ds.clear_film()
            add_ms = timed_add(ds, stream, L)
            if step == 0:
                rec["add_equals_the_frames_film"] = bool(np.array_equal(ds.film_accum().view(np.uint32), film.view(np.uint32)))
                del film
            chunk_ms = timed_add(ds, stream, chunk, first=a)
            if step >= args.warmup:
                ms["gather"].append(round(st["gather_ms"], 3)); ms["add"].append(round(add_ms, 3)); ms["chunk"].append(round(chunk_ms, 3))
        ds.close()
        del L, chunk
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec.update(ms=ms, median_ms=med, add_over_gather=round(med["add"] / med["gather"], 3),
                   chunk_share_of_gather_ms=round(med["gather"] * m / n, 4), chunk_over_its_share=round(med["chunk"] / (med["gather"] * m / n), 2),
                   add_msamples_per_s=round(n / med["add"] / 1e3, 1))
        res["frames"][frame] = rec
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
