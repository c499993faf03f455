"""Time the C5 frame with its homogeneous medium and with the two density regions in its place (density media).

    python tools/density_frames.py [--frames homogeneous,exponential,volumegrid] [--steps K] [--warmup W]

C5 is bench.py's frame: Cornell + 1 M-triangle soup, 1024 x 1024 @ 64 spp, single scattering with stepsize 20, DirectLighting.  The
exponential region keeps the homogeneous region's box and constants with a = 1, b = .002 (the density falls from 1 at the floor to
0.33 at the ceiling); the volumegrid region is a 128^3 grid of seeded densities in [0, 2) over the same box (mean 1).  Each frame is
rendered with the timed kernels; one JSON line per frame gives the GPU milliseconds of every step (rt_last_render_stats) and their
median.  For kernel statistics run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/density_frames.py --steps 1`."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def c5_text():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pbrt_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench.workload("c5")[0]


def with_region(text, kind, pkg):
    m = re.search(r'Volume "homogeneous" ([^\n]*)\n', text)
    assert m, "C5 has a homogeneous region"
    params = m.group(1)
    if kind == "homogeneous":
        return text
    if kind == "exponential":
        region = 'Volume "exponential" %s "float a" [1] "float b" [.002]\n' % params
    else:
        n = 128
        vals = (np.random.default_rng(128).random(n ** 3) * 2.0).astype(np.float32)
        region = 'Volume "volumegrid" %s "integer nx" [%d] "integer ny" [%d] "integer nz" [%d] "float density" [%s]\n' % (
            params, n, n, n, pkg.format_f32(vals, 16))
    return text[:m.start()] + region + text[m.end():]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="homogeneous,exponential,volumegrid")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    pkg = g.load_package()
    base = c5_text()
    for kind in args.frames.split(","):
        t0 = time.time()
        ps = pkg.ParsedScene(text=with_region(base, kind, pkg))
        assert ps.valid and ps.errors == 0, kind
        ds = pkg.DeviceScene(ps)
        setup_s = time.time() - t0
        ds.bind_film(); ds.set_counting(False)
        for _ in range(args.warmup):
            ds.clear_film(); ds.render()
        ms, march = [], []
        for _ in range(args.steps):
            ds.clear_film(); ds.render()
            st = ds.last_stats()
            ms.append(round(st["total_ms"], 2)); march.append(round(st["march_ms"], 2))
        rgb, _ = ds.film()
        ds.close()
        print(json.dumps({"frame": kind, "ms": ms, "median_ms": statistics.median(ms), "march_ms": march, "setup_s": round(setup_s, 1),
                          "film_mean": float(rgb.mean()), "finite": bool(np.isfinite(rgb).all())}), flush=True)


if __name__ == "__main__":
    main()
