"""Rate of BSDF queries at hits that live in device memory, on the scene of bench.py's headline workload (C3: the Cornell box
plus a 1 M-triangle soup, 1920 x 1080 at 16 samples per pixel).

    python tools/bsdf_query_rate.py [--steps K] [--warmup W] [--tris N] [--max-rays M]

The frame's camera rays are generated and traced once on the device (camera_rays_device, rt_trace_closest_device); wi is uniform on the sphere,
u uniform in [0, 1), flags BSDF_ALL.  Then, alternating in one process, with every output buffer allocated beforehand,
  (a) rt_bsdf_device, all eight outputs
  (b) rt_bsdf_device, f alone
  (c) rt_hit_geometry_device, all six fields      (the neighbouring query on the same hits)
are timed with events on torch's current stream around the call (the scene's stream is ordered against it as DeviceScene's wrappers do).  One JSON
line: per query the times of every step, the median, Mqueries/s at the median and the bytes a query reads and writes."""
import argparse
import ctypes as C
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--max-rays", type=int, default=0)
    args = ap.parse_args()
    pkg = g.load_package()
    from pbrt_v1_amd import scenes
    t0 = time.time()
    ps = pkg.ParsedScene(text=scenes.cornell_scene(xres=1920, yres=1080, integrator="directlighting", xsamples=4, ysamples=4, jitter=True,
                                                   pixel_filter="mitchell", soup_tris=args.tris))
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    setup_s = time.time() - t0
    ds.set_counting(False)
    n = ps.n_camera_samples if args.max_rays <= 0 else min(args.max_rays, ps.n_camera_samples)
    rays = ds.camera_rays_device(0, n)
    hits = ds.intersect(rays, fields=())
    n_hits = int((hits["prim"] >= 0).sum().item())
    rec = torch.as_strided(hits["prim"].view(torch.float32), (n, 4), (4, 1))
    gen = torch.Generator(device="cuda").manual_seed(1)
    wi = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=gen), dim=1).contiguous()
    u = torch.rand((n, 3), device="cuda", generator=gen).clamp_(max=1 - 2.0 ** -24)
    f3 = lambda: torch.empty((n, 3), dtype=torch.float32, device="cuda")
    f1 = lambda: torch.empty(n, dtype=torch.float32, device="cuda")
    i1 = lambda: torch.empty(n, dtype=torch.int32, device="cuda")
    out = dict(f=f3(), pdf=f1(), s_wi=f3(), s_f=f3(), s_pdf=f1(), s_type=i1(), n_components=i1(), le=f3())
    geo = dict(p=f3(), ng=f3(), ns=f3(), uv=torch.empty((n, 2), dtype=torch.float32, device="cuda"), material=i1(), light=i1())
    q_all = pkg.RtBsdfQuery(wi=wi.data_ptr(), u=u.data_ptr(), **{k: t.data_ptr() for k, t in out.items()})
    q_f = pkg.RtBsdfQuery(wi=wi.data_ptr(), f=out["f"].data_ptr())
    hg = pkg.RtHitGeometry(**{k: t.data_ptr() for k, t in geo.items()})
    L = pkg.hip_lib()
    rp, hp = C.c_void_p(rays.data_ptr()), C.c_void_p(rec.data_ptr())
    # bytes per query: 32 B RtRay + 16 B RtHit read, plus the inputs read and the outputs written
    queries = {"a_bsdf_all_outputs": (lambda: L.rt_bsdf_device(ds._s, rp, hp, n, C.byref(q_all)), 48 + 24 + 4 * 12 + 2 * 4 + 2 * 4),
               "b_bsdf_f_alone": (lambda: L.rt_bsdf_device(ds._s, rp, hp, n, C.byref(q_f)), 48 + 12 + 12),
               "c_hit_geometry_all_fields": (lambda: L.rt_hit_geometry_device(ds._s, rp, hp, n, C.byref(hg)), 48 + 3 * 12 + 8 + 2 * 4)}
    cur, mine = ds._scene_stream(torch, rays.device)
    ev_ms = {k: [] for k in queries}
    for step in range(args.warmup + args.steps):
        for k, (call, _) in queries.items():           # alternating: every query once per step
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if mine is not None:
                mine.wait_stream(cur)
            rc = call()
            if mine is not None:
                cur.wait_stream(mine)
            e1.record()
            torch.cuda.synchronize()
            if rc != 0:
                raise SystemExit("%s: rt error %d: %s" % (k, rc, L.rt_last_error().decode()))
            if step >= args.warmup:
                ev_ms[k].append(round(e0.elapsed_time(e1), 3))
    lobes = int((out["n_components"] > 0).sum().item())
    ds.close()
    res = {"tool": "bsdf_query_rate", "lib": os.path.basename(pkg.HIP_LIB), "code_id": pkg.code_id(), "tris": args.tris, "queries_per_call": n, "hits": n_hits,
           "hits_with_a_bsdf": lobes, "setup_s": round(setup_s, 1), "queries": {}}
    for k, (_, nbytes) in queries.items():
        med = statistics.median(ev_ms[k])
        res["queries"][k] = {"timed_by": "events", "event_ms": ev_ms[k], "median_ms": med, "mqueries_per_s": round(n / med / 1e3, 1), "bytes_per_query": nbytes,
                             "tb_per_s_at_median": round(n * nbytes / med / 1e9, 2)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
