"""Rate of light queries at points that live in device memory, on the scene of bench.py's headline workload (C3: the Cornell box
plus a 1 M-triangle soup, 1920 x 1080 at 16 samples per pixel; one two-triangle emitter).

    python tools/light_query_rate.py [--steps K] [--warmup W] [--tris N] [--max-rays M]

The frame's camera rays are generated and traced once on the device (camera_rays_device, intersect); the query points are the hits' dg.p with the
shading normal (a miss asks at the origin), the light is light 0 for all, u uniform in [0, 1), wi uniform on the sphere, rng NULL (key = i, counter 0).
Then, alternating in one process, with every output buffer allocated beforehand,
  (a) rt_light_device, the five sampling outputs (s_wi, s_L, s_pdf, s_ray, s_draws)
  (b) rt_light_device, s_wi + s_L + s_pdf alone
  (c) rt_bsdf_device, all eight outputs           (the neighbouring query, on the same hits)
  (d) a device-to-device copy of the rays         (32 bytes read and 32 written per ray: the float4-copy rate of this run)
are timed with events on torch's current stream around the call (the scene's stream is ordered against it as DeviceScene's wrappers do).  One JSON
line: per query the times of every step, the median, Mqueries/s at the median, the bytes a query reads and writes and its share of (d)'s rate."""
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
    lights = ps.lights()
    assert len(lights) == 1 and lights[0]["type"] == "area" and lights[0]["n_tris"] == 2, lights
    ds = pkg.DeviceScene(ps)
    setup_s = time.time() - t0
    ds.set_counting(False)
    n = ps.n_camera_samples if args.max_rays <= 0 else min(args.max_rays, ps.n_camera_samples)
    rays = ds.camera_rays_device(0, n)
    hits = ds.intersect(rays, fields=("p", "ns"))
    n_hits = int((hits["prim"] >= 0).sum().item())
    rec = torch.as_strided(hits["prim"].view(torch.float32), (n, 4), (4, 1))
    gen = torch.Generator(device="cuda").manual_seed(1)
    wi = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=gen), dim=1).contiguous()
    u3 = torch.rand((n, 3), device="cuda", generator=gen).clamp_(max=1 - 2.0 ** -24)
    u2 = u3[:, :2].contiguous()
    li = torch.zeros(n, dtype=torch.int32, device="cuda")
    f3 = lambda: torch.empty((n, 3), dtype=torch.float32, device="cuda")
    f1 = lambda: torch.empty(n, dtype=torch.float32, device="cuda")
    i1 = lambda: torch.empty(n, dtype=torch.int32, device="cuda")
    lout = dict(s_wi=f3(), s_L=f3(), s_pdf=f1(), s_ray=torch.empty((n, 8), dtype=torch.float32, device="cuda"), s_draws=i1())
    bout = dict(f=f3(), pdf=f1(), s_wi=f3(), s_f=f3(), s_pdf=f1(), s_type=i1(), n_components=i1(), le=f3())
    copy_dst = torch.empty_like(rays)
    seed = ps.render_view()["seed"]
    ins = dict(p=hits["p"].data_ptr(), nrm=hits["ns"].data_ptr(), light=li.data_ptr(), u=u2.data_ptr(), seed=seed)
    q_all = pkg.RtLightQuery(**ins, **{k: t.data_ptr() for k, t in lout.items()})
    q_three = pkg.RtLightQuery(**ins, **{k: lout[k].data_ptr() for k in ("s_wi", "s_L", "s_pdf")})
    q_bsdf = pkg.RtBsdfQuery(wi=wi.data_ptr(), u=u3.data_ptr(), **{k: t.data_ptr() for k, t in bout.items()})
    L = pkg.hip_lib()
    rp, hp = C.c_void_p(rays.data_ptr()), C.c_void_p(rec.data_ptr())

    def copy():
        copy_dst.copy_(rays)
        return 0
    # bytes per query: p, n (12 B each), light (4 B) and u (8 B) read, plus the outputs written
    queries = {"a_light_sampling_outputs": (lambda: L.rt_light_device(ds._s, n, C.byref(q_all)), 36 + 2 * 12 + 4 + 32 + 4),
               "b_light_wi_L_pdf": (lambda: L.rt_light_device(ds._s, n, C.byref(q_three)), 36 + 2 * 12 + 4),
               "c_bsdf_all_outputs": (lambda: L.rt_bsdf_device(ds._s, rp, hp, n, C.byref(q_bsdf)), 48 + 24 + 4 * 12 + 2 * 4 + 2 * 4),
               "d_float4_copy": (copy, 64)}
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
    usable = int(((lout["s_pdf"] > 0) & (lout["s_L"] > 0).any(1)).sum().item())
    ds.close()
    res = {"tool": "light_query_rate", "lib": os.path.basename(pkg.HIP_LIB), "code_id": pkg.code_id(), "tris": args.tris, "queries_per_call": n, "hits": n_hits,
           "usable_samples": usable, "setup_s": round(setup_s, 1), "queries": {}}
    copy_rate = n * 64 / statistics.median(ev_ms["d_float4_copy"]) / 1e9
    for k, (_, nbytes) in queries.items():
        med = statistics.median(ev_ms[k])
        rate = n * nbytes / med / 1e9
        res["queries"][k] = {"timed_by": "events", "event_ms": ev_ms[k], "median_ms": med, "mqueries_per_s": round(n / med / 1e3, 1), "bytes_per_query": nbytes,
                             "tb_per_s_at_median": round(rate, 2), "share_of_copy_rate": round(rate / copy_rate, 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
