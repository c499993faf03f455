"""Rate of medium queries at rays and points that live in device memory, on the scene of bench.py's `c5` workload (the Cornell box
plus a 1 M-triangle soup inside a homogeneous medium, 1024 x 1024 at 64 samples per pixel, stepsize 20) and on the same scene with the medium
replaced by a seeded 64^3 volumegrid over the same extent.

    python tools/medium_query_rate.py [--steps K] [--warmup W] [--tris N] [--max-rays M]

The frame's camera rays are generated and traced once on the device (camera_rays_device, intersect); light() gives the shadow rays from the hits to
the scene's one emitter (a miss asks at the origin).  Then, alternating in one process, with every output buffer allocated beforehand,
  (a) rt_medium_device, tr along the shadow rays, the form without u (Scene::Transmittance: one draw, Tau at 4 x stepsize)
  (b) rt_medium_device, tau with u along the camera rays cut at their hits (Tau at stepsize)
  (c) rt_medium_device, the five point outputs at the hits
  (d) a device-to-device copy of the rays         (32 bytes read and 32 written per ray: the float4-copy rate of this run)
  (a_grid), (b_grid) the first two on the volumegrid scene
are timed with events on torch's current stream around the call (the scene's stream is ordered against it as DeviceScene's wrappers do).  One JSON
line: per variant the times of every step, the median, Mqueries/s at the median, the Tau samples its marches take (counted on the host side from
the clipped intervals: ceil(length / step) per ray that meets the region) and their rate, the bytes a query reads and writes and its share of
(d)'s rate."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the device library is loaded: one HIP runtime serves torch and the library, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

GRID_N = 64


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
    text = scenes.cornell_scene(xres=1024, yres=1024, integrator="directlighting", xsamples=8, ysamples=8, jitter=True, pixel_filter="mitchell",
                                soup_tris=args.tris, volume_integrator='"single" "float stepsize" [20]', world_kwargs=dict(volume='"float g" [0]'))
    dens = np.round(np.random.default_rng(5).random(GRID_N ** 3) * 2.0, 3)
    grid_text, k = re.subn(r'Volume "homogeneous"([^\n]*)\n', lambda m: 'Volume "volumegrid"%s "integer nx" [%d] "integer ny" [%d] "integer nz" [%d] "float density" [%s]\n' % (
        m.group(1), GRID_N, GRID_N, GRID_N, " ".join("%g" % v for v in dens)), text)
    assert k == 1
    setups = {}
    for name, t in (("hom", text), ("grid", grid_text)):
        ps = pkg.ParsedScene(text=t)
        assert ps.valid and ps.errors == 0
        ds = pkg.DeviceScene(ps)
        ds.set_counting(False)
        setups[name] = (ps, ds)
    setup_s = time.time() - t0
    ps, ds = setups["hom"]
    step = ps.render_view()["step_size"]
    n = ps.n_camera_samples if args.max_rays <= 0 else min(args.max_rays, ps.n_camera_samples)
    rays = ds.camera_rays_device(0, n)
    hits = ds.intersect(rays, fields=("p", "ns"))
    n_hits = int((hits["prim"] >= 0).sum().item())
    gen = torch.Generator(device="cuda").manual_seed(1)
    u2 = torch.rand((n, 2), device="cuda", generator=gen).clamp_(max=1 - 2.0 ** -24)
    shadow = ds.light(hits["p"], torch.zeros(n, dtype=torch.int32, device="cuda"), n=hits["ns"], u=u2, fields=("s_ray",))["s_ray"]
    cut = rays.clone()
    cut[:, 7] = torch.where(hits["prim"] >= 0, hits["t"], rays[:, 7])
    u = u2[:, 0].contiguous()
    w = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=gen), dim=1).contiguous()
    wp = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=gen), dim=1).contiguous()
    p = hits["p"]
    del hits, u2
    f3 = lambda: torch.empty((n, 3), dtype=torch.float32, device="cuda")
    out3 = f3()
    pout = dict(sigma_a=f3(), sigma_s=f3(), sigma_t=f3(), lve=f3(), phase=torch.empty(n, dtype=torch.float32, device="cuda"))
    copy_dst = torch.empty_like(rays)
    host_values = dict(seed=ps.render_view()["seed"], step_size=step, volume_integrator=pkg.VOLUME_EMISSION)
    q_tr = pkg.RtMediumQuery(rays=shadow.data_ptr(), tr=out3.data_ptr(), **host_values)
    q_tau = pkg.RtMediumQuery(rays=cut.data_ptr(), u=u.data_ptr(), tau=out3.data_ptr(), **host_values)
    q_pt = pkg.RtMediumQuery(p=p.data_ptr(), w=w.data_ptr(), wp=wp.data_ptr(), **host_values, **{k: t.data_ptr() for k, t in pout.items()})
    L = pkg.hip_lib()

    def samples(dsx, r, h):
        """Tau samples of one call: per ray that meets the region ceil(world length inside / h); 0 for the homogeneous region's closed form"""
        if dsx is setups["hom"][1]:
            return 0
        t = dsx.medium(rays=r, fields=("t01", "hit"))
        length = (t["t01"][:, 1] - t["t01"][:, 0]).double() * torch.linalg.norm(r[:, 3:6].double(), dim=1)
        return int(torch.where(t["hit"] > 0, torch.ceil(length / h), torch.zeros_like(length)).sum().item())

    def copy():
        copy_dst.copy_(rays)
        return 0
    hom, grd = setups["hom"][1], setups["grid"][1]
    # bytes per query: the ray (32 B) -- and for (b) u (4 B) -- read, 12 B written; (c) p, w, wp read (36 B), 4 x 12 B + 4 B written
    queries = {"a_tr_shadow_rays": (lambda: L.rt_medium_device(hom._s, n, C.byref(q_tr)), 32 + 12, 0),
               "b_tau_camera_rays": (lambda: L.rt_medium_device(hom._s, n, C.byref(q_tau)), 32 + 4 + 12, 0),
               "c_point_outputs": (lambda: L.rt_medium_device(hom._s, n, C.byref(q_pt)), 36 + 52, 0),
               "d_float4_copy": (copy, 64, 0),
               "a_grid_tr_shadow_rays": (lambda: L.rt_medium_device(grd._s, n, C.byref(q_tr)), 32 + 12, samples(grd, shadow, 4 * step)),
               "b_grid_tau_camera_rays": (lambda: L.rt_medium_device(grd._s, n, C.byref(q_tau)), 32 + 4 + 12, samples(grd, cut, step))}
    streams = {id(hom): hom._scene_stream(torch, rays.device), id(grd): grd._scene_stream(torch, rays.device)}
    ev_ms = {k: [] for k in queries}
    for it in range(args.warmup + args.steps):
        for k, (call, _, _) in queries.items():        # alternating: every variant once per step
            cur, mine = streams[id(grd if "grid" in k else hom)]
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
            if it >= args.warmup:
                ev_ms[k].append(round(e0.elapsed_time(e1), 3))
    res = {"tool": "medium_query_rate", "lib": os.path.basename(pkg.HIP_LIB), "code_id": pkg.code_id(), "tris": args.tris, "queries_per_call": n, "hits": n_hits,
           "step_size": step, "grid": GRID_N, "setup_s": round(setup_s, 1), "queries": {}}
    hom.close(); grd.close()
    copy_rate = n * 64 / statistics.median(ev_ms["d_float4_copy"]) / 1e9
    for k, (_, nbytes, taus) in queries.items():
        med = statistics.median(ev_ms[k])
        rate = n * nbytes / med / 1e9
        res["queries"][k] = {"timed_by": "events", "event_ms": ev_ms[k], "median_ms": med, "mqueries_per_s": round(n / med / 1e3, 1), "tau_samples": taus,
                             "g_tau_samples_per_s": round(taus / med / 1e6, 2), "bytes_per_query": nbytes, "tb_per_s_at_median": round(rate, 2),
                             "share_of_copy_rate": round(rate / copy_rate, 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
