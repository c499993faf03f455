"""Rays and hits in device memory on the GPU: DeviceScene.intersect / occluded / camera_rays_device (rt_trace_closest_device, rt_trace_any_device,
rt_hit_geometry_device, rt_camera_rays_device) against the host-array entry points bit for bit, against the debug integrator's records bit for
bit (the same code on the same rays), against the reference's own Intersection records (probe_cornell, the three quadric probes, the two
fixtures of tests/golden/rays/) and the float64 forms, with field selection, misses, guarded slack, the refusals and a prebuilt scene.
No test feeds a non-finite ray: that guard is tested on the host (tests/test_rays_host.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
# torch BEFORE the device library is loaded, as bench.py does: torch carries a HIP runtime of its own, and the first one a process loads serves both
# (pbrt-v1_amd/__init__.py, "rays and hits in device memory").  A test module is imported when the session is collected, before any fixture loads the library.
import torch

import analytic_cases as A
import rays_cases as R
from conftest import GOLDEN, load_golden
from gpu_checks import need_gpu

pytestmark = pytest.mark.gpu

F32_HALF_ULP = 2.0 ** -24      # a float32 result cannot be nearer to float64 than its own rounding
ROUNDING = 2 * F32_HALF_ULP * A.BAR_FACTOR      # the bar tests/test_gpu_analytic.py holds maxt to
SIZES = (1, 63, 64, 65, 255, 256, 257, 100003)
TRAV_KEYS = ("nodes_visited", "leaf_refs", "tri_tests")
ALL_FIELDS = ("p", "ng", "ns", "uv", "material", "light")


def as_whitted(text):
    return str(text).replace('SurfaceIntegrator "probe"', 'SurfaceIntegrator "whitted"')


def to_device(rays):
    """RAY_DTYPE records -> float32 [n, 8] tensor in device memory"""
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def rays_of_records(pkg, rec):
    rays = np.zeros(len(rec), pkg.RAY_DTYPE)
    rays["o"], rays["d"], rays["mint"], rays["maxt"] = rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7]
    return rays


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def open_scene(pkg, text):
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    return ps, pkg.DeviceScene(ps)


def scene_texts():
    return {"probe_cornell (kd-tree)": as_whitted(load_golden("probe_cornell")["scene"]),
            "debug_quadrics_grid (grid, quadrics)": load_golden("debug/debug_quadrics_grid")["scene"],
            "soup of 5 k triangles": load_golden("direct_soup5k_seed7")["scene"]}


# ---------------------------------------------------------------------------------------------- 1. the host path's hits, bit for bit
@pytest.mark.parametrize("label", list(scene_texts()))
def test_same_hits_and_counts_as_the_host_entry_points(pkg, label):
    """intersect(fields=()) == trace_closest in prim, t, b1, b2 and occluded == trace_any, for n around the wave and block sizes and for 100 003
    rays (the camera rays tiled), with counting on and off: on, the traversal counters advance by what the host path adds for the same rays;
    off, they do not move"""
    need_gpu(pkg)
    ps, ds = open_scene(pkg, scene_texts()[label])
    every = ds.camera_rays(0, ps.n_camera_samples)
    base = every[np.linspace(0, len(every) - 1, 625).astype(np.int64)]          # 625 rays spread over the frame
    for n in SIZES:
        rays = np.tile(base, -(-n // len(base)))[:n]
        ds.set_counting(True); ds.reset_counters()
        hits = ds.trace_closest(rays)
        c_closest = ds.counters()
        ds.reset_counters()
        occ = ds.trace_any(rays)
        c_any = ds.counters()
        dev = to_device(rays)
        for counting in (True, False):
            ds.set_counting(counting); ds.reset_counters()
            got = host(ds.intersect(dev, fields=()))
            c = ds.counters()
            for k in ("prim", "t", "b1", "b2"):
                assert np.array_equal(got[k].view(np.uint32), hits[k].view(np.uint32)), (label, n, counting, k)
            assert all(c[k] == (c_closest[k] if counting else 0) for k in TRAV_KEYS), (label, n, counting, c, c_closest)
            ds.reset_counters()
            got_occ = ds.occluded(dev).cpu().numpy()
            c = ds.counters()
            assert got_occ.dtype == np.uint8 and np.array_equal(got_occ, occ), (label, n, counting)
            assert all(c[k] == (c_any[k] if counting else 0) for k in TRAV_KEYS), (label, n, counting, c, c_any)
        if n == SIZES[-1]:
            print("RAYS-HOST %s n %d hits %d occluded %d nodes %d tri tests %d" % (label, n, int((hits["prim"] >= 0).sum()), int(occ.sum()),
                                                                                  c_closest["nodes_visited"], c_closest["tri_tests"]))
            assert 0 < (hits["prim"] >= 0).sum() < n
    ds.close()


# ---------------------------------------------------------------------------------------------- 2. camera rays
CAMERA_SAMPLERS = {"stratified": '"integer xsamples" [2] "integer ysamples" [2] "bool jitter" ["true"]',
                   "lowdiscrepancy": '"integer pixelsamples" [3]',          # rounded up to 4
                   "random": '"integer xsamples" [2] "integer ysamples" [2]'}


def camera_scenes():
    out = {"perspective (probe_cornell)": as_whitted(load_golden("probe_cornell")["scene"])}
    for name in A.PROBES:
        out[name] = as_whitted(np.load(os.path.join(GOLDEN, "analytic", name + ".npz"))["scene"])
    # the two integrators whose sample requests live in a device table (DirectLighting "all": per light; bidirectional: its BidirTable), under each
    # sampler: a camera ray must not depend on them, nor wait for them
    probe = str(load_golden("probe_cornell")["scene"])
    for integ, line in (("directlighting all", 'SurfaceIntegrator "directlighting" "string strategy" ["all"]'), ("bidirectional", 'SurfaceIntegrator "bidirectional"')):
        for sampler, params in CAMERA_SAMPLERS.items():
            text = re.sub(r'^SurfaceIntegrator "probe".*$', line, probe, flags=re.M)
            text = re.sub(r'^Sampler "keyed".*$', 'Sampler "%s" "integer seed" [0] %s' % (sampler, params), text, flags=re.M)
            assert text.count(line) == 1 and text.count('Sampler "%s"' % sampler) == 1
            out["%s, %s (probe_cornell)" % (integ, sampler)] = text
    return out


@pytest.mark.parametrize("label", list(camera_scenes()))
def test_camera_rays_device_equals_camera_rays(pkg, label):
    """perspective, orthographic (screen window), environment and thin-lens frames, and DirectLighting "all" and bidirectional frames under the three
    samplers: the whole frame and a window that starts inside it"""
    need_gpu(pkg)
    ps, ds = open_scene(pkg, camera_scenes()[label])
    n = ps.n_camera_samples
    for first, count in ((0, n), (37, 101), (n - 1, 1)):
        want = ds.camera_rays(first, count).view(np.uint32).reshape(count, 8)
        got = ds.camera_rays_device(first, count)
        assert tuple(got.shape) == (count, 8) and got.is_cuda and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (label, first, count)
    assert tuple(ds.camera_rays_device(0, 0).shape) == (0, 8)
    ds.close()


# ---------------------------------------------------------------------------------------------- 3. the debug integrator's records
@pytest.mark.parametrize("name", ["debug_normals_mesh", "debug_ns_reversed", "debug_quadrics_grid", "debug_soup_ortho"])
def test_hit_geometry_equals_the_debug_integrators_records(pkg, name):
    """The frame rendered with the channel triples (u, v, hit), (nx, ny, nz), (snx, sny, snz): samples() of each against intersect on
    camera_rays_device of the same descriptor -- uv, |ng|, |ns| and prim >= 0, bit for bit.  (tests/test_gpu_debug.py holds the films to the reference.)"""
    need_gpu(pkg)
    ps, ds = open_scene(pkg, load_golden("debug/" + name)["scene"])
    assert ps.integrator == pkg.RT_INTEGRATOR_DEBUG
    n = ps.n_camera_samples
    rd = ps.render_struct()
    codes = lambda *names: sum(pkg.RT_DEBUG_NAMES.index(c) << (8 * i) for i, c in enumerate(names))
    rec = {}
    for triple in (("u", "v", "hit"), ("nx", "ny", "nz"), ("snx", "sny", "snz")):
        rd.strategy = codes(*triple)
        ds.render()
        rec[triple[0]] = ds.samples()[:, 0:3].copy()
    got = host(ds.intersect(ds.camera_rays_device(0, n), fields=("uv", "ng", "ns")))
    ds.close()
    hit = got["prim"] >= 0
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    print("RAYS-DEBUG %s samples %d hits %d" % (name, n, int(hit.sum())))
    assert 0 < hit.sum() < n
    assert np.array_equal(hit.astype(np.float32), rec["u"][:, 2])
    assert np.array_equal(bits(got["uv"]), bits(rec["u"][:, 0:2]))
    assert np.array_equal(bits(np.abs(got["ng"])), bits(rec["nx"]))
    assert np.array_equal(bits(np.abs(got["ns"])), bits(rec["snx"]))
    assert (got["uv"][~hit] == 0).all() and (got["ng"][~hit] == 0).all() and (got["ns"][~hit] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. the reference's records, existing fixtures
def test_probe_cornell_records(pkg):
    """triangles only: hit mask and t are the reference's bit for bit; p, nn, (u, v) within float32 rounding of its records"""
    need_gpu(pkg)
    g = load_golden("probe_cornell")
    rec = g["records"]
    ps, ds = open_scene(pkg, as_whitted(g["scene"]))
    got = host(ds.intersect(to_device(rays_of_records(pkg, rec))))
    ds.close()
    hit = rec[:, 8] > 0
    assert np.array_equal(got["prim"] >= 0, hit) and 0 < hit.sum() < len(rec)
    assert np.array_equal(got["t"][hit].view(np.uint32), rec[hit, 9].view(np.uint32))
    for what, a, b in (("p", got["p"], rec[:, 10:13]), ("ng", got["ng"], rec[:, 13:16]), ("uv", got["uv"], rec[:, 16:18])):
        print("RAYS-CORNELL %s largest difference %.3g" % (what, float(np.abs(a[hit] - b[hit]).max())))
        assert np.allclose(a[hit], b[hit], rtol=ROUNDING, atol=ROUNDING), what
    # triangles without per-vertex N / S: the shading normal is the geometric one
    assert np.array_equal(got["ns"], got["ng"])
    mat, light = ps.tri_tables()
    assert np.array_equal(got["material"][hit], mat[got["prim"][hit]].astype(np.int32)) and np.array_equal(got["light"][hit], light[got["prim"][hit]])
    assert (got["material"][~hit] == -1).all() and (got["light"][~hit] == -1).all()


def held_to_the_form(label, sc, g, got, with_ns):
    """outside the fixture's band: hit mask and t are the reference's bit for bit; p, ng, (u, v) (and ns) deviate from the float64 form by at most
    BAR_FACTOR x the reference's own recorded deviation, never below float32 half-ulp"""
    rec, band = g["records"], g["band"]
    assert band.mean() <= A.BAND_CAP
    inc = ~band
    hit = rec[:, 8] > 0
    assert np.array_equal((got["prim"] >= 0)[inc], hit[inc]), label
    assert np.array_equal(got["t"][inc & hit].view(np.uint32), rec[inc & hit, 9].view(np.uint32)), label
    f = R.evaluate(sc, rec, with_band=False)
    both = inc & hit & f["hit"]
    assert both.sum() >= 100, (label, int(both.sum()))
    d = R.deviations(f, got["t"], got["p"], got["ng"], got["uv"], both, ns=got["ns"] if with_ns else None)
    bars = dict(dev_p=float(g["dev_p"]), dev_n=float(g["dev_n"]), dev_uv=float(g["dev_uv"]), dev_ns=float(g["dev_n"]))
    for k, ref_dev in bars.items():
        if k in d:
            bar = max(A.BAR_FACTOR * ref_dev, F32_HALF_ULP)
            print("RAYS-FORM %s %s %.3g (bar %.3g, the reference's own %.3g)" % (label, k, d[k], bar, ref_dev))
    for k, ref_dev in bars.items():
        if k in d:
            assert d[k] <= max(A.BAR_FACTOR * ref_dev, F32_HALF_ULP), (label, k, d[k], ref_dev)
    return both


@pytest.mark.parametrize("name", list(A.PROBES))
def test_quadric_probes_against_the_reference_and_the_float64_forms(pkg, name):
    need_gpu(pkg)
    g = np.load(os.path.join(GOLDEN, "analytic", name + ".npz"))
    ps, ds = open_scene(pkg, as_whitted(g["scene"]))
    got = host(ds.intersect(to_device(rays_of_records(pkg, g["records"]))))
    ds.close()
    held_to_the_form(name, A.form(name), g, got, with_ns=False)
    assert np.array_equal(got["ns"], got["ng"])              # a quadric's shading normal is its geometric one


# ---------------------------------------------------------------------------------------------- 5. the new fixtures
@pytest.mark.parametrize("name", list(R.CASES))
def test_rays_fixtures_against_the_reference_and_the_float64_forms(pkg, name):
    """meshes with per-vertex uv, N and S under ReverseOrientation and under Scale -1 1 1 (kd-tree, perspective), and the same next to a partial
    sphere, a disk and a cylinder (grid, orthographic): p, ng, uv as above, ns against the form under the dev_n bar, material and light exactly
    the host tables' entries of the primitive hit"""
    need_gpu(pkg)
    g = np.load(os.path.join(GOLDEN, "rays", name + ".npz"))
    ps, ds = open_scene(pkg, R.product_text(g["scene"]))
    got = host(ds.intersect(to_device(rays_of_records(pkg, g["records"]))))
    ds.close()
    both = held_to_the_form(name, R.form(name), g, got, with_ns=True)
    # the shading normals are not the geometric ones here: the check above is one of ns
    assert np.abs(got["ns"][both] - got["ng"][both]).max() > 1e-2
    hit = got["prim"] >= 0
    mat, light = ps.tri_tables()
    assert np.array_equal(got["material"][hit], mat[got["prim"][hit]].astype(np.int32))
    assert np.array_equal(got["light"][hit], light[got["prim"][hit]])
    assert set(got["material"][hit].tolist()) == set(range(ps.n_materials)) and set(got["light"][hit].tolist()) == {-1, 0}
    assert (got["material"][~hit] == -1).all() and (got["light"][~hit] == -1).all()


# ---------------------------------------------------------------------------------------------- 6. field selection, misses, slack
def test_each_field_alone_misses_and_guarded_slack(pkg):
    need_gpu(pkg)
    g = np.load(os.path.join(GOLDEN, "rays", "rays_mixed_grid.npz"))
    ps, ds = open_scene(pkg, R.product_text(g["scene"]))
    rays = rays_of_records(pkg, g["records"])
    dev = to_device(rays)
    full = host(ds.intersect(dev))
    assert set(full) == {"prim", "t", "b1", "b2"} | set(ALL_FIELDS)
    for f in ALL_FIELDS:
        one = host(ds.intersect(dev, fields=(f,)))
        assert set(one) == {"prim", "t", "b1", "b2", f}
        for k in one:
            assert np.array_equal(one[k].view(np.uint32), full[k].view(np.uint32)), (f, k)
    # rays that point away from the world, and empty rays (mint > maxt): misses, zeros, -1
    away, empty = rays.copy(), rays.copy()
    away["d"] = -away["d"]
    empty["mint"], empty["maxt"] = 5.0, 1.0
    for label, r in (("away", away), ("empty", empty)):
        got = host(ds.intersect(to_device(r)))
        assert (got["prim"] == -1).all() and (ds.occluded(to_device(r)).cpu().numpy() == 0).all(), label
        for k in ("t", "b1", "b2", "p", "ng", "ns", "uv"):
            assert (got[k].view(np.uint32) == 0).all(), (label, k)
        assert (got["material"] == -1).all() and (got["light"] == -1).all(), label
    # slack behind the n records that are passed stays as it was
    n, pad = 1000, 64
    L = pkg.hip_lib()
    hits = torch.full((n + pad, 4), 7777.0, dtype=torch.float32, device="cuda")
    occ = torch.full((n + pad,), 77, dtype=torch.uint8, device="cuda")
    buf = {f: (torch.full((n + pad,), 7777, dtype=torch.int32, device="cuda") if f in ("material", "light") else
               torch.full((n + pad, 2 if f == "uv" else 3), 7777.0, dtype=torch.float32, device="cuda")) for f in ALL_FIELDS}
    torch.cuda.synchronize()
    geom = pkg.RtHitGeometry(**{f: t.data_ptr() for f, t in buf.items()})
    assert L.rt_trace_closest_device(ds._s, C.c_void_p(dev.data_ptr()), n, C.c_void_p(hits.data_ptr())) == 0
    assert L.rt_hit_geometry_device(ds._s, C.c_void_p(dev.data_ptr()), C.c_void_p(hits.data_ptr()), n, C.byref(geom)) == 0
    assert L.rt_trace_any_device(ds._s, C.c_void_p(dev.data_ptr()), n, C.c_void_p(occ.data_ptr())) == 0
    ds.sync()
    assert (hits[n:] == 7777.0).all().item() and (occ[n:] == 77).all().item()
    for f, t in buf.items():
        assert (t[n:] == 7777).all().item(), f
        assert np.array_equal(t[:n].cpu().numpy().view(np.uint32), full[f][:n].view(np.uint32)), f
    assert np.array_equal(hits[:n, 1].cpu().numpy().view(np.uint32), full["t"][:n].view(np.uint32))
    ds.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_name_their_cause(pkg):
    need_gpu(pkg)
    ps, ds = open_scene(pkg, as_whitted(load_golden("probe_cornell")["scene"]))
    L = pkg.hip_lib()
    rays = ds.camera_rays_device(0, 64)
    hits = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    occ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    R_, H_, O_ = rays.data_ptr(), hits.data_ptr(), occ.data_ptr()
    geom, nothing = pkg.RtHitGeometry(p=p.data_ptr()), pkg.RtHitGeometry()

    def refused(rc, *words):
        msg = L.rt_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (rc, msg, words)
    refused(L.rt_trace_closest_device(ds._s, C.c_void_p(R_ + 4), 8, C.c_void_p(H_)), "rt_trace_closest_device", "dev_rays", "16-byte aligned")
    refused(L.rt_trace_closest_device(ds._s, C.c_void_p(R_), 8, C.c_void_p(H_ + 4)), "dev_hits", "16-byte aligned")
    refused(L.rt_trace_any_device(ds._s, C.c_void_p(R_ + 4), 8, C.c_void_p(O_)), "rt_trace_any_device", "16-byte aligned")
    refused(L.rt_hit_geometry_device(ds._s, C.c_void_p(R_), C.c_void_p(H_ + 8), 8, C.byref(geom)), "rt_hit_geometry_device", "dev_hits", "16-byte aligned")
    refused(L.rt_camera_rays_device(ds._s, ps.render_desc, 0, 8, C.c_void_p(R_ + 4)), "rt_camera_rays_device", "16-byte aligned")
    big = 2 ** 30 + 1
    refused(L.rt_trace_closest_device(ds._s, C.c_void_p(R_), big, C.c_void_p(H_)), "above 2^30", str(big))
    refused(L.rt_trace_any_device(ds._s, C.c_void_p(R_), big, C.c_void_p(O_)), "above 2^30")
    refused(L.rt_hit_geometry_device(ds._s, C.c_void_p(R_), C.c_void_p(H_), big, C.byref(geom)), "above 2^30")
    refused(L.rt_camera_rays_device(ds._s, ps.render_desc, 0, big, C.c_void_p(R_)), "above 2^30")
    refused(L.rt_hit_geometry_device(ds._s, C.c_void_p(R_), C.c_void_p(H_), 8, C.byref(nothing)), "every field", "null")
    refused(L.rt_trace_closest_device(ds._s, None, 8, C.c_void_p(H_)), "null ray pointer")
    refused(L.rt_trace_closest_device(ds._s, C.c_void_p(R_), 8, None), "null hit pointer")
    refused(L.rt_trace_any_device(ds._s, C.c_void_p(R_), 8, None), "null output pointer")
    refused(L.rt_hit_geometry_device(ds._s, C.c_void_p(R_), C.c_void_p(H_), 8, None), "null RtHitGeometry")
    # n == 0 is success and launches nothing
    assert L.rt_trace_closest_device(ds._s, C.c_void_p(R_), 0, C.c_void_p(H_)) == 0
    assert L.rt_trace_any_device(ds._s, C.c_void_p(R_), 0, C.c_void_p(O_)) == 0
    assert L.rt_hit_geometry_device(ds._s, C.c_void_p(R_), C.c_void_p(H_), 0, C.byref(geom)) == 0
    assert L.rt_camera_rays_device(ds._s, ps.render_desc, 0, 0, C.c_void_p(R_)) == 0
    ds.sync()
    assert (hits == 0).all().item() and (occ == 0).all().item() and (p == 0).all().item()      # nothing above wrote anything
    # the wrapper hands a contiguous [n, 8] view that starts 4 bytes into an allocation to the library, which refuses it
    flat = torch.zeros(8 * 16 + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(16, 8)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(pkg.RtError, match="16-byte aligned"):
        ds.intersect(view)
    empty = ds.intersect(torch.zeros((0, 8), dtype=torch.float32, device="cuda"))
    assert tuple(empty["prim"].shape) == (0,) and tuple(empty["p"].shape) == (0, 3)
    ds.close()


# ---------------------------------------------------------------------------------------------- 8. prebuilt scenes
@pytest.mark.parametrize("name", list(R.CASES))
def test_prebuilt_scene_answers_the_same(pkg, name):
    """rt_scene_create_prebuilt on the accelerator of an rt_scene_create scene (gpu_checks.assert_prebuilt_agrees' construction)"""
    need_gpu(pkg)
    g = np.load(os.path.join(GOLDEN, "rays", name + ".npz"))
    ps, a = open_scene(pkg, R.product_text(g["scene"]))
    dev = to_device(rays_of_records(pkg, g["records"]))
    want, want_occ = host(a.intersect(dev)), a.occluded(dev).cpu().numpy()
    nodes, refs = a.accel_arrays()
    info = a.accel_info()
    a.close()
    b = pkg.DeviceScene(ps, prebuilt=(nodes, refs, info))
    got, got_occ = host(b.intersect(dev)), b.occluded(dev).cpu().numpy()
    b.close()
    assert (want["prim"] >= 0).sum() > 100
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
    assert np.array_equal(got_occ, want_occ)
