"""GPU parity tests: the HIP path, called through the C ABI (include/pbrt_hip.h), against
  (1) the committed golden films / probe records produced by the unmodified reference,
  (2) the CPU oracle on larger seeded inputs, with identical ray / node / triangle-test counts,
  (3) the compiled reference run live when oracle/_ref travelled with the repo,
  (4) size-independent properties at the benchmark's full size.
Tolerances (float32 path; BASELINE.json: per-pixel L2 < 1e-4):
  * Whitted / DirectLighting: every pixel within 1e-5 absolute of the reference film (observed: bit-exact or 6e-8);
  * Path: >= 99.5 % of pixels with per-pixel L2 < 1e-4 and mean per-pixel L2 < 1e-4 under the keyed RNG -- the
    residue is one divergent path per affected pixel where the device's cosf/sinf differ from glibc's in the last bit
    and flip a hit/miss decision (SURVEY.md section 4.1 measured 0.6 % for the reference against *itself* across
    compiler flags)."""
import numpy as np
import pytest
import __graft_entry__ as g_entry
from conftest import golden_names, load_golden, film_metrics
from gpu_checks import assert_flavours_agree, need_gpu

pytestmark = pytest.mark.gpu

FILMS = [n for n in golden_names() if not n.startswith("probe_")]


def libm_bound(name, integrator):
    """Scenes whose geometry goes through device libm (sinf/cosf/acosf/atan2f: cosine-sampled bounces of the path
    integrator, quadric hits) can flip a hit/miss at a silhouette by a last-bit difference from glibc: the bar there is the
    north-star's per-pixel L2 < 1e-4 on >= 99.5 % of pixels and on average, instead of every pixel."""
    return integrator == 2 or name.startswith("sphere_") or name.startswith("quadrics")


def oracle_one_ulp_sensitivity(pkg, oracle, ps, accel=None):
    """How much the REFERENCE ALGORITHM's own film moves when libm's cosf is one ulp different (CPU restatement with
    ConcentricSampleDisk's dx and the sphere emitter's cone direction bumped by one ulp).  pbrt-v1's fixed RAY_EPSILON = 1e-3 makes some scenes ill-conditioned:
    a ray leaving a transformed sphere at world coordinates ~400 re-hits it at t = 1e-3 +- rounding noise, so a last-bit
    change flips whole paths (measured: 5 % of the pixels of sphere_path_soup).  Such a scene cannot be reproduced pixel
    by pixel under any other libm; the bar for it is "no further from the reference than the reference is from itself".
    A second source: a PARTIAL sphere used as an area light.  When the sampled cone direction passes through the clipped-away
    part, Sphere::Sample falls back to the point of closest approach to the centre (sphere.cpp:63-66), whose normal is
    perpendicular to the ray by construction, so the sign of a rounding-noise dot product decides between Lemit and black."""
    import ctypes as C
    L = oracle.lib()
    L.oracle_set_perturb.restype = None; L.oracle_set_perturb.argtypes = [C.c_int]
    nodes, refs, bounds, info = accel if accel is not None else ps.kdtree()      # accel: the device scene's arrays (kd-tree or grid)
    a = oracle.render(ps, nodes, refs, bounds, info=info)[0]
    L.oracle_set_perturb(1)
    try:
        b = oracle.render(ps, nodes, refs, bounds, info=info)[0]
    finally:
        L.oracle_set_perturb(0)
    return film_metrics(b, a)


# Cases that may take the "no worse than the reference algorithm's own one-ulp sensitivity" bar instead of the per-pixel one
# (pbrt-v1's fixed RAY_EPSILON makes them ill-conditioned under ANY other libm).  Every case records which bar it
# met in gpurun_out/parity_cases.json (also printed at the end of the session); a case NOT listed here that needs the
# fallback fails, so a regression cannot hide behind it.
FALLBACK_ALLOWED = {"sphere_path_soup", "quadrics_path", "mix:10", "mix:11", "mix:15"}
_CASES = {}


def record_case(name, metrics, fallback=False, sensitivity=None):
    import json, os
    _CASES[name] = dict(bar="one-ulp-sensitivity" if fallback else "per-pixel", frac=metrics.get("frac"), mean_l2=metrics.get("mean_l2"),
                        maxabs=metrics.get("maxabs"), sensitivity=sensitivity)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_cases.json"), "w") as f:
            json.dump(dict(fallback_allowed=sorted(FALLBACK_ALLOWED), fallback_used=sorted(k for k, v in _CASES.items() if v["bar"] != "per-pixel"),
                           cases=_CASES), f, indent=1)
    except OSError:
        pass
    if fallback:
        assert name in FALLBACK_ALLOWED, "case %r needed the one-ulp-sensitivity bar but is not on the allow-list: %r" % (name, _CASES[name])


def check_film(name, rgb, alpha, ref_rgb, ref_alpha, integrator, self_sensitivity=None):
    m = film_metrics(rgb, ref_rgb)
    if libm_bound(name, integrator):
        if not (m["frac"] >= 0.995 and m["mean_l2"] < 1e-4):
            s = self_sensitivity() if self_sensitivity else None
            assert s is not None and s["frac"] < 0.995, (name, m, s)          # only an ill-conditioned scene may miss the bar
            assert m["frac"] >= s["frac"] - 0.02 and m["mean_l2"] <= 2 * s["mean_l2"] + 1e-5, (name, m, s)
            record_case(name, m, True, s)
        else:
            record_case(name, m)
        assert (np.abs(alpha - ref_alpha) > 1e-5).mean() <= 0.005, name
    else:
        assert m["maxabs"] <= 1e-5, (name, m)
        assert np.abs(alpha - ref_alpha).max() <= 1e-5, name
        record_case(name, m)
    return m


@pytest.mark.parametrize("name", FILMS)
def test_device_film_matches_reference_golden(pkg, oracle, name):
    need_gpu(pkg)
    g = load_golden(name)
    ps = pkg.ParsedScene(text=g["scene"])
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    # ... and the TIMED kernels (COUNT = false: what bench.py measures -- the by-vertex path form among them) against the reference's film DIRECTLY, not only through
    # their equality with the counting twin (VERDICT r05 weak #1a): the flavour plan_schedule (rt_frame_plan.h) picks for this scene and the register-capped one it picks for large trees
    timed = []
    for env in ({}, dict(PBRT_HIP_HIGH_OCC="1")):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            ds.set_counting(False); ds.clear_film(); ds.render()
            timed.append(ds.film())
    ds.close()
    sens = (lambda: oracle_one_ulp_sensitivity(pkg, oracle, ps)) if ps.kdtree is not None and "grid" not in name else None
    check_film(name, rgb, alpha, g["rgb"], g["alpha"], ps.integrator, sens)
    for trgb, talpha in timed:
        check_film(name, trgb, talpha, g["rgb"], g["alpha"], ps.integrator, sens)
    st = g["stats"]
    tol = 0 if not libm_bound(name, ps.integrator) else max(4, int(2e-4 * st["closest_rays"]))
    assert abs(cnt["closest_rays"] - st["closest_rays"]) <= tol and abs(cnt["any_rays"] - st["any_rays"]) <= tol
    assert cnt["camera_rays"] == int(st["stats"]["Camera Rays Traced"]) and cnt["bad_samples"] == 0


@pytest.mark.parametrize("name", golden_names("probe_"))
def test_camera_and_trace_entry_points_against_probe_records(pkg, name):
    """rt_camera_rays, rt_trace_closest, rt_trace_any vs what the reference's camera / Scene::Intersect /
    Scene::IntersectP produced inside the probe integrator plugin."""
    need_gpu(pkg)
    g = load_golden(name)
    rec = g["records"]
    ps = pkg.ParsedScene(text=g["scene"].replace('SurfaceIntegrator "probe"', 'SurfaceIntegrator "whitted"'))
    ds = pkg.DeviceScene(ps)
    rays = ds.camera_rays(0, len(rec))
    assert len(rec) == ps.n_camera_samples
    if "lens" in name:      # thin lens: ConcentricSampleDisk calls cosf/sinf (device libm vs glibc differ in the last bit)
        assert np.abs(rays["o"] - rec[:, 0:3]).max() <= 1e-4
    else:
        assert np.array_equal(rays["o"], rec[:, 0:3])
    assert np.array_equal(rays["mint"], rec[:, 6])
    assert np.abs(rays["d"] - rec[:, 3:6]).max() <= 2e-7 and np.allclose(rays["maxt"], rec[:, 7], rtol=1e-6)
    # trace the REFERENCE's rays so that traversal is compared in isolation
    ref_rays = np.zeros(len(rec), pkg.RAY_DTYPE)
    ref_rays["o"] = rec[:, 0:3]; ref_rays["d"] = rec[:, 3:6]; ref_rays["mint"] = rec[:, 6]; ref_rays["maxt"] = rec[:, 7]
    hits = ds.trace_closest(ref_rays)
    hit = rec[:, 8] > 0
    assert np.array_equal(hits["prim"] >= 0, hit)
    assert np.array_equal(hits["t"][hit], rec[hit, 9])                       # bit-exact t
    assert np.array_equal((hits["b1"] + hits["b2"])[hit], rec[hit, 16]) and np.array_equal(hits["b2"][hit], rec[hit, 17])
    seg = np.zeros(int(hit.sum()), pkg.RAY_DTYPE)
    seg["o"] = rec[hit, 10:13]
    seg["d"] = (np.array([278, 540, 280], np.float32) - rec[hit, 10:13]).astype(np.float32)
    seg["mint"] = 1e-3; seg["maxt"] = np.float32(1.0) - np.float32(1e-3)
    assert np.array_equal(ds.trace_any(seg).astype(bool), rec[hit, 18] > 0)
    ds.close()


def test_trace_matches_oracle_on_random_rays_and_edge_cases(pkg, scenes, oracle):
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(xres=8, yres=8, soup_tris=20000, keyed=True))
    ds = pkg.DeviceScene(ps)
    nodes, refs = ds.accel_arrays()
    info = ds.accel_info()
    bounds = np.array(list(info.bounds), np.float32)
    rng = np.random.default_rng(5)
    n = 200000
    rays = np.zeros(n, pkg.RAY_DTYPE)
    rays["o"] = rng.uniform(-100, 650, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["d"] = d.astype(np.float32)
    rays["mint"] = 1e-3; rays["maxt"] = np.inf
    # edge cases: axis-parallel directions (1/0 = inf slabs), origin on a split plane / box face, zero-length and
    # inverted intervals, origins outside the tree bounds, rays that start on a triangle
    rays["d"][:3000] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 3000)] * rng.choice([-1, 1], (3000, 1)).astype(np.float32)
    rays["o"][3000:4000, 1] = 0.0
    rays["o"][4000:5000, 0] = bounds[0]
    rays["maxt"][5000:5500] = 1e-3
    rays["maxt"][5500:6000] = 0.0
    rays["o"][6000:7000] += 5000
    tv = ps.tri_verts()
    rays["o"][7000:8000] = tv[rng.integers(0, len(tv), 1000)].mean(1)
    hits = ds.trace_closest(rays)
    ref, oc = oracle.trace(ps, rays, False, nodes, refs, bounds)
    assert np.array_equal(hits["prim"], ref["prim"]) and np.array_equal(hits["t"], ref["t"])
    assert np.array_equal(hits["b1"], ref["b1"]) and np.array_equal(hits["b2"], ref["b2"])
    rays["maxt"] = np.where(np.isinf(rays["maxt"]), np.float32(300), rays["maxt"])
    occ = ds.trace_any(rays)
    refo, _ = oracle.trace(ps, rays, True, nodes, refs, bounds)
    assert np.array_equal(occ, refo)
    # empty input
    assert len(ds.trace_closest(rays[:0])) == 0
    ds.close()


@pytest.mark.parametrize("cfg", [
    dict(xres=160, yres=120, integrator="path", xsamples=2, ysamples=2, jitter=True, pixel_filter="mitchell", soup_tris=20000),
    dict(xres=200, yres=200, integrator="directlighting", xsamples=2, ysamples=2, jitter=True, soup_tris=50000),
    dict(xres=256, yres=256, integrator="whitted", soup_tris=3000, soup_materials=True),
    dict(xres=160, yres=160, integrator="directlighting", soup_tris=30000, accelerator="grid"),
    dict(xres=128, yres=128, integrator="path", sampler="lowdiscrepancy", pixelsamples=8, soup_tris=5000, accelerator="grid"),
])
def test_device_matches_oracle_on_larger_seeded_scenes(pkg, scenes, oracle, cfg):
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(keyed=True, **cfg))
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    nodes, refs = ds.accel_arrays()
    info = ds.accel_info()
    bounds = np.array(list(info.bounds), np.float32)
    ds.close()
    orgb, oalpha, _, ocnt = oracle.render(ps, nodes, refs, bounds, info=info)
    check_film(str(cfg), rgb, alpha, orgb, oalpha, ps.integrator)
    if ps.integrator != 2:
        # same rays, same tree, same order: identical work counters (the basis of the roofline's algorithmic bytes)
        for k in ("camera_rays", "closest_rays", "any_rays", "nodes_visited", "leaf_refs", "tri_tests"):
            assert cnt[k] == ocnt[k], (k, cnt[k], ocnt[k])
    else:
        for k in ("closest_rays", "any_rays", "nodes_visited", "tri_tests"):
            assert abs(cnt[k] - ocnt[k]) <= 3e-4 * ocnt[k] + 8, (k, cnt[k], ocnt[k])
    # pushes beyond the LDS ring (12 entries in the megakernel, 8 in the pipeline's trace kernel) spill to HBM: legal (and exercised
    # here), but must stay rare
    assert cnt["stack_overflows"] <= 2e-3 * cnt["nodes_visited"] + 1


@pytest.mark.parametrize("sampler", ["stratified", "lowdiscrepancy", "random", "medium"])
def test_direct_lighting_all_takes_any_number_of_lights(pkg, scenes, oracle, sampler):
    """DirectLightingIntegrator::RequestSamples asks for 2 x 2-D + 1 x 1-D per light without bound (directlighting.cpp:39-66).  Rounds 1-4 held the
    requests in the frame descriptor and refused the 21st light (VERDICT r04 missing #4); the per-light requests now live in HBM (DevFrame::light_dims).
    64 lights -- 63 point lights and the two-triangle ceiling emitter with 4 samples -- against the oracle, for every sampler, and in a medium (the queue
    pipeline's shade kernel reads the same table); the live reference where it travelled."""
    need_gpu(pkg)
    rng = np.random.default_rng(12)
    pts = "".join('LightSource "point" "point from" [%.1f %.1f %.1f] "color I" [%.0f %.0f %.0f]\n' % (*rng.uniform((40, 60, 40), (510, 520, 500)), *rng.uniform(2000, 9000, 3))
                  for _ in range(63))
    kw = dict(xres=40, yres=40, integrator="directlighting", soup_tris=2000, keyed=True, world_kwargs=dict(extra=pts, light_nsamples=4))
    if sampler == "lowdiscrepancy":
        kw.update(sampler="lowdiscrepancy", pixelsamples=4)
    elif sampler == "random":
        kw.update(sampler="random", xsamples=2, ysamples=2)
    else:
        kw.update(xsamples=2, ysamples=2, jitter=True)
    if sampler == "medium":
        kw.update(volume_integrator='"single" "float stepsize" [60]')
        kw["world_kwargs"]["volume"] = '"float g" [0]'
    text = scenes.cornell_scene(**kw)
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    nodes, refs = ds.accel_arrays()
    info = ds.accel_info()
    bounds = np.array(list(info.bounds), np.float32)
    ds.close()
    orgb, oalpha, _, ocnt = oracle.render(ps, nodes, refs, bounds, info=info)
    check_film("all64:" + sampler, rgb, alpha, orgb, oalpha, 1)
    for k in ("camera_rays", "closest_rays", "any_rays"):
        assert cnt[k] == ocnt[k], (k, cnt[k], ocnt[k])
    assert cnt["any_rays"] >= 60 * cnt["camera_rays"] * 0.5          # every lit vertex casts a shadow ray per point light
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(scenes.cornell_scene(count=True, **kw), keyed=True)
    except FileNotFoundError:
        return
    check_film("all64 live:" + sampler, rgb, alpha, ref_rgb, ref_alpha, 1)


def test_live_reference_when_present(pkg, scenes):
    """The compiled reference travels to the GPU box (oracle/_ref): render one scene with both, live."""
    need_gpu(pkg)
    text = scenes.cornell_scene(xres=96, yres=96, integrator="path", xsamples=3, ysamples=3, jitter=True, soup_tris=4000,
                                keyed=True, count=True, seed=11)
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(text, keyed=True)
    except FileNotFoundError:
        pytest.skip("oracle/_ref not on this box")
    rgb, alpha, cnt, _ = pkg.render_text(text)
    check_film("live", rgb, alpha, ref_rgb, ref_alpha, 2)


def test_shards_on_one_gpu_sum_to_the_full_film(pkg, scenes):
    """Multi-GPU partition (tiles round-robin, film sum) exercised on one device: 3 shards accumulated into the
    same bound film == one shard, up to float summation order."""
    need_gpu(pkg)
    text = scenes.cornell_scene(xres=96, yres=64, integrator="path", xsamples=2, ysamples=2, jitter=True, pixel_filter="mitchell", keyed=True)
    ps = pkg.ParsedScene(text=text)
    ds = pkg.DeviceScene(ps); ds.render(); full = ds.film_accum(); c1 = ds.counters(); ds.close()
    ps2 = pkg.ParsedScene(text=text)
    ds2 = pkg.DeviceScene(ps2); ds2.bind_film()
    for r in range(3):
        ps2.set_shard(r, 3, 16)
        ds2.render()
    parts = ds2.film_accum(); c3 = ds2.counters(); ds2.close()
    assert np.allclose(parts, full, rtol=2e-5, atol=2e-6)
    assert c3["camera_rays"] == c1["camera_rays"] and c3["closest_rays"] == c1["closest_rays"]


GATHER_CASES = {
    # filter reach 2 (mitchell / gaussian / triangle), reach 1 (box), odd film sizes, 1 / 6 / 16 samples per pixel (6: not a multiple of the
    # accumulation pass's batch), a crop window, a lens, the low-discrepancy sampler
    "mitchell_4spp": dict(xres=75, yres=53, integrator="path", xsamples=2, ysamples=2, jitter=True, pixel_filter="mitchell"),
    "gaussian_6spp": dict(xres=64, yres=40, integrator="directlighting", xsamples=3, ysamples=2, jitter=True, pixel_filter="gaussian"),
    "triangle_1spp": dict(xres=33, yres=130, integrator="whitted", xsamples=1, ysamples=1, jitter=True, pixel_filter="triangle"),
    "box_16spp_crop": dict(xres=90, yres=70, integrator="path", xsamples=4, ysamples=4, jitter=True, pixel_filter="box", crop=(0.21, 0.83, 0.13, 0.9)),
    "box_wide": dict(xres=48, yres=48, integrator="whitted", xsamples=2, ysamples=1, jitter=True, pixel_filter="box", filter_params='"float xwidth" [1.3] "float ywidth" [1.3]'),
    "mitchell_ld8_lens": dict(xres=40, yres=70, integrator="path", sampler="lowdiscrepancy", pixelsamples=8, pixel_filter="mitchell", lensradius=6.0, focaldistance=900.0),
    "sinc_reach4": dict(xres=50, yres=34, integrator="whitted", xsamples=2, ysamples=2, jitter=True, pixel_filter="sinc"),
    "mitchell_128spp": dict(xres=20, yres=14, integrator="whitted", xsamples=16, ysamples=8, jitter=True, pixel_filter="mitchell"),      # 32 records per lane and row: beyond the lookahead
    "gaussian_256spp": dict(xres=18, yres=12, integrator="whitted", xsamples=16, ysamples=16, jitter=True, pixel_filter="gaussian"),     # a sample row does not fit 64 KB of LDS: no slot kernel
    "gaussian_unequal": dict(xres=44, yres=36, integrator="whitted", xsamples=2, ysamples=2, jitter=True, pixel_filter="gaussian", filter_params='"float xwidth" [2.7] "float ywidth" [1.2]'),
}


GATHER_REACH = {"mitchell_4spp": (2, 2), "gaussian_6spp": (2, 2), "triangle_1spp": (2, 2), "box_16spp_crop": (1, 1), "box_wide": (1, 1),
                "mitchell_ld8_lens": (2, 2), "sinc_reach4": (4, 4), "gaussian_unequal": (3, 1), "mitchell_128spp": (2, 2), "gaussian_256spp": (2, 2)}


@pytest.mark.parametrize("name", sorted(GATHER_CASES))
def test_the_three_film_gathers_agree_bit_for_bit(pkg, scenes, name, monkeypatch):
    """ImageFilm::AddSample runs as one of three kernels (rt_film.hip): film_slot_kernel (filters reaching 1 or 2 pixels both ways: one
    pixel per lane, sample rows staged in LDS with the footprint tests and table indices precomputed per record), film_march_kernel (up
    to 3 rows: a lane marches down a pixel column) and the staged film_gather_kernel (anything).  All three must produce the SAME bits --
    the staged one is the kernel the reference-film fixtures were pinned with in rounds 1-2 -- whatever the strip height, on one shard
    and on the 1-D / 2-D tiles of a 3-rank partition."""
    need_gpu(pkg)
    text = scenes.cornell_scene(keyed=True, seed=11, soup_tris=200, **GATHER_CASES[name])
    ps = pkg.ParsedScene(text=text)
    ds = pkg.DeviceScene(ps); ds.bind_film()
    reach = GATHER_REACH[name]                     # floor(filter width + .5) in x and y
    kinds = ["staged"] + (["march"] if reach[1] <= 3 else []) + (["slot"] if reach[0] == reach[1] and reach[0] in (1, 2) and name != "gaussian_256spp" else [])
    shards = [(0, 1, 1), (1, 3, 16), (2, 3, (16, 8))]
    for shard in shards:
        ps.set_shard(*shard)
        ref = None
        for kind in kinds:
            for rows in (None, "1", "3", "7", "1000"):
                with pytest.MonkeyPatch.context() as mp:
                    mp.setenv("PBRT_HIP_GATHER", kind)
                    if rows: mp.setenv("PBRT_HIP_GATHER_ROWS", rows)
                    ds.clear_film(); ds.render()
                got = ds.film_accum()
                if ref is None:
                    ref = got
                    assert np.isfinite(ref).all() and ref[4].max() > 0
                assert np.array_equal(got, ref), (name, shard, kind, rows, float(np.abs(got - ref).max()))
                if kind == "staged": break
    # the default choice, and a loud refusal of a kernel that cannot serve the filter
    ps.set_shard(0, 1, 1)
    ds.clear_film(); ds.render(); base = ds.film_accum()
    for kind in ("slot", "march"):
        if kind not in kinds:
            monkeypatch.setenv("PBRT_HIP_GATHER", kind)
            with pytest.raises(pkg.RtError):
                ds.render()
            monkeypatch.delenv("PBRT_HIP_GATHER")
    monkeypatch.setenv("PBRT_HIP_GATHER", "staged")
    ds.clear_film(); ds.render()
    assert np.array_equal(ds.film_accum(), base)
    ds.close()


def test_full_size_properties(pkg, scenes):
    """BASELINE configs[1] at full size (1024x1024 @ 64 spp, path maxdepth 5): properties that need no oracle.
      * every camera sample of the extent is rendered exactly once: sum of filter weights per pixel is the same
        closed form the reference's AddSample would produce (box filter, unjittered strata: 64 per interior pixel);
      * linearity: radiance is linear in the emitter's L -- doubling L doubles every accumulator;
      * no NaN/negative/inf samples; alpha in [0,1]; ray counts reproducible run to run;
      * determinism and flavours: two renders of the counting twin and one of the timed kernel give the bit-identical film."""
    need_gpu(pkg)
    kw = dict(xres=1024, yres=1024, integrator="path", xsamples=8, ysamples=8, jitter=False, pixel_filter="box", keyed=True)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(**kw))
    ds = pkg.DeviceScene(ps); ds.render(); a = ds.film_accum(); ca = ds.counters()
    ds.reset_counters(); ds.clear_film(); ds.render(); a2 = ds.film_accum(); ca2 = ds.counters()
    # the TIMED flavour (what bench.py measures on C2: the register-capped kernel, batched rounds) gives the counting twin's film bit for bit
    ds.set_counting(False); ds.clear_film(); ds.render(); a3 = ds.film_accum(); ds.close()
    assert ca["camera_rays"] == 1025 * 1025 * 64 and ca["bad_samples"] == 0 and ca == ca2
    assert np.array_equal(a, a2), "two renders of the counting twin differ"
    assert np.array_equal(a, a3), "the timed kernel's film differs from its counting twin's"
    assert np.all(a[4][1:-1, 1:-1] == 64.0)
    assert np.isfinite(a).all() and a[:3].min() >= 0 and np.all(a[3] <= a[4] + 1e-3)
    ps2 = pkg.ParsedScene(text=scenes.cornell_scene(world_kwargs=dict(light_L=(34, 24, 8)), **kw))
    ds2 = pkg.DeviceScene(ps2); ds2.render(); b = ds2.film_accum(); cb = ds2.counters(); ds2.close()
    assert cb["closest_rays"] == ca["closest_rays"] and cb["any_rays"] == ca["any_rays"]
    assert np.allclose(b[:3], 2 * a[:3], rtol=1e-4, atol=1e-4) and np.array_equal(b[4], a[4])


@pytest.mark.parametrize("k", range(10))
def test_by_vertex_path_kernels_equal_the_per_ray_twins_on_random_scenes(pkg, scenes, k, monkeypatch):
    """Round 5: the timed path kernels run a vertex at a time (rt_integrate.h advance_pass_byv: the MIS and continuation rays are started inside the traversal loop, the two
    EstimateDirect terms are added a vertex later); the counting twins still run ray by ray.  Seeded random scenes -- soup size, material mix, path depth 1 .. 10, the three
    samplers, kd-tree and grid, a lens, several lights incl. none and delta only, the register-capped flavour forced on tiny trees -- must give bit-identical films, and the
    timed kernel the same film twice."""
    need_gpu(pkg)
    rng = np.random.default_rng(500 + k)
    kw = dict(xres=int(rng.integers(24, 72)), yres=int(rng.integers(24, 72)), integrator="path", maxdepth=int(rng.integers(1, 11)), keyed=True,
              soup_tris=int(rng.choice([0, 300, 3000, 30000])), soup_materials=bool(rng.integers(0, 2)), accelerator=str(rng.choice(["kdtree", "kdtree", "grid"])),
              pixel_filter=str(rng.choice(["box", "mitchell", "gaussian"])), seed=int(rng.integers(0, 1000)))
    sampler = str(rng.choice(["stratified", "lowdiscrepancy", "random"]))
    if sampler == "lowdiscrepancy":
        kw.update(sampler=sampler, pixelsamples=int(rng.choice([1, 4, 8])))
    else:
        kw.update(sampler=sampler, xsamples=int(rng.integers(1, 4)), ysamples=int(rng.integers(1, 3)))
        if sampler == "stratified":
            kw["jitter"] = bool(rng.integers(0, 2))
    if rng.integers(0, 3) == 0:
        kw.update(lensradius=float(rng.uniform(1, 8)), focaldistance=float(rng.uniform(500, 1100)))
    lights = int(rng.integers(0, 4))                                   # 0: the ceiling emitter only, 1: + a point light, 2: a point light only, 3: no light at all
    wk = dict(mirror_quad=bool(rng.integers(0, 2)))
    if lights == 1: wk.update(point_light=True)
    if lights == 2: wk.update(point_light=True, area_light=False)
    if lights == 3: wk.update(area_light=False)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(world_kwargs=wk, **kw))
    assert ps.valid and ps.errors == 0, kw
    monkeypatch.setenv("PBRT_HIP_HIGH_OCC", "1")                       # the flavour the by-vertex form lives in, also on tiny trees
    ds = pkg.DeviceScene(ps)
    ds.set_counting(True); ds.render(); twin = ds.film_accum(); cnt = ds.counters()
    ds.set_counting(False); ds.clear_film(); ds.render(); a = ds.film_accum(); st = ds.last_stats()
    ds.clear_film(); ds.render(); b = ds.film_accum()
    ds.close()
    assert st["pipeline"] == 0
    assert np.array_equal(a, twin), ("by vertex != per ray", kw, wk)
    assert np.array_equal(a, b), ("two renders of the timed kernel differ", kw)
    assert cnt["camera_rays"] > 0 and cnt["bad_samples"] == 0


@pytest.mark.parametrize("cfg", [
    dict(xres=64, yres=64, integrator="path", maxdepth=5, xsamples=2, ysamples=2, jitter=True, keyed=True),                                  # Cornell alone: 14 triangles, leaves of up to 9
    dict(xres=64, yres=48, integrator="directlighting", xsamples=2, ysamples=2, jitter=True, keyed=True, soup_tris=3000, soup_materials=True),
    dict(xres=64, yres=48, integrator="path", maxdepth=6, xsamples=2, ysamples=1, keyed=True, soup_tris=40000, soup_materials=True,
         accel_params='"integer maxprims" [8] "integer intersectcost" [2] "float emptybonus" [0]'),                                        # fat leaves: long entry lists
    dict(xres=48, yres=48, integrator="whitted", xsamples=1, ysamples=1, keyed=True, soup_tris=20000, soup_materials=True,
         volume_integrator='"single" "float stepsize" [40]', world_kwargs=dict(volume='"float g" [.2]')),                                  # the march kernel's traversal loop
])
def test_leaf_layout_forms_agree(pkg, scenes, cfg, monkeypatch):
    """Round 6: a leaf's primitives are reached through ENTRIES into one record per primitive (rt_traverse.h RT_LE_*: first inline, second in the node's other word, the rest
    in a list that is requested together with the record before it), or, on scenes of a few thousand references, through RUNS of consecutive records.  Which form a scene gets
    is a host-side choice (rt_scene.hip leaf_cursor_layout) that must never show: the same frame under the default, under entries forced (PBRT_HIP_LEAF_RUNS=0: Cornell's leaves of
    nine through the list path), under runs forced (=1) and under entries over per-reference copies (PBRT_HIP_LEAF_COPIES) -- films and EVERY counter equal, counting twin and timed
    kernels (both megakernel flavours and the queue pipeline's trace kernel) alike, with the device-filled records verified against the host fill."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(**cfg))
    assert ps.valid and ps.errors == 0
    monkeypatch.setenv("PBRT_HIP_VERIFY_DERIVED", "1")
    base = None
    for env in ({}, dict(PBRT_HIP_LEAF_RUNS="0"), dict(PBRT_HIP_LEAF_RUNS="1"), dict(PBRT_HIP_LEAF_RUNS="0", PBRT_HIP_LEAF_COPIES="1")):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            ds = pkg.DeviceScene(ps)                          # (the layout knobs are read by rt_scene_create)
        ds.render(); acc = ds.film_accum(); cnt = ds.counters()
        for flavour in (dict(PBRT_HIP_HIGH_OCC="0"), dict(PBRT_HIP_HIGH_OCC="1"), dict(PBRT_HIP_PIPELINE="1")):
            with pytest.MonkeyPatch.context() as mp:
                for k, v in flavour.items():
                    mp.setenv(k, v)
                ds.set_counting(False); ds.clear_film(); ds.render()
                assert np.array_equal(ds.film_accum(), acc), (env, flavour)
        ds.close()
        if base is None:
            base = (acc, cnt)
            continue
        assert np.array_equal(acc, base[0]), env
        assert cnt == base[1], (env, cnt, base[1])


def test_errors_are_loud(pkg, scenes):
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(xres=8, yres=8))
    ds = pkg.DeviceScene(ps)
    import ctypes as C
    assert pkg.hip_lib().rt_film_bind(ds._s, None, 4, 4) == 0          # a film of the wrong size
    ds._film_bound = True
    with pytest.raises(pkg.RtError) as e:
        ds.render()
    assert "film size" in str(e.value)
    assert pkg.hip_lib().rt_render(ds._s, None) < 0 and pkg.hip_lib().rt_render(None, ps.render_desc) < 0
    ds.close()


# PBRT_HIP_PIPE_VERTEX left at its default, the per-ray form forced, and so few slots that every slot is refilled many times
FLAVOUR_PIPELINE_ENVS = (dict(PBRT_HIP_PIPELINE="1"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="0"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_SLOTS="512"))


@pytest.mark.parametrize("name", ["path_soup2k", "direct_soup5k_seed7", "whitted_glass_mirror", "grid_path_soup3k_eager", "vol_single_path_grid",
                                  "plastic_path", "sphere_whitted", "qlight_path", "path_jitter_mitchell_4spp"])
def test_timed_kernels_produce_the_same_film_as_the_counting_twins(pkg, name):
    """bench.py times the COUNT=false kernels (and, on large scenes, the register-capped high-occupancy flavour); the parity
    tests above render with the counting twins.  Scheduling never changes a sample's arithmetic and the film gather is
    deterministic, so every flavour must give the bit-identical film.
    The queue pipeline: by vertex (rt_pipe_vertex.h: path integrator without a medium; every other frame takes the per-ray form), per
    ray, and with so few slots that every slot is refilled many times; its counting twin must also reproduce the ray counts."""
    need_gpu(pkg)
    ds = pkg.DeviceScene(pkg.ParsedScene(text=load_golden(name)["scene"]))
    ref, _ = assert_flavours_agree(ds, name, FLAVOUR_PIPELINE_ENVS, expect_pipeline=None)
    ds.set_counting(True); ds.clear_film(); ds.render()                 # and the flavour that rt_render chooses for the frame by itself
    got = ds.film_accum()
    ds.close()
    assert np.array_equal(got, ref), (name, "default", float(np.abs(got - ref).max()))


def _random_scene(scenes, rng):
    """A Cornell box with a random mix of everything the path supports: materials, quadrics (some emitting), delta lights,
    camera, sampler, integrator, accelerator, optional medium."""
    mats = ['Material "matte" "color Kd" [%.2f %.2f %.2f] "float sigma" [%d]' % (*rng.uniform(.1, .8, 3), rng.choice([0, 0, 30])),
            'Material "plastic" "color Kd" [%.2f %.2f %.2f] "float roughness" [%.2f]' % (*rng.uniform(.1, .7, 3), rng.uniform(.05, .4)),
            'Material "uber" "color Kd" [%.2f %.2f %.2f] "color Kr" [.2 .2 .2] "color opacity" [%.1f %.1f %.1f]' % (*rng.uniform(.1, .7, 3), *rng.choice([1.0, 0.7], 3)),
            'Material "mirror"', 'Material "glass" "float index" [%.2f]' % rng.uniform(1.2, 1.7)]
    shapes = ['Shape "sphere" "float radius" [%d]' % rng.integers(30, 80),
              'Shape "sphere" "float radius" [60] "float zmin" [-30] "float zmax" [45] "float phimax" [%d]' % rng.integers(180, 360),
              'Shape "cylinder" "float radius" [%d] "float zmin" [-50] "float zmax" [60]' % rng.integers(20, 60),
              'Shape "disk" "float radius" [%d] "float innerradius" [%d]' % (rng.integers(50, 90), rng.choice([0, 20])),
              'Shape "cone" "float radius" [50] "float height" [%d]' % rng.integers(60, 140),
              'Shape "paraboloid" "float radius" [50] "float zmax" [%d]' % rng.integers(60, 120),
              'Shape "hyperboloid" "point p1" [50 0 -40] "point p2" [30 30 50]']
    extra = []
    for _ in range(int(rng.integers(1, 4))):
        emit = rng.random() < 0.3
        shp = shapes[int(rng.integers(0, 4 if emit else len(shapes)))]
        extra.append("AttributeBegin\n%s%s\nTranslate %d %d %d\nRotate %d %d %d %d\n%s\nAttributeEnd\n" % (
            'AreaLightSource "area" "color L" [%d %d %d]\n' % tuple(rng.integers(3, 12, 3)) if emit else "", mats[int(rng.integers(0, len(mats)))],
            *rng.integers(100, 450, 3), rng.integers(0, 180), *rng.integers(0, 2, 2), 1, shp))
    if rng.random() < 0.5:
        extra.append('LightSource "spot" "point from" [278 500 100] "point to" [%d 0 %d] "color I" [300000 300000 300000]\n' % tuple(rng.integers(100, 450, 2)))
    if rng.random() < 0.3:
        extra.append('LightSource "distant" "point from" [%.1f 1 %.1f] "point to" [0 0 0] "color L" [1 1 1]\n' % tuple(rng.uniform(-1, 1, 2)))
    kw = dict(xres=int(rng.integers(24, 48)), yres=int(rng.integers(24, 48)), integrator=str(rng.choice(["whitted", "directlighting", "path"])),
              accelerator=str(rng.choice(["kdtree", "grid"])), jitter=bool(rng.random() < 0.5), soup_tris=int(rng.choice([0, 0, 300, 3000])),
              pixel_filter=str(rng.choice(["box", "mitchell", "gaussian", "triangle"])), keyed=True, seed=int(rng.integers(0, 1000)))
    if rng.random() < 0.3:
        kw.update(sampler="lowdiscrepancy", pixelsamples=int(rng.choice([2, 4, 8])))
    else:
        kw.update(xsamples=int(rng.integers(1, 3)), ysamples=int(rng.integers(1, 3)))
    world = dict(extra="".join(extra), area_light=bool(rng.random() < 0.7), point_light=bool(rng.random() < 0.3))
    if rng.random() < 0.25:
        world["volume"] = '"float g" [%.1f]' % rng.uniform(-.3, .5)
        kw["volume_integrator"] = '"%s" "float stepsize" [%d]' % (rng.choice(["single", "emission"]), rng.integers(40, 90))
    text = scenes.cornell_scene(world_kwargs=world, **kw)
    cam = rng.random()
    if cam < 0.15:
        text = text.replace('Camera "perspective" "float fov" [39.3]', 'Camera "orthographic" "float screenwindow" [-300 300 -290 290]')
    elif cam < 0.3:
        text = text.replace("LookAt 278 273 -800  278 273 0  0 1 0", "LookAt 278 273 200  278 273 600  0 1 0").replace(
            'Camera "perspective" "float fov" [39.3]', 'Camera "environment"')
    return text


@pytest.mark.parametrize("k", range(16))
def test_randomized_feature_mixes_against_the_oracle(pkg, scenes, oracle, k):
    """Seeded random combinations of every supported plugin (materials, quadrics incl. emitters, lights, cameras, samplers,
    integrators, accelerators, medium), device against the CPU restatement (itself pinned bit-exactly on the reference's
    films): catches interactions no hand-written fixture covers."""
    need_gpu(pkg)
    text = _random_scene(scenes, np.random.default_rng(1000 + k))
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0, text
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    nodes, refs = ds.accel_arrays()
    info = ds.accel_info()
    bounds = np.array(list(info.bounds), np.float32)
    ds.close()
    orgb, oalpha, _, ocnt = oracle.render(ps, nodes, refs, bounds, info=info)
    assert cnt["camera_rays"] == ocnt["camera_rays"] and cnt["bad_samples"] == ocnt["bad_samples"]
    m = film_metrics(rgb, orgb)
    if m["frac"] >= 0.99 and m["mean_l2"] < 2e-4:
        record_case("mix:%d" % k, m)
    else:
        # an ill-conditioned mix (see oracle_one_ulp_sensitivity): pixels cannot be compared one by one under another libm.  The
        # device must then be about as far from the oracle as the oracle is from its one-ulp twin (the device differs in every
        # libm function, the twin only in one cosf) and must carry the same energy.
        s = oracle_one_ulp_sensitivity(pkg, oracle, ps, (nodes, refs, bounds, info))
        assert s["frac"] < 0.995, (k, m, s)
        assert m["frac"] >= 0.75 * s["frac"] - 0.02, (k, m, s)
        assert abs(float(rgb.mean()) - float(orgb.mean())) <= 0.05 * float(orgb.mean()) + 1e-3, (k, float(rgb.mean()), float(orgb.mean()))
        record_case("mix:%d" % k, m, True, s)


def _converged_variant(text, seed):
    """The same scene at 32x the samples per pixel (another keyed-RNG seed for the second estimate)."""
    import re
    def mul(m, k):
        return '"integer %s" [%d]' % (m.group(1), int(m.group(2)) * k)
    text = re.sub(r'"integer (xsamples)" \[(\d+)\]', lambda m: mul(m, 8), text)
    text = re.sub(r'"integer (ysamples)" \[(\d+)\]', lambda m: mul(m, 4), text)
    text = re.sub(r'"integer (pixelsamples)" \[(\d+)\]', lambda m: mul(m, 32), text)
    text, n = re.subn(r'"integer seed" \[\d+\]', '"integer seed" [%d]' % seed, text)
    assert n == 1
    return text


@pytest.mark.parametrize("case", sorted(FALLBACK_ALLOWED))
def test_allow_listed_cases_converge_to_the_oracle(pkg, scenes, oracle, case):
    """The five ill-conditioned cases cannot be compared pixel by pixel under another libm (see oracle_one_ulp_sensitivity): one
    flipped last bit sends a whole path elsewhere.  What must still hold is that the device computes the same INTEGRAL.  Each case is
    rendered at 32x its samples per pixel: the oracle twice (seeds A and B), the device once (seed A), and compared on 4x4-pixel block
    means.  d_ref = oracle_A - oracle_B is pure Monte-Carlo noise; d_dev = device_A - oracle_B must look like it:
      * rms(d_dev) <= 1.25 rms(d_ref)            (no extra error anywhere),
      * |mean(device_A - oracle_A)| <= 4 rms(d_ref) / sqrt(#blocks)   (no energy bias),
      * every block within max(6 rms(d_ref), 1.5 max|d_ref|) + 3 % of its value (no local bias beyond the noise's own tail)."""
    need_gpu(pkg)
    if case.startswith("mix:"):
        base = _random_scene(scenes, np.random.default_rng(1000 + int(case[4:])))
    else:
        base = str(load_golden(case)["scene"])
    films = {}
    for tag, seed, dev in (("oA", 11, False), ("oB", 23, False), ("dA", 11, True)):
        ps = pkg.ParsedScene(text=_converged_variant(base, seed))
        assert ps.valid and ps.errors == 0
        ds = pkg.DeviceScene(ps)
        if dev:
            ds.set_counting(False); ds.render(); films[tag] = ds.film()[0]
        else:
            nodes, refs = ds.accel_arrays(); info = ds.accel_info()
            films[tag] = oracle.render(ps, nodes, refs, np.array(list(info.bounds), np.float32), info=info)[0]
        ds.close()
    def blocks(img):
        h, w = img.shape[0] // 4 * 4, img.shape[1] // 4 * 4
        return img[:h, :w].reshape(h // 4, 4, w // 4, 4, 3).mean(axis=(1, 3))
    bo_a, bo_b, bd = blocks(films["oA"]), blocks(films["oB"]), blocks(films["dA"])
    d_ref, d_dev = bo_a - bo_b, bd - bo_b
    rms_ref, rms_dev = float(np.sqrt((d_ref ** 2).mean())), float(np.sqrt((d_dev ** 2).mean()))
    nb = d_ref.size
    m = dict(rms_ref=rms_ref, rms_dev=rms_dev, mean_dev=float(d_dev.mean()), mean_ref=float(d_ref.mean()), level=float(bo_b.mean()), blocks=nb)
    record_case("converged:" + case, dict(frac=1.0, mean_l2=rms_dev, maxabs=float(np.abs(d_dev).max())), False, m)
    assert rms_ref > 0 and rms_dev <= 1.25 * rms_ref + 1e-4, m
    # energy: with the SAME seed the two differ only on the few paths a last bit flips, so their means agree far inside the noise of either
    # (the oracle's own two seeds can differ by more than that: heavy tails)
    assert abs(m["mean_dev"] - m["mean_ref"]) <= 4 * rms_ref / np.sqrt(nb) + 1e-4, m
    # Monte-Carlo noise of these scenes is heavy-tailed (a block that caught a caustic path): the oracle's own worst block sets the scale
    worst_ref = float(np.abs(d_ref).max())
    assert np.all(np.abs(d_dev) <= max(6 * rms_ref, 1.5 * worst_ref) + 0.03 * np.abs(bo_b) + 1e-3), (m, float(np.abs(d_dev).max()), worst_ref)


def test_film_into_caller_buffers(pkg, scenes):
    """rt_film_resolve into caller-provided (e.g. page-locked, reused) buffers gives the film it allocates itself; wrong shapes
    are rejected on the host side."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=scenes.cornell_scene(xres=40, yres=24, integrator="directlighting", keyed=True))
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    out = (np.full((24, 40, 3), -1, np.float32), np.full((24, 40), -1, np.float32))
    r2, a2 = ds.film(out=out)
    assert r2 is out[0] and a2 is out[1] and np.array_equal(r2, rgb) and np.array_equal(a2, alpha)
    with pytest.raises(ValueError):
        ds.film(out=(np.zeros((24, 40, 4), np.float32), out[1]))
    ds.close()
