"""Medium queries at caller-supplied rays and points on the GPU: DeviceScene.medium (rt_medium_device) against the reference's own answers per
query (the four fixtures of tests/golden/medium/, made by the reference-side plugin tests/golden/medium_probe.cpp), the offsets a homogeneous
region ignores, tr = exp(-tau), next-event estimation through a homogeneous and through an exponential medium composed into a frame bit for bit,
lv as a frame's Lv, the launch shapes, the march guard, a scene without a medium, the refusals, and that a query is no frame."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
# torch BEFORE the device library is loaded, as bench.py does (see tests/test_gpu_rays.py)
import torch

import analytic_cases as A
import bsdf_forms as B
import medium_cases as MC
from conftest import GOLDEN, load_golden
from gpu_checks import need_gpu

pytestmark = pytest.mark.gpu

INPUTS = ("p", "w", "wp", "rays", "u", "u_scatter", "rng")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def open_scene(pkg, text):
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    return ps, pkg.DeviceScene(ps)


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(GOLDEN, "medium", name + ".npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the float64 forms on the fixture (for the exclusion mask): computed once per session"""
    fx = fixture(name)
    return MC.evaluate(name, fx, int(fx["seed"]))


def inputs(fx, rows=slice(None), skip=()):
    return {k: dev(fx[k][rows]) for k in INPUTS if k not in skip}


def ask(ds, fx, rows=slice(None)):
    """every output of the fixture's layout: one call with u (tau, tr with a sample, lv and its draws), one without (Scene::Transmittance and its draw)"""
    got = host(ds.medium(**inputs(fx, rows)))
    null = host(ds.medium(**inputs(fx, rows, skip=("u",)), fields=("tr", "draws")))
    got["draws_lv"], got["tr_null"], got["draws_tr"] = got.pop("draws"), null["tr"], null["draws"]
    return got


# ---------------------------------------------------------------------------------------------- 1. the reference's answers, per query
@pytest.mark.parametrize("name", list(MC.CASES))
def test_every_output_agrees_with_the_reference_per_query(pkg, name):
    """every float output within 4 x max(ref_err(case, output), the median ref_err of that output over the cases) of the reference's value in the
    measure of bsdf_forms.query_error -- ref_err being the reference's own largest error against the float64 forms, stored in the fixtures --; hit
    and the draws equal the reference's.  Only the queries the forms' rule leaves out (at most 3 %) are not compared."""
    need_gpu(pkg)
    fx, w = fixture(name), expected(name)
    inc = ~w["excluded"]
    assert w["excluded"].mean() <= A.BAND_CAP
    median = np.median([fixture(c)["ref_err"] for c in MC.CASES], axis=0)
    ps, ds = open_scene(pkg, MC.product_text(fx["scene"]))
    got = ask(ds, fx)
    ds.close()
    ans = fx["answers"]
    failed = []
    assert not got["status"][inc].any()
    for i, k in enumerate(MC.OUTPUTS):
        bar = A.BAR_FACTOR * max(float(fx["ref_err"][i]), float(median[i]))
        e = B.query_error(got[k], MC.answer(ans, k), inc)[inc].max()
        differ = int((bits(got[k][inc]) != bits(MC.answer(ans, k)[inc])).reshape(int(inc.sum()), -1).any(-1).sum())
        print("MEDIUM-REF %s %-8s e %.3g bar %.3g (ref_err %.3g, median %.3g), %d of %d differ in a bit" % (name, k, e, bar, fx["ref_err"][i], median[i], differ, int(inc.sum())))
        if not e <= bar:
            failed.append((k, float(e), bar))
    for k in MC.DISCRETE:
        differ = int((got[k][inc] != MC.answer(ans, k)[inc]).sum())
        print("MEDIUM-REF %s %-8s differing %d of %d" % (name, k, differ, int(inc.sum())))
        if differ:
            failed.append((k, differ))
    assert not failed, (name, failed)


# ---------------------------------------------------------------------------------------------- 2. a homogeneous region ignores the offsets
def test_offsets_do_not_reach_a_homogeneous_region(pkg):
    """tau and tr are bitwise the same for any u, any rng and the form without u, whose draw is still made (draws == 1)"""
    need_gpu(pkg)
    fx = fixture("homogeneous_ctm")
    ps, ds = open_scene(pkg, MC.product_text(fx["scene"]))
    rays = dev(fx["rays"])
    n = len(fx["rays"])
    rs = np.random.RandomState(3)
    base = host(ds.medium(rays=rays, u=dev(fx["u"]), rng=dev(fx["rng"]), fields=("tau", "tr", "draws")))
    other = host(ds.medium(rays=rays, u=dev(rs.uniform(size=n).astype(np.float32)), rng=dev(rs.randint(0, 1 << 30, (n, 2)).astype(np.uint32)), fields=("tau", "tr", "draws")))
    null = host(ds.medium(rays=rays, rng=dev(fx["rng"]), fields=("tr", "draws")))
    null0 = host(ds.medium(rays=rays, fields=("tr", "draws")))
    ds.close()
    assert base["tau"].any(-1).mean() > .3
    assert np.array_equal(bits(base["tau"]), bits(other["tau"])) and np.array_equal(bits(base["tr"]), bits(other["tr"]))
    assert np.array_equal(bits(base["tr"]), bits(null["tr"])) and np.array_equal(bits(base["tr"]), bits(null0["tr"]))
    assert not base["draws"].any() and not other["draws"].any() and (null["draws"] == 1).all() and (null0["draws"] == 1).all()


# ---------------------------------------------------------------------------------------------- 3. tr is exp of tau
@pytest.mark.parametrize("name", list(MC.CASES))
def test_tr_with_a_sample_is_exp_of_the_calls_own_tau(pkg, name):
    """tr asked alone, with u, is bitwise the tr of the call that also returns tau, and that tr is exp(-tau) of the returned tau: the float32
    exponential of a float32 argument, two units in the last place allowed for the device's expf against the host's"""
    need_gpu(pkg)
    fx = fixture(name)
    ps, ds = open_scene(pkg, MC.product_text(fx["scene"]))
    both = host(ds.medium(rays=dev(fx["rays"]), u=dev(fx["u"]), fields=("tau", "tr")))
    alone = host(ds.medium(rays=dev(fx["rays"]), u=dev(fx["u"]), fields=("tr",)))
    ds.close()
    assert np.array_equal(bits(both["tr"]), bits(alone["tr"]))
    want = np.exp(-both["tau"].astype(np.float64))
    assert (np.abs(both["tr"] - want) <= 2 * np.spacing(want.astype(np.float32))).all()
    assert both["tau"].any(-1).mean() > .3


# ---------------------------------------------------------------------------------------------- 4., 5. next-event estimation through a medium
def dot32(a, b):
    """dot3 of rt_math.h in float32: a.x * b.x + a.y * b.y + a.z * b.z, left to right, every operation rounded (the build has -ffp-contract=off)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


HEAD = ('LookAt 0 -3 -9 0 -3 0 0 1 0\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" ["o.exr"]\n'
        'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\nPixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n')
NEE_WORLD = ('LightSource "point" "point from" [0 3 -2] "color I" [20 30 40]\n'
             'AttributeBegin\nTranslate -4 -2 -4\nRotate 20 0 0 1\nLightSource "spot" "point from" [0 0 0] "point to" [.6 -.7 1] "float coneangle" [40] "float conedeltaangle" [12] "color I" [30 25 20]\nAttributeEnd\n'
             'AttributeBegin\nRotate 25 0 0 1\nLightSource "distant" "point from" [1 4 -1] "point to" [0 0 0] "color L" [3 2.5 2]\nAttributeEnd\n'
             'AttributeBegin\nMaterial "matte" "color Kd" [.6 .5 .4]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 -5 -4 6 -5 -4 6 -5 6 -6 -5 6]\nAttributeEnd\n'
             'AttributeBegin\nMaterial "matte" "color Kd" [.4 .6 .7] "float sigma" [25]\n'
             'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -1 -3 3 -1 -3 3 -1 3 -2 -1 3]\nAttributeEnd\n'
             'AttributeBegin\nMaterial "matte" "color Kd" [.7 .7 .3]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 -5 5 6 -5 5 6 2 5 -6 2 5]\nAttributeEnd\n')
NEE_INTEGRATOR = 'SurfaceIntegrator "directlighting" "string strategy" ["all"] "integer maxdepth" [0]\n'
HOM_BOX = 'Volume "homogeneous" "point p0" [-7 -6 -6] "point p1" [7 4 7] "color sigma_a" [.03 .04 .05] "color sigma_s" [.02 .03 .01]\n'
EXP_BOX = ('AttributeBegin\nRotate 10 0 0 1\nVolume "exponential" "point p0" [-8 -7 -7] "point p1" [8 6 8] "color sigma_a" [.03 .04 .05] "color sigma_s" [.02 .03 .01] '
           '"float a" [1.5] "float b" [.3] "vector updir" [.2 1 .1]\nAttributeEnd\n')


def nee_through_a_medium(pkg, text, density):
    """the composition of tests/test_gpu_lights.py with the medium's factors: per light ((f * s_L) * |s_wi . ns|) * (1 / s_pdf), the pending
    contribution the frame forms before the shadow ray returns, times tr(s_ray) when it returns unoccluded (rt_integrate.h ST_SHADOW_DONE), summed in
    scene order; then tr(camera ray cut at the hit) * sum + 0 -- every product restated in float32 on the host.  The factors are the reference's
    f * (L * Transmittance) * AbsDot / pdf (transport.cpp:155-159); the ORDER of the products is the frame kernels', which multiply the transmittance
    in last, and only that order can equal a frame in every bit.  The reference's order is printed beside it: it differs from the frame in the last
    bit of some records."""
    ps, ds = open_scene(pkg, text)
    n = ps.n_camera_samples
    assert [l["type"] for l in ps.lights()] == ["point", "spot", "distant"]
    ds.bind_film(); ds.clear_film(); ds.render()
    rec = ds.samples()[:, :3]
    rays = ds.camera_rays_device(0, n)
    hits = ds.intersect(rays, fields=("p", "ns", "material"))
    h = host(hits)
    hit = h["prim"] >= 0
    ns = h["ns"]
    vs = ds.volume_samples(0, n)
    start = vs["rng"].cpu().numpy().view(np.uint32)
    total, literal = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    reached = np.zeros(n, np.uint32)                                      # lights before this one whose shadow ray reached Transmittance
    kept_by_light, shadowed, dimmed = [], 0, 0
    u = torch.zeros((n, 2), dtype=torch.float32, device="cuda")           # delta lights ignore u
    for l in range(3):
        s = ds.light(hits["p"], dev(np.full(n, l, np.int32)), n=hits["ns"], u=u, fields=("s_wi", "s_L", "s_pdf", "s_ray"))
        occ = ds.occluded(s["s_ray"]).cpu().numpy() > 0
        f = ds.bsdf(rays, hits, wi=s["s_wi"], fields=("f",))["f"].cpu().numpy()
        rng = np.stack([start[:, 0], start[:, 1] + reached], -1).astype(np.uint32)
        tr = ds.medium(rays=s["s_ray"], rng=dev(rng), fields=("tr", "draws"))       # Scene::Transmittance(s_ray): no sample, one draw
        assert (tr["draws"].cpu().numpy() == 1).all()
        tr = tr["tr"].cpu().numpy()
        s = host(s)
        pend = ((f * s["s_L"]) * np.abs(dot32(s["s_wi"], ns))[:, None]) * (np.float32(1) / s["s_pdf"])[:, None]      # div_s rt_math.h: a * (1 / pdf)
        keep = hit & (s["s_pdf"] > 0) & s["s_L"].any(-1) & f.any(-1) & ~occ
        shadowed += int((hit & s["s_L"].any(-1) & f.any(-1) & occ).sum())
        dimmed += int((keep & (tr < 1).all(-1)).sum())
        kept_by_light.append(int(keep.sum()))
        total = total + np.where(keep[:, None], pend * tr, np.float32(0)).astype(np.float32)
        lit = ((f * (s["s_L"] * tr)) * np.abs(dot32(s["s_wi"], ns))[:, None]) * (np.float32(1) / s["s_pdf"])[:, None]     # the reference's order (transport.cpp:155-159)
        literal = literal + np.where(keep[:, None], lit, np.float32(0)).astype(np.float32)
        reached = reached + keep.astype(np.uint32)
    cut = rays.clone()
    cut[:, 7] = torch.where(hits["prim"] >= 0, hits["t"], rays[:, 7])     # Intersect shortened the ray Scene::Li hands to the volume integrator
    T = ds.medium(rays=cut, u=vs["u"], fields=("tr",))["tr"].cpu().numpy()  # Transmittance with the sample: no draw
    ds.close()
    want = (T * total + np.float32(0)).astype(np.float32)
    print("MEDIUM-NEE %s samples %d hit %d kept per light %s shadowed %d dimmed %d" % (density, n, hit.sum(), kept_by_light, shadowed, dimmed))
    differ = int((bits(rec[hit]) != bits(want[hit])).any(-1).sum())
    print("MEDIUM-NEE %s records that differ from the composition in a bit: %d of %d" % (density, differ, hit.sum()))
    other = (T * literal + np.float32(0)).astype(np.float32)
    print("MEDIUM-NEE %s ... and with s_L * tr formed first, as the reference multiplies: %d of %d, largest relative difference %.3g" % (
        density, int((bits(rec[hit]) != bits(other[hit])).any(-1).sum()), hit.sum(), float(np.abs(other[hit] / np.maximum(rec[hit], 1e-30) - 1)[rec[hit] > 0].max())))
    assert np.array_equal(bits(rec[hit]), bits(want[hit])), differ
    assert not rec[~hit].any()
    assert hit.sum() > 200 and min(kept_by_light) > 30 and shadowed > 20 and dimmed > 100       # the scene shows what it is for
    assert (T[hit] < 1).all() and (T[hit] > 0).all()


def test_next_event_estimation_through_a_homogeneous_medium_composes_into_a_frame_bit_for_bit(pkg):
    """a 16 x 16 DirectLighting "all" frame, maxdepth 0, of three matte surfaces under a point, a spot and a distant light inside a homogeneous box
    with Le black under VolumeIntegrator "emission": floats 0..2 of every hit sample's record equal tr(camera ray cut at the hit) * sum + 0"""
    need_gpu(pkg)
    nee_through_a_medium(pkg, HEAD + NEE_INTEGRATOR + 'VolumeIntegrator "emission" "float stepsize" [.5]\nWorldBegin\n' + HOM_BOX + NEE_WORLD + "WorldEnd\n", "homogeneous")


def test_next_event_estimation_through_an_exponential_medium_composes_into_a_frame_bit_for_bit(pkg):
    """the same through an exponential region under a CTM: the camera ray's tr takes u from volume_samples(), each shadow ray's tr is the form
    without u at rng = (key, start + the number of earlier lights that reached Transmittance)"""
    need_gpu(pkg)
    nee_through_a_medium(pkg, HEAD + NEE_INTEGRATOR + 'VolumeIntegrator "emission" "float stepsize" [.5]\nWorldBegin\n' + EXP_BOX + NEE_WORLD + "WorldEnd\n", "exponential")


# ---------------------------------------------------------------------------------------------- 6. lv is a frame's Lv
def test_lv_is_a_frames_lv_bit_for_bit(pkg):
    """a 16 x 16 frame of the emitting, strongly absorbing volumegrid with no light and one triangle outside the view: floats 0..2 of every record
    equal lv(camera ray, u_scatter, rng) with u_scatter and rng from volume_samples() (T * 0 + Lv is Lv); some march takes the roulette's draw"""
    need_gpu(pkg)
    med = MC.CASES["grid_roulette"]["medium"]
    text = ('LookAt .2 .3 -6 .25 .25 0 0 1 0\nCamera "perspective" "float fov" [35]\nFilm "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" ["o.exr"]\n'
            'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["true"]\nPixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n'
            'SurfaceIntegrator "directlighting"\nVolumeIntegrator "emission" "float stepsize" [.25]\nWorldBegin\n' + A._volume_text(med) +
            'AttributeBegin\nMaterial "matte"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [50 50 50 51 50 50 50 51 50]\nAttributeEnd\nWorldEnd\n')
    ps, ds = open_scene(pkg, text)
    n = ps.n_camera_samples
    ds.bind_film(); ds.clear_film(); ds.render()
    rec = ds.samples()[:, :3]
    rays = ds.camera_rays_device(0, n)
    vs = ds.volume_samples(0, n)
    got = host(ds.medium(rays=rays, u_scatter=vs["u_scatter"], rng=vs["rng"], fields=("lv", "draws", "hit", "t01", "status")))
    ds.close()
    differ = int((bits(rec) != bits(got["lv"])).any(-1).sum())
    steps = np.ceil((got["t01"][:, 1] - got["t01"][:, 0]) / np.float32(.25)).astype(np.int32)
    roulette = (got["hit"] == 1) & (got["draws"] != steps)                # without the roulette a march draws once per step
    print("MEDIUM-LV records that differ in a bit: %d of %d; marches %d, with a roulette draw %d" % (differ, n, (got["hit"] == 1).sum(), roulette.sum()))
    assert np.array_equal(bits(rec), bits(got["lv"])), differ
    assert (got["hit"] == 1).sum() > 100 and got["lv"].any(-1).sum() > 100 and not got["status"].any()
    assert roulette.sum() >= 1


# ---------------------------------------------------------------------------------------------- 7. launch shapes
def test_launch_shapes_and_single_outputs(pkg):
    """n = 1, 63, 64, 65, 256, 257 and a fixture tiled to about 6.6e5 rows (more than the resident threads: the grid-stride loop) give the rows
    of the one-call answer bitwise; an output asked alone equals the same output asked with all the others"""
    need_gpu(pkg)
    fx = fixture("grid_roulette")
    ps, ds = open_scene(pkg, MC.product_text(fx["scene"]))
    whole = host(ds.medium(**inputs(fx)))
    for n in (1, 63, 64, 65, 256, 257):
        part = host(ds.medium(**inputs(fx, slice(0, n))))
        for k, v in part.items():
            assert np.array_equal(bits(v), bits(whole[k][:n])), (n, k)
    reps = 645
    big = {k: dev(np.tile(fx[k], (reps,) + (1,) * (fx[k].ndim - 1))) for k in INPUTS}
    got = ds.medium(**big)
    m = len(fx["rays"])
    for k, v in got.items():
        v = v.reshape((reps, m) + tuple(v.shape[1:]))
        assert bool((v.view(torch.int32) == torch.from_numpy(bits(whole[k]).view(np.int32)).cuda()[None]).all().item()), k
    del big, got
    ins = inputs(fx)
    for k in pkg.MEDIUM_FIELDS:
        if k == "draws":                                                  # how far the stream moved depends on what was asked: with lv, lv's draws
            alone = host(ds.medium(**ins, fields=("lv", "draws")))
        else:
            alone = host(ds.medium(**ins, fields=(k,)))
        assert np.array_equal(bits(alone[k]), bits(whole[k])), k
    ds.close()
    assert whole["lv"].any() and whole["draws"].max() > 5 and whole["hit"].sum() > 300


# ---------------------------------------------------------------------------------------------- 8. the march guard
def test_a_march_that_cannot_advance_is_not_started(pkg):
    """rays that meet an axis-aligned exponential region 3e8 units from their origin, where t + step == t for every step the query uses, an
    unusable ray (a NaN origin, a zero direction) and ordinary rays in one call: the call returns, the flagged rows are zero in tau, tr and lv
    with bit 0 of status set, and the ordinary rows are bitwise what a call without the others gives.  The guard refuses these marches before
    their first step; nothing here runs a loop that would not end."""
    need_gpu(pkg)
    med = dict(MC.CASES["exponential_ctm"]["medium"], ctm=[])
    text = ('LookAt 0 0 -9 0 0 0 0 1 0\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [4] "integer yresolution" [4] "string filename" ["o.exr"]\n'
            'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\nSurfaceIntegrator "directlighting"\n'
            'VolumeIntegrator "emission" "float stepsize" [.25]\nWorldBegin\n' + A._volume_text(med) +
            'AttributeBegin\nMaterial "matte"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [50 50 50 51 50 50 50 51 50]\nAttributeEnd\nWorldEnd\n')
    fx = fixture("exponential_ctm")
    n = 192
    rays = fx["rays"][:n].copy()
    kind = np.arange(n) % 4                                               # 0, 2: ordinary; 1: far away; 3: unusable
    far = kind == 1
    rs = np.random.RandomState(8)
    rays[far, 0:3] = np.stack([rs.uniform(-.5, 1, far.sum()), rs.uniform(-.2, .7, far.sum()), np.full(far.sum(), -3e8)], -1)
    rays[far, 3:6], rays[far, 6], rays[far, 7] = [0, 0, 1], 0, np.inf
    bad = kind == 3
    rays[bad & (np.arange(n) % 8 == 3), 0] = np.nan
    rays[bad & (np.arange(n) % 8 == 7), 3:6] = 0
    ps, ds = open_scene(pkg, text)
    other = {k: fx[k][:n] for k in ("u", "u_scatter", "rng")}
    fields = ("hit", "tau", "tr", "lv", "draws", "status")
    got = host(ds.medium(rays=dev(rays), **{k: dev(v) for k, v in other.items()}, fields=fields))
    ds.sync()
    good = ~(far | bad)
    alone = host(ds.medium(rays=dev(rays[good]), **{k: dev(v[good]) for k, v in other.items()}, fields=fields))
    ds.close()
    flagged = far | bad
    assert (got["status"][flagged] & 1).all() and not got["status"][good].any()
    for k in ("tau", "tr", "lv"):
        assert not got[k][flagged].any(), k
    assert (got["hit"][far] == 1).all() and not got["hit"][bad].any()
    for k in fields:
        assert np.array_equal(bits(got[k][good]), bits(alone[k])), k
    assert got["tau"][good].any(-1).sum() > 20 and got["lv"][good].any(-1).sum() > 20


# ---------------------------------------------------------------------------------------------- 9. no medium
def test_a_scene_without_a_medium(pkg):
    """tr = 1, zeros in every other float output, hit = 0, draws = 1 exactly where the form without u was asked"""
    need_gpu(pkg)
    fx = fixture("grid")
    ps, ds = open_scene(pkg, str(load_golden("probe_cornell")["scene"]).replace('SurfaceIntegrator "probe"', 'SurfaceIntegrator "whitted"'))
    got = host(ds.medium(**inputs(fx), step_size=.25))
    null = host(ds.medium(**inputs(fx, skip=("u",)), step_size=.25, fields=("tr", "draws", "hit")))
    ds.close()
    for k, v in got.items():
        assert (v == 1).all() if k == "tr" else not v.any(), k
    assert (null["tr"] == 1).all() and (null["draws"] == 1).all() and not null["hit"].any()


# ---------------------------------------------------------------------------------------------- 10. a query is not a frame
def test_a_query_leaves_the_last_frame_as_it_was(pkg):
    """film, samples(), counters() and last_stats() after medium() and volume_samples() calls on a rendered scene, bitwise; a second render() gives the first film"""
    need_gpu(pkg)
    fx = fixture("exponential_ctm")
    ps, ds = open_scene(pkg, MC.product_text(fx["scene"]))
    ds.bind_film(); ds.set_counting(True); ds.clear_film(); ds.reset_counters()
    ds.render()
    film, samples, cnt, stats = ds.film_accum(), ds.samples(), ds.counters(), ds.last_stats()
    first = ask(ds, fx)
    for _ in range(2):
        again = ask(ds, fx)
        ds.volume_samples(0, ps.n_camera_samples)
        for k in first:
            assert np.array_equal(bits(again[k]), bits(first[k])), k
        ds.sync()
        assert np.array_equal(bits(ds.film_accum()), bits(film)) and np.array_equal(bits(ds.samples()), bits(samples))
        assert ds.counters() == cnt and ds.last_stats() == stats
    ds.clear_film(); ds.reset_counters()
    ds.render()
    assert np.array_equal(bits(ds.film_accum()), bits(film)) and np.array_equal(bits(ds.samples()), bits(samples)) and ds.counters() == cnt
    ds.close()


# ---------------------------------------------------------------------------------------------- 11. refusals
def test_refusals_name_the_function_and_launch_nothing(pkg):
    need_gpu(pkg)
    fx = fixture("grid")
    ps, ds = open_scene(pkg, MC.product_text(fx["scene"]))
    L = pkg.hip_lib()
    n = 64
    ins = {k: dev(fx[k][:n]) for k in INPUTS}
    out = {k: torch.zeros((n, 3), dtype=torch.float32, device="cuda") for k in ("sigma_a", "sigma_s", "sigma_t", "lve", "tau", "tr", "lv")}
    out.update(phase=torch.zeros(n, dtype=torch.float32, device="cuda"), t01=torch.zeros((n, 2), dtype=torch.float32, device="cuda"))
    out.update({k: torch.zeros(n, dtype=torch.int32, device="cuda") for k in ("hit", "draws", "status")})
    torch.cuda.synchronize()
    Q = lambda **kw: pkg.RtMediumQuery(**{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    host_values = dict(seed=5, step_size=.25, volume_integrator=pkg.VOLUME_EMISSION)
    whole = Q(**ins, **host_values, **out)
    drop = lambda *names, **more: Q(**{k: v for k, v in dict(ins, **host_values, **out).items() if k not in names}, **more)
    cases = (((None, n, whole), ("null scene",)),
             ((ds._s, n, None), ("null RtMediumQuery",)),
             ((ds._s, n, Q(**ins, **host_values)), ("every output", "null")),
             ((ds._s, n, drop("p")), ("sigma_a, sigma_s, sigma_t, lve or phase", "p is null")),
             ((ds._s, n, drop("w")), ("phase", "w or wp is null")),
             ((ds._s, n, drop("wp")), ("phase", "w or wp is null")),
             ((ds._s, n, Q(w=ins["w"], wp=ins["wp"], **host_values, phase=out["phase"])), ("p is null",)),
             ((ds._s, n, drop("rays")), ("hit, t01, tau, tr, lv, draws or status", "rays is null")),
             ((ds._s, n, drop("u")), ("tau is wanted", "u is null")),
             ((ds._s, n, drop("u_scatter")), ("lv is wanted", "u_scatter is null")),
             ((ds._s, n, drop("rays", rays=ins["rays"].data_ptr() + 8)), ("rays", "16-byte aligned")),
             ((ds._s, n, drop("volume_integrator", volume_integrator=pkg.VOLUME_SINGLE)), ("lv", "RT_VOLUME_SINGLE")),
             ((ds._s, n, drop("step_size", step_size=0.0)), ("step_size", "positive and finite")),
             ((ds._s, n, drop("step_size", step_size=-1.0)), ("step_size", "positive and finite")),
             ((ds._s, n, drop("step_size", step_size=float("inf"))), ("step_size", "positive and finite")),
             ((ds._s, n, drop("step_size", step_size=float("nan"))), ("step_size", "positive and finite")),
             ((ds._s, n, drop("step_size", step_size=5e-5)), ("step_size too small", "65536")),
             ((ds._s, 2 ** 30 + 1, whole), ("above 2^30",)))
    for args, words in cases:
        q = args[2]
        assert L.rt_medium_device(args[0], args[1], C.byref(q) if q is not None else None) == -1, words          # RT_EINVAL
        msg = L.rt_last_error().decode()
        assert "rt_medium_device" in msg and all(wd in msg for wd in words), msg
    assert L.rt_medium_device(ds._s, 0, None) == 0                                               # n == 0: RT_OK, nothing launched
    assert L.rt_medium_device(ds._s, 0, C.byref(whole)) == 0
    # rt_volume_samples_device: the refusals of rt_sample_positions_device
    rd = ps.render_desc
    words4 = torch.zeros((n + 1, 4), dtype=torch.int32, device="cuda")
    for args, words in (((None, rd, 0, 8, C.c_void_p(words4.data_ptr())), ("null scene",)),
                        ((ds._s, None, 0, 8, C.c_void_p(words4.data_ptr())), ("null render description",)),
                        ((ds._s, rd, 0, 8, None), ("null output pointer",)),
                        ((ds._s, rd, 0, 8, C.c_void_p(words4.data_ptr() + 4)), ("dev_out", "16-byte aligned")),
                        ((ds._s, rd, ps.n_camera_samples - 7, 8, C.c_void_p(words4.data_ptr())), ("beyond the frame's camera samples",))):
        assert L.rt_volume_samples_device(*args) == -1, words
        msg = L.rt_last_error().decode()
        assert "rt_volume_samples_device" in msg and all(wd in msg for wd in words), msg
    assert L.rt_volume_samples_device(ds._s, rd, 5, 0, None) == 0
    ds.sync()
    assert all(not t.any().item() for t in out.values()) and not words4.any().item()          # nothing was launched: nothing was written
    # the wrapper's own checks on device tensors
    p, rays, u = ins["p"], ins["rays"], ins["u"]
    for kw, word in ((dict(rays=rays, fields=("sigma_a",)), "p: needed"), (dict(p=p, fields=("phase",)), "w, wp: needed"), (dict(p=p, fields=("tau",)), "rays: needed"),
                     (dict(rays=rays, fields=("tau",)), "u: needed"), (dict(rays=rays, fields=("lv",)), "u_scatter: needed"), (dict(rays=rays, fields=("nope",)), "unknown field"),
                     (dict(rays=rays, fields=()), "at least one"), (dict(rays=rays, u=u.double(), fields=("tau",)), "float32"),
                     (dict(rays=rays, u=u[:, None].contiguous(), fields=("tau",)), "shape"), (dict(rays=rays, u=u.cpu(), fields=("tau",)), "is on"),
                     (dict(rays=rays, rng=ins["rng"].float(), fields=("tr",)), "dtype")):
        with pytest.raises(ValueError) as e:
            ds.medium(**kw)
        assert word in str(e.value), (kw.keys(), str(e.value))
    assert ds.medium(rays=rays[:0].contiguous(), fields=("hit",))["hit"].shape == (0,)
    ds.close()
