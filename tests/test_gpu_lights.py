"""Light queries at caller-supplied points on the GPU: DeviceScene.light (rt_light_device) against the reference's own answers per query (the four
fixtures of tests/golden/lights/, made by the reference-side plugin tests/golden/light_probe.cpp), the pdf of a sampled direction, the shadow ray
handed to occluded(), next-event estimation composed into a DirectLighting frame bit for bit, the keyed draw under a caller's key, the refusals, and
that a query is no frame."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
# torch BEFORE the device library is loaded, as bench.py does (see tests/test_gpu_rays.py)
import torch

import analytic_cases as A
import bsdf_forms as B
import light_cases as LC
import light_forms as LF
from conftest import GOLDEN
from gpu_checks import need_gpu

pytestmark = pytest.mark.gpu

SAMPLE_FIELDS = ("s_wi", "s_L", "s_pdf", "s_ray", "s_draws")


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
    z = np.load(os.path.join(GOLDEN, "lights", name + ".npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the float64 forms on the fixture (for the exclusion mask): computed once per session"""
    fx = fixture(name)
    return LC.evaluate(name, fx, int(fx["seed"]))


def ask(ds, fx, fields, rows=None):
    """the fixture's queries in two launches -- the form with a normal, the form without -- put back in the fixture's order"""
    rows = np.arange(len(fx["p"])) if rows is None else rows
    out = {}
    for wn in (1, 0):
        sel = rows[fx["with_normal"][rows] == wn]
        t = lambda k: dev(fx[k][sel])
        got = host(ds.light(t("p"), t("light"), n=t("nrm") if wn else None, u=t("u"), rng=t("rng"), wi=t("wi"), fields=fields))
        for k, v in got.items():
            out.setdefault(k, np.zeros((len(fx["p"]),) + v.shape[1:], v.dtype))[sel] = v
    return out


def split_ray(got):
    r = got.pop("s_ray")
    got.update(s_ray_o=r[:, 0:3], s_ray_d=r[:, 3:6], mint=r[:, 6], maxt=r[:, 7])
    return got


# ---------------------------------------------------------------------------------------------- 1. the reference's answers, per query
@pytest.mark.parametrize("fields", ["all", "s_wi"])
@pytest.mark.parametrize("name", list(LC.CASES))
def test_every_output_agrees_with_the_reference_per_query(pkg, name, fields):
    """every float output within 4 x max(ref_err(case, output), the median ref_err of that output over the cases) of the reference's value in the
    measure of bsdf_forms.query_error -- ref_err being the reference's own largest error against the float64 forms, stored in the fixtures --;
    s_draws, is_delta, the shadow ray's mint and maxt and which outputs are exactly zero equal the reference's.  Only the queries the forms' rule
    leaves out (at most 3 %) are not compared.  Once with all outputs, once with s_wi alone (the wave-uniform output selection)."""
    need_gpu(pkg)
    fx, w = fixture(name), expected(name)
    inc = ~w["excluded"]
    assert w["excluded"].mean() <= A.BAND_CAP
    median = np.median([fixture(c)["ref_err"] for c in LC.CASES], axis=0)
    ps, ds = open_scene(pkg, LC.product_text(fx["scene"]))
    got = ask(ds, fx, pkg.LIGHT_FIELDS if fields == "all" else ("s_wi",))
    ds.close()
    if fields == "all":
        split_ray(got)
    ans = fx["answers"]
    failed = []
    zero = lambda a: ~np.asarray(a).reshape(len(a), -1).any(-1)
    for i, k in enumerate(LC.OUTPUTS):
        if k not in got:
            continue
        bar = A.BAR_FACTOR * max(float(fx["ref_err"][i]), float(median[i]))
        e = B.query_error(got[k], LC.answer(ans, k), inc, unit_scale=(k == "s_wi"))[inc].max()
        differ = int((bits(got[k][inc]) != bits(LC.answer(ans, k)[inc])).reshape(int(inc.sum()), -1).any(-1).sum())
        print("LIGHT-REF %s %-8s e %.3g bar %.3g (ref_err %.3g, median %.3g), %d of %d differ in a bit" % (name, k, e, bar, fx["ref_err"][i], median[i], differ, int(inc.sum())))
        if not e <= bar:
            failed.append((k, float(e), bar))
        if not np.array_equal(zero(got[k])[inc], zero(LC.answer(ans, k))[inc]):
            failed.append((k, "zero pattern", int((zero(got[k])[inc] != zero(LC.answer(ans, k))[inc]).sum())))
    for k in ("s_draws", "is_delta", "mint", "maxt"):
        if k not in got:
            continue
        differ = int((got[k][inc] != LC.answer(ans, k)[inc]).sum())
        print("LIGHT-REF %s %-8s differing %d of %d" % (name, k, differ, int(inc.sum())))
        if differ:
            failed.append((k, differ))
    assert not failed, (name, failed)


# ---------------------------------------------------------------------------------------------- 2. the pdf of the sampled direction
def test_pdf_at_the_sampled_direction_is_the_samples_pdf_bit_for_bit(pkg):
    """on the triangle emitters both are shape->Pdf(p, wi) (area.cpp:65, :71)"""
    need_gpu(pkg)
    fx = fixture("emitters_tri")
    ps, ds = open_scene(pkg, LC.product_text(fx["scene"]))
    p, li, u, rng = (dev(fx[k]) for k in ("p", "light", "u", "rng"))
    s = ds.light(p, li, u=u, rng=rng, fields=("s_wi", "s_pdf"))
    again = ds.light(p, li, wi=s["s_wi"], fields=("pdf",))["pdf"].cpu().numpy()
    s_pdf = s["s_pdf"].cpu().numpy()
    ds.close()
    assert (s_pdf > 0).sum() > 1000 and (s_pdf == 0).sum() > 20
    assert np.array_equal(bits(again), bits(s_pdf)), int((bits(again) != bits(s_pdf)).sum())


# ---------------------------------------------------------------------------------------------- 3. the shadow ray
HEAD = ('LookAt 0 -3 -9 0 -3 0 0 1 0\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" ["o.exr"]\n'
        'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\nPixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n')
MATTE = 'Material "matte" "color Kd" [.6 .5 .4]\n'
FLOOR = 'AttributeBegin\n' + MATTE + 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-9 -9 -9 9 -9 -9 9 -9 9 -9 -9 9]\nAttributeEnd\n'
POINT_AT = (0.0, 3.0, 0.0)
# the query points lie in the box [-2, 2] x [-4, -2] x [-2, 2]; the point and spot lights stand above it, the emitter is a wall at x = 5 that faces it:
# no segment from the box to a light meets anything
OPEN_LIGHTS = ('LightSource "point" "point from" [0 3 0] "color I" [20 30 40]\n'
               'LightSource "spot" "point from" [-3 2 0] "point to" [0 -3 0] "float coneangle" [60] "float conedeltaangle" [10] "color I" [30 25 20]\n'
               'LightSource "distant" "point from" [1 4 -1] "point to" [0 0 0] "color L" [3 2.5 2]\n'
               'AttributeBegin\n' + MATTE + 'AreaLightSource "area" "color L" [2 3 4]\n'
               'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [5 -5 -2 5 -5 2 5 0 2 5 0 -2]\nAttributeEnd\n')
BLOCKER = 'AttributeBegin\n' + MATTE + 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-.5 0 -.5 .5 0 -.5 .5 0 .5 -.5 0 .5]\nAttributeEnd\n'
HALF = .5                 # the blocker: the square |x|, |z| <= HALF in the plane y = 0


def box_points(n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-2, 2, n), rs.uniform(-4, -2, n), rs.uniform(-2, 2, n)], -1).astype(np.float32)


def test_shadow_rays_go_to_occluded_as_they_are(pkg):
    """without blockers occluded(s_ray) is 0 for every usable sample (pdf > 0, L not black) of a point, a spot, a distant light and an emitter; with a
    square between the points and the point light it is 1 exactly where the float64 segment p -> light crosses the square (a band of 1e-4 about its
    edges left out)"""
    need_gpu(pkg)
    n = 1024
    p = box_points(n, 31)
    u = np.random.RandomState(32).uniform(size=(n, 2)).astype(np.float32)
    text = HEAD + 'SurfaceIntegrator "directlighting"\nWorldBegin\n' + OPEN_LIGHTS + FLOOR + "WorldEnd\n"
    ps, ds = open_scene(pkg, text)
    assert [l["type"] for l in ps.lights()] == ["point", "spot", "distant", "area"]
    usable = 0
    for l in range(4):
        s = ds.light(dev(p), dev(np.full(n, l, np.int32)), u=dev(u), fields=("s_L", "s_pdf", "s_ray"))
        occ = ds.occluded(s["s_ray"]).cpu().numpy()
        ok = (s["s_pdf"].cpu().numpy() > 0) & s["s_L"].cpu().numpy().any(-1)
        assert ok.sum() > n // 2, (l, int(ok.sum()))
        assert not occ[ok].any(), (l, int(occ[ok].sum()))
        usable += int(ok.sum())
    ds.close()
    ps, ds = open_scene(pkg, HEAD + 'SurfaceIntegrator "directlighting"\nWorldBegin\n' + OPEN_LIGHTS + BLOCKER + FLOOR + "WorldEnd\n")
    s = ds.light(dev(p), dev(np.zeros(n, np.int32)), u=dev(u), fields=("s_ray",))
    occ = ds.occluded(s["s_ray"]).cpu().numpy()
    ds.close()
    pd = p.astype(np.float64)
    t = (0 - pd[:, 1]) / (POINT_AT[1] - pd[:, 1])                       # where the segment meets the plane y = 0
    x, z = pd[:, 0] + t * (POINT_AT[0] - pd[:, 0]), pd[:, 2] + t * (POINT_AT[2] - pd[:, 2])
    inside = (np.abs(x) < HALF) & (np.abs(z) < HALF)
    band = (np.abs(np.abs(x) - HALF) < 1e-4) & (np.abs(z) < HALF + 1e-4) | (np.abs(np.abs(z) - HALF) < 1e-4) & (np.abs(x) < HALF + 1e-4)
    print("LIGHT-SHADOW usable %d, in the square's shadow %d of %d, band %d" % (usable, inside.sum(), n, band.sum()))
    assert inside.sum() > 100 and (~inside).sum() > 100 and band.mean() <= A.BAND_CAP
    assert np.array_equal(occ[~band] > 0, inside[~band]), int(((occ > 0) != inside)[~band].sum())


# ---------------------------------------------------------------------------------------------- 4. next-event estimation, composed into a frame
def dot32(a, b):
    """dot3 of rt_math.h in float32: a.x * b.x + a.y * b.y + a.z * b.z, left to right, every operation rounded (the build has -ffp-contract=off)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


NEE_FRAME = (HEAD + 'SurfaceIntegrator "directlighting" "string strategy" ["all"] "integer maxdepth" [0]\nWorldBegin\n'
             'LightSource "point" "point from" [0 3 -2] "color I" [20 30 40]\n'
             'AttributeBegin\nTranslate -4 -2 -4\nRotate 20 0 0 1\nLightSource "spot" "point from" [0 0 0] "point to" [.6 -.7 1] "float coneangle" [40] "float conedeltaangle" [12] "color I" [30 25 20]\nAttributeEnd\n'
             'AttributeBegin\nRotate 25 0 0 1\nLightSource "distant" "point from" [1 4 -1] "point to" [0 0 0] "color L" [3 2.5 2]\nAttributeEnd\n'
             'AttributeBegin\nMaterial "matte" "color Kd" [.6 .5 .4]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 -5 -4 6 -5 -4 6 -5 6 -6 -5 6]\nAttributeEnd\n'
             'AttributeBegin\nMaterial "matte" "color Kd" [.4 .6 .7] "float sigma" [25]\n'         # a shelf above the floor: its shadow covers a good part of it
             'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -1 -3 3 -1 -3 3 -1 3 -2 -1 3]\nAttributeEnd\n'
             'AttributeBegin\nMaterial "matte" "color Kd" [.7 .7 .3]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 -5 5 6 -5 5 6 2 5 -6 2 5]\nAttributeEnd\n'
             'WorldEnd\n')


def test_next_event_estimation_composes_into_a_directlighting_frame_bit_for_bit(pkg):
    """a 16 x 16 DirectLighting "all" frame of three matte surfaces (a floor, a wall and an Oren-Nayar shelf that shadows both) under a point, a spot and a distant light: floats
    0..2 of every camera sample's record are the sum over the lights, in scene order, of ((f * s_L) * |s_wi . ns|) / s_pdf for the lights EstimateDirect
    keeps (pdf > 0, L not black, f not black, s_ray not occluded; transport.cpp:153-166, :31-50) -- camera_rays_device -> intersect -> light -> occluded ->
    bsdf(f), every product and sum restated in float32 on the host"""
    need_gpu(pkg)
    ps, ds = open_scene(pkg, NEE_FRAME)
    n = ps.n_camera_samples
    assert [l["type"] for l in ps.lights()] == ["point", "spot", "distant"]
    ds.bind_film(); ds.clear_film(); ds.render()
    rec = ds.samples()[:, :3]
    rays = ds.camera_rays_device(0, n)
    hits = ds.intersect(rays, fields=("p", "ns", "material"))
    h = host(hits)
    hit = h["prim"] >= 0
    ns = h["ns"]
    total = np.zeros((n, 3), np.float32)                                  # UniformSampleAllLights' L
    kept_by_light, shadowed = [], 0
    u = torch.zeros((n, 2), dtype=torch.float32, device="cuda")           # delta lights ignore u
    for l in range(3):
        s = ds.light(hits["p"], dev(np.full(n, l, np.int32)), n=hits["ns"], u=u, fields=("s_wi", "s_L", "s_pdf", "s_ray"))
        occ = ds.occluded(s["s_ray"]).cpu().numpy() > 0
        f = ds.bsdf(rays, hits, wi=s["s_wi"], fields=("f",))["f"].cpu().numpy()
        s = host(s)
        term = ((f * s["s_L"]) * np.abs(dot32(s["s_wi"], ns))[:, None]) * (np.float32(1) / s["s_pdf"])[:, None]      # div_s rt_math.h: a * (1 / pdf)
        keep = hit & (s["s_pdf"] > 0) & s["s_L"].any(-1) & f.any(-1) & ~occ
        shadowed += int((hit & s["s_L"].any(-1) & f.any(-1) & occ).sum())
        kept_by_light.append(int(keep.sum()))
        total = total + np.where(keep[:, None], term, np.float32(0)).astype(np.float32)       # L += Ld / nSamples, nSamples = 1
    ds.close()
    print("LIGHT-NEE samples %d hit %d kept per light %s shadowed %d materials %s" % (n, hit.sum(), kept_by_light, shadowed, np.unique(h["material"][hit])))
    differ = int((bits(rec[hit]) != bits(total[hit])).any(-1).sum())
    print("LIGHT-NEE records that differ from the composition in a bit: %d of %d" % (differ, hit.sum()))
    assert np.array_equal(bits(rec[hit]), bits(total[hit])), differ
    assert not rec[~hit].any()
    assert hit.sum() > 200 and min(kept_by_light) > 30 and shadowed > 20 and len(np.unique(h["material"][hit])) == 3       # the scene shows what it is for


# ---------------------------------------------------------------------------------------------- 5. the draw under a caller's key
def test_a_draw_reproduces_under_the_callers_key(pkg):
    """the two-triangle emitter of the "infinite" case asked with rng = (k, c): the triangle sampled is the one the float32 keyed value
    pcg(c + pcg(k + seed * 0x9E3779B9)) picks (restated in numpy, light_forms.keyed_draw), under the scene's seed and under another; rng = None is (i, 0)"""
    need_gpu(pkg)
    fx = fixture("infinite")
    ps, ds = open_scene(pkg, LC.product_text(fx["scene"]))
    n = 2048
    rs = np.random.RandomState(41)
    p = (np.array([2.0, 0.0, 1.0]) + rs.uniform(-3, 3, (n, 3))).astype(np.float32)
    u = rs.uniform(.05, .9, (n, 2)).astype(np.float32)
    rng = np.stack([rs.randint(0, 1 << 31, n), rs.randint(0, 40, n)], -1).astype(np.uint32)
    rng[::7, 0] |= np.uint32(0x80000000)
    li = np.full(n, 2, np.int32)
    form = LC.forms("infinite")[2]
    picks = set()
    for seed in (None, 77):
        got = host(ds.light(dev(p), dev(li), u=dev(u), rng=dev(rng), seed=seed, fields=("s_ray", "s_draws")))
        draw = LF.keyed_draw(rng[:, 0], rng[:, 1], LC.SEED if seed is None else seed)
        want = form.query(p.astype(np.float64), None, False, u[:, 0].astype(np.float64), u[:, 1].astype(np.float64), draw, np.tile([0.0, 0.0, 1.0], (n, 1)))
        ok = ~(np.abs(draw.astype(np.float64) - form.cdf[0]) <= LF.CDF_ULPS * 2.0 ** -24)
        assert ok.mean() > .99 and (got["s_draws"] == 1).all()
        assert np.abs(got["s_ray"][ok, 3:6] - want["s_ray_d"][ok]).max() < 1e-4
        picks |= set(np.unique(want["tag"][ok] // 16))
        # the other triangle's point is far from this one's: the bound above tells the picks apart
        other = form.query(p.astype(np.float64), None, False, u[:, 0].astype(np.float64), u[:, 1].astype(np.float64), np.float32(1) - draw, np.tile([0.0, 0.0, 1.0], (n, 1)))
        flipped = ok & (other["tag"] // 16 != want["tag"] // 16)
        assert flipped.sum() > n // 4 and np.abs(other["s_ray_d"][flipped] - want["s_ray_d"][flipped]).max(-1).min() > 1e-2
    assert picks == {0, 1}
    a = host(ds.light(dev(p), dev(li), u=dev(u), fields=SAMPLE_FIELDS))
    idx = np.stack([np.arange(n), np.zeros(n)], -1).astype(np.uint32)
    b = host(ds.light(dev(p), dev(li), u=dev(u), rng=dev(idx), fields=SAMPLE_FIELDS))
    ds.close()
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


# ---------------------------------------------------------------------------------------------- 6. a query is not a frame
def test_a_query_leaves_the_last_frame_as_it_was(pkg):
    """film, samples(), counters() and last_stats() after light() calls on a rendered scene, bitwise; then a second render() gives the first film"""
    need_gpu(pkg)
    fx = fixture("infinite")
    ps, ds = open_scene(pkg, LC.product_text(fx["scene"]))
    ds.bind_film(); ds.set_counting(True); ds.clear_film(); ds.reset_counters()
    ds.render()
    film, samples, cnt, stats = ds.film_accum(), ds.samples(), ds.counters(), ds.last_stats()
    first = ask(ds, fx, pkg.LIGHT_FIELDS)
    for _ in range(2):
        again = ask(ds, fx, pkg.LIGHT_FIELDS)
        for k in first:
            assert np.array_equal(bits(again[k]), bits(first[k])), k
        ds.sync()
        assert np.array_equal(bits(ds.film_accum()), bits(film)) and np.array_equal(bits(ds.samples()), bits(samples))
        assert ds.counters() == cnt and ds.last_stats() == stats
    ds.clear_film(); ds.reset_counters()
    ds.render()
    assert np.array_equal(bits(ds.film_accum()), bits(film)) and np.array_equal(bits(ds.samples()), bits(samples)) and ds.counters() == cnt
    again = ask(ds, fx, pkg.LIGHT_FIELDS)
    ds.close()
    for k in first:
        assert np.array_equal(bits(again[k]), bits(first[k])), k


# ---------------------------------------------------------------------------------------------- 7. refusals, a bad light index
def test_refusals_name_the_function_and_launch_nothing(pkg):
    need_gpu(pkg)
    fx = fixture("delta")
    ps, ds = open_scene(pkg, LC.product_text(fx["scene"]))
    L = pkg.hip_lib()
    n = 64
    p, nrm, li, u, rng, wi = (dev(fx[k][:n]) for k in ("p", "nrm", "light", "u", "rng", "wi"))
    out = {k: torch.zeros((n, 3), dtype=torch.float32, device="cuda") for k in ("s_wi", "s_L", "le")}
    out.update({k: torch.zeros(n, dtype=torch.float32, device="cuda") for k in ("s_pdf", "pdf")})
    out.update({k: torch.zeros(n, dtype=torch.int32, device="cuda") for k in ("s_draws", "is_delta")})
    out["s_ray"] = torch.zeros((n + 1, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    Q = lambda **kw: pkg.RtLightQuery(**{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    ins = dict(p=p, nrm=nrm, light=li, u=u, rng=rng, wi=wi, seed=5)
    whole = Q(**ins, **out)
    drop = lambda *names, **more: Q(**{k: v for k, v in dict(ins, **out).items() if k not in names}, **more)
    cases = (((None, n, whole), ("null scene",)),
             ((ds._s, n, None), ("null RtLightQuery",)),
             ((ds._s, n, drop("p")), ("null p",)),
             ((ds._s, n, drop("light")), ("null light",)),
             ((ds._s, n, Q(**ins)), ("every output", "null")),
             ((ds._s, n, drop("u")), ("s_wi, s_L, s_pdf, s_ray or s_draws", "u is null")),
             ((ds._s, n, Q(p=p, light=li, wi=wi, s_draws=out["s_draws"])), ("s_wi, s_L, s_pdf, s_ray or s_draws", "u is null")),
             ((ds._s, n, drop("wi")), ("pdf or le", "wi is null")),
             ((ds._s, n, Q(p=p, light=li, u=u, le=out["le"])), ("pdf or le", "wi is null")),
             ((ds._s, n, drop("s_ray", s_ray=out["s_ray"].data_ptr() + 8)), ("s_ray", "16-byte aligned")),
             ((ds._s, 2 ** 30 + 1, whole), ("above 2^30",)))
    for args, words in cases:
        q = args[2]
        assert L.rt_light_device(args[0], args[1], C.byref(q) if q is not None else None) == -1, words          # RT_EINVAL
        msg = L.rt_last_error().decode()
        assert "rt_light_device" in msg and all(wd in msg for wd in words), msg
    assert L.rt_light_device(ds._s, 0, None) == 0                                                # n == 0: RT_OK, nothing launched
    assert L.rt_light_device(ds._s, 0, C.byref(whole)) == 0
    ds.sync()
    assert all(not t.any().item() for t in out.values())                                      # nothing was launched: nothing was written
    # the wrapper's own checks on device tensors
    for kw, word in ((dict(fields=("s_wi",)), "u: needed"), (dict(u=u, fields=("pdf",)), "wi: needed"), (dict(u=u, fields=("nope",)), "unknown field"),
                     (dict(u=u, fields=()), "at least one"), (dict(u=u.double(), fields=("s_wi",)), "float32"), (dict(u=u, wi=wi[:, :2].contiguous(), fields=("le",)), "shape"),
                     (dict(u=u.cpu(), fields=("s_wi",)), "is on"), (dict(u=u, rng=rng.float(), fields=("s_wi",)), "dtype")):
        with pytest.raises(ValueError) as e:
            ds.light(p, li, **kw)
        assert word in str(e.value), (kw.keys(), str(e.value))
    assert ds.light(p[:0].contiguous(), li[:0].contiguous(), fields=("is_delta",))["is_delta"].shape == (0,)
    # a light index outside the scene's lights: zeros in every output, the neighbours untouched
    base = host(ds.light(p, li, n=nrm, u=u, rng=rng, wi=wi))
    bad = li.clone()
    bad[3], bad[17], bad[40] = -1, 3, 2 ** 31 - 1
    got = host(ds.light(p, bad, n=nrm, u=u, rng=rng, wi=wi))
    ds.close()
    changed = np.zeros(n, bool)
    changed[[3, 17, 40]] = True
    for k, v in got.items():
        assert not v[changed].any(), k
        assert np.array_equal(bits(v[~changed]), bits(base[k][~changed])), k
    assert base["s_ray"][changed].any() and base["is_delta"][changed].all()
