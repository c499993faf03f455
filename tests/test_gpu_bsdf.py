"""BSDF queries at caller-supplied hits on the GPU: DeviceScene.bsdf (rt_bsdf_device) against the reference's own answers per query (the five
fixtures of tests/golden/bsdf/, made by the reference-side plugin tests/golden/bsdf_probe.cpp), composed into Whitted frames bit for bit (f in the
light loop, the specular Sample_f in the mirror step), its sampling against its f, launch shapes and single outputs, misses and bad records, the
refusals, and that a query is no frame."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
# torch BEFORE the device library is loaded, as bench.py does (see tests/test_gpu_rays.py)
import torch

import analytic_cases as A
import analytic_forms as F
import bsdf_cases as BC
import bsdf_forms as B
from conftest import GOLDEN
from gpu_checks import need_gpu

pytestmark = pytest.mark.gpu

FIELDS = ("f", "pdf", "s_wi", "s_f", "s_pdf", "s_type", "n_components", "le")
RT_RAYS_BLOCK = 256


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def open_scene(pkg, text):
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    return ps, pkg.DeviceScene(ps)


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(GOLDEN, "bsdf", name + ".npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the float64 forms on the fixture (for the exclusion mask and the reference's primitive): computed once per session"""
    fx = fixture(name)
    return BC.evaluate(name, fx, fx["answers"])


def query_tensors(fx, reps=1):
    t = lambda a: dev(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))
    return t(fx["rays"][fx["ridx"]]), t(fx["wi"]), t(fx["u"]), t(fx["flags"])


def same(a, b, *what):
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), what + (k,)


# ---------------------------------------------------------------------------------------------- 1. the reference's answers, per query
@pytest.mark.parametrize("name", list(BC.CASES))
def test_every_output_agrees_with_the_reference_per_query(pkg, name):
    """every float output within 4 x max(ref_err(case, output), the median ref_err of that output over the cases) of the reference's value in the
    measure of bsdf_forms.query_error -- ref_err being the reference's own largest error against the float64 forms, stored in the fixtures --;
    s_type and n_components equal; on the triangle-only cases the primitive hit is the reference's.  Only the queries the forms' geometric rule
    leaves out (at most 3 %) are not compared."""
    need_gpu(pkg)
    fx, w = fixture(name), expected(name)
    inc = ~w["excluded"]
    assert w["excluded"].mean() <= A.BAND_CAP
    median = np.median([fixture(c)["ref_err"] for c in BC.CASES], axis=0)
    ps, ds = open_scene(pkg, BC.product_text(fx["scene"]))
    rays, wi, u, flags = query_tensors(fx)
    hits = ds.intersect(rays, fields=())
    got = host(ds.bsdf(rays, hits, wi=wi, u=u, flags=flags))
    prim = hits["prim"].cpu().numpy()
    ds.close()
    ans = fx["answers"]
    assert np.array_equal(prim[inc] >= 0, w["hit"][inc]), name
    if BC.CASES[name]["triangles_only"]:
        assert np.array_equal(prim[inc], w["prim"][inc]), (name, int((prim[inc] != w["prim"][inc]).sum()))
    failed = []
    for i, k in enumerate(BC.OUTPUTS):
        bar = A.BAR_FACTOR * max(float(fx["ref_err"][i]), float(median[i]))
        e = B.query_error(got[k], BC.answer(ans, k), inc, unit_scale=(k == "s_wi"))[inc].max()
        print("BSDF-REF %s %-6s e %.3g bar %.3g (ref_err %.3g, median %.3g)" % (name, k, e, bar, fx["ref_err"][i], median[i]))
        if not e <= bar:
            failed.append((k, float(e), bar))
    for k in ("s_type", "n_components"):
        differ = int((got[k][inc] != BC.answer(ans, k)[inc]).sum())
        print("BSDF-REF %s %-12s differing %d of %d" % (name, k, differ, int(inc.sum())))
        if differ:
            failed.append((k, differ))
    assert not failed, (name, failed)


# ---------------------------------------------------------------------------------------------- 2. f in Whitted's light loop, bit for bit
HEAD = ('LookAt 0 0 -7 0 0 0 0 1 0\nCamera "perspective" "float fov" [50]\nFilm "image" "integer xresolution" [32] "integer yresolution" [32] "string filename" ["o.exr"]\n'
        'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\nPixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n')
def frame_text(surfaces, light, maxdepth):
    """a 32 x 32 Whitted frame (one unjittered sample per pixel) of bsdf_cases-style surfaces under one light"""
    out = [HEAD, 'SurfaceIntegrator "whitted" "integer maxdepth" [%d]\nWorldBegin\n%s\n' % (maxdepth, light)]
    for s in surfaces:
        out.append("AttributeBegin\n" + A._ctm_text(s.get("ctm", [])) + 'Material "%s" %s\n' % (s["material"][0], A._params(s["material"][1])) + A._mesh_text(s["shape"][1]) + "AttributeEnd\n")
    return "".join(out) + "WorldEnd\n"


def quad(cx, cy, cz, rx, ry, half, material):
    s = BC._quad(cx, cy, rx, ry, material, half=half)
    s["ctm"][0] = ("Translate", cx, cy, cz)
    return s


TRANSLUCENT = ("translucent", dict(Kd=(.6, .5, .4), Ks=(.3, .3, .3), reflect=(.6, .5, .5), transmit=(.4, .5, .6), roughness=.2))
# the light stands to the right of and behind the quads: the two on the left face it, ...
LIGHT_FRAME = frame_text([quad(-1.5, 1.5, 0, 10, -50, 1.3, ("plastic", dict(Kd=(.3, .3, .6), Ks=(.4, .4, .4), roughness=.1))),
                          quad(2.0, 1.9, 3, -15, -35, 1.7, TRANSLUCENT),
                          quad(-1.5, -1.5, 0, 5, 15, 1.3, TRANSLUCENT),        # ... this one shows the camera one side and the light the other: the transmission lobes answer
                          quad(2.0, -1.9, 3, 10, -60, 1.9, ("matte", dict(Kd=(.6, .7, .5), sigma=20)))],
                         'LightSource "distant" "point from" [6 2 1] "point to" [0 0 0] "color L" [3 2.5 2]', 0)


def dot32(a, b):
    """dot3 of rt_math.h in float32: a.x * b.x + a.y * b.y + a.z * b.z, left to right, every operation rounded (the build has -ffp-contract=off)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def test_f_composes_into_a_whitted_frame_bit_for_bit(pkg):
    """plastic, translucent (lit from the front and from behind) and Oren-Nayar quads under one unoccluded distant light, maxdepth 0: floats 0..2 of every
    camera sample's record are (f * L) * |dot(wi, ns)| (rt_integrate.h, Whitted's light loop: ln.pend, added to a black L), f from bsdf(), ns from
    intersect(), wi and L from the light's descriptor"""
    need_gpu(pkg)
    ps, ds = open_scene(pkg, LIGHT_FRAME)
    n = ps.n_camera_samples
    light = ps.lights()[0]
    wi, L = light["dir"].astype(np.float32), light["L"].astype(np.float32)
    ds.bind_film(); ds.clear_film(); ds.render()
    rec = ds.samples()[:, :3]
    rays = ds.camera_rays_device(0, n)
    hits = ds.intersect(rays, fields=("p", "ns", "ng", "material"))
    f = ds.bsdf(rays, hits, wi=dev(np.tile(wi, (n, 1))), fields=("f",))["f"].cpu().numpy()
    h = host(hits)
    hit = h["prim"] >= 0
    # the light is unoccluded but for a few samples: the frame's shadow ray (p, wi, RT_RAY_EPSILON, inf) asked again decides which
    shadow = torch.cat([hits["p"], dev(np.tile(wi, (n, 1))), torch.full((n, 1), float(np.float32(1e-3)), device="cuda"), torch.full((n, 1), float("inf"), device="cuda")], 1)
    blocked = ds.occluded(shadow.contiguous()).cpu().numpy() > 0
    ds.close()
    assert (blocked & hit).sum() < 20
    want = (f * L[None, :]) * np.abs(dot32(wi[None, :], h["ns"]))[:, None]
    want[blocked] = 0
    lit = hit & (np.abs(rec).max(-1) > 0)
    d = rays.cpu().numpy()[:, 3:6]
    through = hit & (dot32(wi[None, :], h["ng"]) * dot32(-d, h["ng"]) <= 0) & lit
    print("BSDF-WHITTED samples %d hit %d lit %d through the sheet %d materials %s" % (n, hit.sum(), lit.sum(), through.sum(), np.unique(h["material"][lit])))
    assert lit.sum() > 300 and through.sum() > 30 and len(np.unique(h["material"][lit])) >= 3
    assert np.array_equal(bits(rec[hit]), bits(want[hit].astype(np.float32))), int((bits(rec[hit]) != bits(want[hit])).any(-1).sum())
    assert not rec[~hit].any()


# ---------------------------------------------------------------------------------------------- 3. specular Sample_f in Whitted's mirror step
MIRROR_FRAME = frame_text([dict(shape=A.quad_mesh((-9, -2, -8, 9, -2, -8, 9, -2, 6, -9, -2, 6)), material=("matte", dict(Kd=(.7, .6, .5)))),
                           dict(shape=A.quad_mesh((-9, -2, 4, 9, -2, 4, 9, 9, 4, -9, 9, 4)), material=("matte", dict(Kd=(.4, .6, .7)))),
                           quad(-1.4, .3, 0, -35, 10, 1.2, ("mirror", dict(Kr=(.9, .9, .8)))),            # tilted down: it shows the camera the floor
                           quad(1.4, .3, 0, -30, -15, 1.2, ("glass", dict(Kr=(.9, .9, .9), Kt=(.8, .9, .9), index=1.5)))],
                          'LightSource "point" "point from" [0 5 -3] "color I" [60 50 40]', 1)


def test_specular_sample_f_composes_into_whitteds_mirror_step_bit_for_bit(pkg):
    """a mirror and a glass quad over a matte floor, before a matte wall, one point light, maxdepth 1: the record of a camera sample that hits the mirror is
    (child * s_f) * |dot(s_wi, ns)| (rt_integrate.h frame_pop onto a black L; pdf is 1) with s_wi, s_f from bsdf(flags = REFLECTION | SPECULAR) and
    child = radiance() of the ray (p, s_wi, RT_RAY_EPSILON, inf) at the same sample index; on the glass it is the reflection term, then the
    transmission term added.  Compared where both children end on a matte surface or leave the scene: there Li at depth 1 of the frame is Li of the
    query (neither recurses, neither draws)."""
    need_gpu(pkg)
    ps, ds = open_scene(pkg, MIRROR_FRAME)
    n = ps.n_camera_samples
    names = [m["type"] for m in ps.materials()]
    ds.bind_film(); ds.clear_film(); ds.render()
    rec = ds.samples()[:, :3]
    rays = ds.camera_rays_device(0, n)
    hits = ds.intersect(rays, fields=("p", "ns", "material"))
    u = torch.full((n, 3), .5, dtype=torch.float32, device="cuda")
    terms, ends_matte = {}, np.ones(n, bool)
    for lobe in (pkg.BSDF_REFLECTION, pkg.BSDF_TRANSMISSION):
        s = ds.bsdf(rays, hits, u=u, flags=torch.full((n,), lobe | pkg.BSDF_SPECULAR, dtype=torch.int32, device="cuda"), fields=("s_wi", "s_f", "s_pdf", "s_type"))
        sampled = s["s_pdf"] > 0
        child = rays.clone()                                                            # (a sample without this lobe keeps its camera ray: its term is not read)
        child[:, 0:3] = torch.where(sampled[:, None], hits["p"], rays[:, 0:3])
        child[:, 3:6] = torch.where(sampled[:, None], s["s_wi"], rays[:, 3:6])
        child[:, 6] = torch.where(sampled, torch.full_like(s["s_pdf"], float(np.float32(1e-3))), rays[:, 6])         # RAY_EPSILON core/pbrt.h:211
        child[:, 7] = torch.where(sampled, torch.full_like(s["s_pdf"], float("inf")), rays[:, 7])
        Li = ds.radiance(child.contiguous(), first=0)[:, :3].cpu().numpy()
        end = ds.intersect(child.contiguous(), fields=("material",))
        end_mat = end["material"].cpu().numpy()
        sm = sampled.cpu().numpy()
        ends_matte &= ~sm | (end_mat < 0) | np.array([names[m] == "matte" if m >= 0 else True for m in end_mat])
        ad = np.abs(dot32(s["s_wi"].cpu().numpy(), hits["ns"].cpu().numpy()))
        term = (Li * s["s_f"].cpu().numpy()) * ad[:, None]
        assert (s["s_pdf"].cpu().numpy()[sm] == 1).all() and (s["s_type"].cpu().numpy()[sm] == (lobe | pkg.BSDF_SPECULAR)).all()
        terms[lobe] = np.where(sm[:, None], term, np.float32(0)).astype(np.float32)
    mat = hits["material"].cpu().numpy()
    ds.close()
    mirror = np.array([m >= 0 and names[m] == "mirror" for m in mat]) & ends_matte
    glass = np.array([m >= 0 and names[m] == "glass" for m in mat]) & ends_matte
    want = (np.float32(0) + terms[pkg.BSDF_REFLECTION]) + terms[pkg.BSDF_TRANSMISSION]
    print("BSDF-MIRROR samples %d mirror %d (non-black %d) glass %d (non-black %d)" % (n, mirror.sum(), (np.abs(rec[mirror]).max(-1) > 0).sum(), glass.sum(),
                                                                                     (np.abs(rec[glass]).max(-1) > 0).sum()))
    assert (np.abs(rec[mirror]).max(-1) > 0).sum() > 40 and (np.abs(rec[glass]).max(-1) > 0).sum() > 40
    assert not terms[pkg.BSDF_TRANSMISSION][mirror].any()
    assert np.array_equal(bits(rec[mirror]), bits(want[mirror])), int((bits(rec[mirror]) != bits(want[mirror])).any(-1).sum())
    assert np.array_equal(bits(rec[glass]), bits(want[glass])), int((bits(rec[glass]) != bits(want[glass])).any(-1).sum())


# ---------------------------------------------------------------------------------------------- 4. sampling agrees with f
def sphere_quadrature(fn, n_theta):
    """midpoint rule in (cos theta, phi) over the sphere: sum fn(wi) * 4 pi / N"""
    nphi = 2 * n_theta
    ct = (np.arange(n_theta) + .5) / n_theta * 2 - 1
    ph = (np.arange(nphi) + .5) / nphi * 2 * np.pi
    ct, ph = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1 - ct * ct)
    wi = np.stack([st * np.cos(ph), st * np.sin(ph), ct], -1).reshape(-1, 3)
    return fn(wi).sum(0) * 4 * np.pi / len(wi)


def test_sampling_agrees_with_f(pkg):
    """per non-specular material of gallery_flat, at one hit: a 64 x 64 stratified grid of (u1, u2) per non-specular lobe, the lobe asked for by its own
    BxDFType as flags; the mean of s_f |cos| / s_pdf over a lobe's grid (a failed sample counts 0) estimates the integral of that lobe's f |cos| over the
    sphere, and the sum over the lobes that of the material's f |cos|, which a float64 midpoint quadrature of analytic_forms.Material.f gives; they agree
    within six standard errors of the sum plus the quadrature's own error (its distance from the same rule at half the resolution).
    (One lobe per call on purpose: with several lobes matching, Sample_f adds the other lobes' Pdf, and BRDFToBTDF::Pdf asks its BRDF at -wi,
    reflection.cpp:231-234, where its Sample_f mirrors the drawn direction in z only, :67-72 -- for translucent's glossy transmission the averaged pdf is
    then not the density the directions were drawn with, in the reference as here, and the joint estimate is off by 8 %: .725 against .669 in red.)"""
    need_gpu(pkg)
    fx, w = fixture("gallery_flat"), expected("gallery_flat")
    sc, mats, _ = BC.form("gallery_flat")
    ps, ds = open_scene(pkg, BC.product_text(fx["scene"]))
    rays_all = fx["rays"][fx["ridx"]]
    r64 = fx["rays"].astype(np.float64)
    surf = sc.closest(r64[:, 0:3], r64[:, 3:6], r64[:, 6], r64[:, 7])[2][fx["ridx"]]
    g = (np.arange(64) + .5) / 64
    u1, u2 = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    u = np.stack([u1, u2, np.full(len(u1), .5)], -1).astype(np.float32)
    n = len(u)
    checked = 0
    for s, (kind, kw, _) in enumerate(mats):
        lobes = [l.type for l in B.material_lobes(kind, kw, 1) if not l.type & B.SPECULAR]
        if not lobes:
            continue                                                 # mirror, glass
        i = np.flatnonzero((surf == s) & ~w["excluded"] & w["hit"])
        i = i[len(i) // 2]                                           # a query in the middle of the quad's share of the frame
        rays = dev(rays_all[i:i + 1]).repeat(n, 1).contiguous()
        hits = ds.intersect(rays, fields=("ns",))
        ns = hits["ns"].cpu().numpy().astype(np.float64)
        mean, var = np.zeros(3), np.zeros(3)
        for lobe in lobes:
            out = host(ds.bsdf(rays, hits, u=dev(u), flags=dev(np.full(n, lobe, np.int32)), fields=("s_wi", "s_f", "s_pdf", "s_type", "n_components")))
            assert (out["n_components"] == 1).all() and set(np.unique(out["s_type"])) <= {0, lobe}, (kind, lobe)
            ok = out["s_pdf"] > 0
            cos = np.abs((out["s_wi"].astype(np.float64) * ns).sum(-1))
            with np.errstate(all="ignore"):
                est = np.where(ok[:, None], out["s_f"].astype(np.float64) * (cos / out["s_pdf"])[:, None], 0.0)
            mean += est.mean(0)
            var += est.var(0, ddof=1) / n
        se = np.sqrt(var)
        wo, nrm = -rays_all[i, 3:6].astype(np.float64), ns[0]
        material = F.Material(kind, **kw)
        integrand = lambda wi: material.f(np.broadcast_to(wo, wi.shape), wi, np.broadcast_to(nrm, wi.shape)) * np.abs(wi @ nrm)[:, None]
        fine, coarse = sphere_quadrature(integrand, 384), sphere_quadrature(integrand, 192)
        qerr = np.abs(fine - coarse)
        print("BSDF-SAMPLING %-11s lobes %d mean %s quadrature %s 6 se %s quadrature error %s" % (kind, len(lobes), mean, fine, 6 * se, qerr))
        assert (np.abs(mean - fine) <= 6 * se + qerr).all(), (kind, mean, fine, se, qerr)
        checked += 1
    ds.close()
    assert checked == 6


# ---------------------------------------------------------------------------------------------- 5. launch shapes, single outputs, flags = NULL
def test_launch_shapes_single_outputs_and_null_flags(pkg):
    """the first n rows of one n = 4096 call for n = 1, 63, 64, 65, RT_RAYS_BLOCK +- 1 and 4096, bit for bit; each of the eight outputs asked for alone;
    flags = None against an array of BSDF_ALL; and more queries than resident lanes on the textured scene (a lane then takes several queries and
    resolves each one's material into its one record): every copy of the 4096 answers the same"""
    need_gpu(pkg)
    for name in ("gallery_flat", "gallery_textured"):
        fx = fixture(name)
        ps, ds = open_scene(pkg, BC.product_text(fx["scene"]))
        reps = -(-4096 // len(fx["ridx"]))
        rays, wi, u, flags = (t[:4096].contiguous() for t in query_tensors(fx, reps))
        hits = ds.intersect(rays, fields=())
        rec = torch.stack([hits["prim"].view(torch.float32), hits["t"], hits["b1"], hits["b2"]], 1).contiguous()
        full = host(ds.bsdf(rays, rec, wi=wi, u=u, flags=flags))
        assert set(full) == set(FIELDS) and (full["n_components"] > 0).sum() > 1000
        for n in (1, 63, 64, 65, RT_RAYS_BLOCK - 1, RT_RAYS_BLOCK, RT_RAYS_BLOCK + 1, 4096):
            part = host(ds.bsdf(rays[:n].contiguous(), rec[:n].contiguous(), wi=wi[:n].contiguous(), u=u[:n].contiguous(), flags=flags[:n].contiguous()))
            same(part, {k: v[:n] for k, v in full.items()}, name, n)
        for k in FIELDS:
            one = host(ds.bsdf(rays, rec, wi=wi if k in ("f", "pdf") else None, u=u if k.startswith("s_") else None, flags=flags, fields=(k,)))
            assert list(one) == [k]
            same(one, {k: full[k]}, name, "alone")
        every = torch.full_like(flags, pkg.BSDF_ALL)
        same(host(ds.bsdf(rays, rec, wi=wi, u=u, flags=None)), host(ds.bsdf(rays, rec, wi=wi, u=u, flags=every)), name, "flags = None")
        if name == "gallery_textured":
            big = 161                                                # 161 x 4096 = 659 456 queries: above the 2048 threads x 256 CUs a device keeps resident
            tile = lambda t: t.repeat((big,) + (1,) * (t.dim() - 1)).contiguous()
            many = host(ds.bsdf(tile(rays), tile(rec), wi=tile(wi), u=tile(u), flags=tile(flags)))
            for k, v in many.items():
                v = v.reshape((big, 4096) + v.shape[1:])
                assert np.array_equal(bits(v), bits(np.broadcast_to(full[k], v.shape))), (name, "many", k)
        ds.close()


# ---------------------------------------------------------------------------------------------- 6. misses and bad records
def test_misses_and_bad_records_give_zeros_and_leave_their_neighbours_alone(pkg):
    need_gpu(pkg)
    fx = fixture("gallery_emitters")
    ps, ds = open_scene(pkg, BC.product_text(fx["scene"]))
    rays, wi, u, flags = query_tensors(fx)
    n = len(rays)
    hits = ds.intersect(rays, fields=())
    rec = torch.stack([hits["prim"].view(torch.float32), hits["t"], hits["b1"], hits["b2"]], 1).contiguous()
    base = host(ds.bsdf(rays, rec, wi=wi, u=u, flags=flags))
    prim = hits["prim"].cpu().numpy()
    assert 0 < (prim < 0).sum() < n and np.abs(base["le"]).max() > 0
    for k, v in base.items():
        assert not v[prim < 0].any(), k                              # the scene's own misses, interleaved with its hits
    bad = prim.copy()
    bad[::3] = -1
    bad[1::5] = ps.n_tris + np.arange(len(bad[1::5]))                # beyond the scene
    bad[2::7] = np.iinfo(np.int32).min
    rec2 = rec.clone()
    rec2[:, 0] = dev(bad.astype(np.int32)).view(torch.float32)
    got = host(ds.bsdf(rays, rec2, wi=wi, u=u, flags=flags))
    ds.close()
    changed = bad != prim
    assert changed.sum() > n // 3
    for k, v in got.items():
        assert not v[changed | (prim < 0)].any(), k
        assert np.array_equal(bits(v[~changed]), bits(base[k][~changed])), k


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_name_the_function_and_launch_nothing(pkg):
    need_gpu(pkg)
    fx = fixture("gallery_flat")
    ps, ds = open_scene(pkg, BC.product_text(fx["scene"]))
    L = pkg.hip_lib()
    rays, wi, u, flags = (t[:64].contiguous() for t in query_tensors(fx))
    hits = ds.intersect(rays, fields=())
    rec = torch.stack([hits["prim"].view(torch.float32), hits["t"], hits["b1"], hits["b2"]], 1).contiguous()
    out = {k: torch.zeros((64, 3), dtype=torch.float32, device="cuda") for k in ("f", "s_wi", "s_f", "le")}
    out.update({k: torch.zeros(64, dtype=torch.float32, device="cuda") for k in ("pdf", "s_pdf")})
    out.update({k: torch.zeros(64, dtype=torch.int32, device="cuda") for k in ("s_type", "n_components")})
    torch.cuda.synchronize()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    Q = lambda **kw: pkg.RtBsdfQuery(**{k: v.data_ptr() for k, v in kw.items()})
    whole = Q(wi=wi, u=u, flags=flags, **out)
    cases = (((None, p(rays), p(rec), 64, whole), ("null scene",)),
             ((ds._s, None, p(rec), 64, whole), ("null ray pointer",)),
             ((ds._s, p(rays), None, 64, whole), ("null hit pointer",)),
             ((ds._s, p(rays), p(rec), 64, None), ("null RtBsdfQuery",)),
             ((ds._s, p(rays), p(rec), 64, Q(wi=wi, u=u, flags=flags)), ("every output", "null")),
             ((ds._s, p(rays), p(rec), 64, Q(u=u, f=out["f"])), ("f or pdf", "wi is null")),
             ((ds._s, p(rays), p(rec), 64, Q(u=u, pdf=out["pdf"])), ("f or pdf", "wi is null")),
             ((ds._s, p(rays), p(rec), 64, Q(wi=wi, s_f=out["s_f"])), ("s_wi, s_f, s_pdf or s_type", "u is null")),
             ((ds._s, p(rays), p(rec), 64, Q(wi=wi, s_type=out["s_type"])), ("s_wi, s_f, s_pdf or s_type", "u is null")),
             ((ds._s, p(rays, 4), p(rec), 8, whole), ("dev_rays", "16-byte aligned")),
             ((ds._s, p(rays), p(rec, 8), 8, whole), ("dev_hits", "16-byte aligned")),
             ((ds._s, p(rays), p(rec), 2 ** 30 + 1, whole), ("above 2^30",)))
    for args, words in cases:
        q = args[4]
        assert L.rt_bsdf_device(args[0], args[1], args[2], args[3], C.byref(q) if q is not None else None) == -1, words          # RT_EINVAL
        msg = L.rt_last_error().decode()
        assert "rt_bsdf_device" in msg and all(wd in msg for wd in words), msg
    assert L.rt_bsdf_device(ds._s, None, None, 0, None) == 0                                    # n == 0: RT_OK, nothing launched
    assert L.rt_bsdf_device(ds._s, p(rays), p(rec), 0, C.byref(whole)) == 0
    ds.sync()
    assert all(not t.any().item() for t in out.values())                                      # nothing was launched: nothing was written
    # the wrapper's own checks
    for kw, word in ((dict(fields=("f",)), "wi"), (dict(fields=("s_f",)), "u"), (dict(fields=("nope",)), "unknown field"), (dict(fields=()), "at least one"),
                     (dict(wi=wi.double(), fields=("f",)), "float32"), (dict(wi=wi[:, :2].contiguous(), fields=("f",)), "shape"),
                     (dict(wi=wi.cpu(), fields=("f",)), "is on"), (dict(flags=flags.float(), fields=("le",)), "int32")):
        with pytest.raises(ValueError) as e:
            ds.bsdf(rays, hits, **kw)
        assert word in str(e.value), (kw.keys(), str(e.value))
    assert ds.bsdf(rays[:0].contiguous(), rec[:0].contiguous(), fields=("le", "n_components"))["n_components"].shape == (0,)
    ds.close()


# ---------------------------------------------------------------------------------------------- 8. a query is not a frame
def test_a_query_leaves_the_last_frame_as_it_was(pkg):
    """film, samples(), counters() and last_stats() after bsdf() calls on a rendered scene with textured materials (whose resolved records share the
    frames' pool), bitwise; then a second render() gives the first film"""
    need_gpu(pkg)
    fx = fixture("gallery_textured")
    ps, ds = open_scene(pkg, BC.product_text(fx["scene"]))
    ds.bind_film(); ds.set_counting(True); ds.clear_film(); ds.reset_counters()
    ds.render()
    film, samples, cnt, stats = ds.film_accum(), ds.samples(), ds.counters(), ds.last_stats()
    rays, wi, u, flags = query_tensors(fx)
    hits = ds.intersect(rays, fields=())
    cnt_hits = ds.counters()                                         # (the trace counts; the query must not)
    first = host(ds.bsdf(rays, hits, wi=wi, u=u, flags=flags))
    for _ in range(2):
        same(host(ds.bsdf(rays, hits, wi=wi, u=u, flags=flags)), first, "repeat")
        ds.sync()
        assert np.array_equal(bits(ds.film_accum()), bits(film)) and np.array_equal(bits(ds.samples()), bits(samples))
        assert ds.counters() == cnt_hits and ds.last_stats() == stats
    ds.clear_film(); ds.reset_counters()
    ds.render()
    assert np.array_equal(bits(ds.film_accum()), bits(film)) and np.array_equal(bits(ds.samples()), bits(samples)) and ds.counters() == cnt
    same(host(ds.bsdf(rays, hits, wi=wi, u=u, flags=flags)), first, "after a frame")
    ds.close()
