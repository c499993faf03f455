"""The device's per-sample radiance against float64: lights, BSDF lobes, quadrics, the mirror step and the homogeneous medium, one term per
case (tests/analytic_cases.py).  Under SurfaceIntegrator "whitted" with delta lights no random number enters a sample's radiance, so every
record of DeviceScene.samples() (rt_samples_read: radiance, alpha and image position of each camera sample before filtering) is one
evaluation of f(wo, wi) Li |cos| that tests/analytic_forms.py computes in float64 from the record's own image position: 4 225 unjittered
and 16 900 jittered positions per case, the extra row and column of the sample extent included.

The error of a sample is e = max_c |got - L| / (max_c |L| + 0.01 Lcase) (analytic_forms.sample_error); samples within 0.02 pixel of a
discontinuity of the float64 scene (analytic_forms.band) are left out, at most 3 % per case and never by the size of an error; a sample
passes if e <= 4 max(ref_err(case), median ref_err of the case's family), ref_err being the UNMODIFIED reference's own largest e on the
fixture's film (tests/golden/analytic/, tests/test_analytic_host.py).  The films go against the fixtures' films under the strict bar of
tests/test_gpu_parity.py, every pixel within 1e-5, on every case, quadrics included, outside the fixture's band.

The "geometry" cases hold the debug integrator's records (u, v, |ng|, |ns|, the hit mask of each camera sample, alpha exactly 1) to the float64 meshes
and quadrics, the "textures" cases a Whitted sample of a surface whose material is resolved from a Texture graph at the hit: same measure, band and bars.

The "march" cases (VolumeIntegrator "emission" / "single" through homogeneous, exponential and volumegrid regions: march_begin, march_steps, density_at,
density_tau, the pipeline's march kernel) draw random offsets, so a record is held to the exact float64 integral within the allowance D that bounds what ANY
offset can do: e' = max_c max(0, |got - L| - D) over the same scale, under 4 max(ref_err, the family's median, medium_homogeneous's ref_err).  Their films stay
under the strict bar against the reference's films (rendered with the same keyed random numbers), and a camera ray that hits nothing carries Lv at alpha 0."""
import os

import numpy as np
import pytest

import analytic_cases as A
import analytic_forms as F
from conftest import GOLDEN, film_metrics
from gpu_checks import need_gpu

pytestmark = pytest.mark.gpu

NAMES = list(A.CASES)
FLAVOUR_CASES = ["plastic_rough_.02", "quadric_hyperboloid", "medium_homogeneous",       # one lobe, one quadric, the medium,
                 "geom_mesh_n_shading", "tex_mix_depth4",                                 # one debug frame, one textured frame,
                 "march_single_forward", "dens_grid_single_thin"]                         # a march through a homogeneous and through a density region


def load(name):
    z = np.load(os.path.join(GOLDEN, "analytic", name + ".npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ref_errs():
    return {n: float(load(n)["ref_err"]) for n in NAMES}


def check_film(name, rgb, alpha, g):
    """The strict bar of the parity tests (conftest.film_metrics: every pixel within 1e-5, colour and alpha) for EVERY case, quadrics included;
    a pixel is its one sample, so the pixels of the fixture's band (a discontinuity within 0.02 pixel, where the device's atan2f may decide a
    clip edge otherwise than glibc's; at most 3 % by the fixture's cap) are left out."""
    inc = ~g["band"]
    assert g["band"].mean() <= A.BAND_CAP
    m = film_metrics(rgb[inc], g["rgb"][inc])
    da = float(np.abs(alpha - g["alpha"])[inc].max())
    print("ANALYTIC-FILM", name, m, "alpha maxabs %.3g" % da, "band pixels", int(g["band"].sum()))
    assert np.isfinite(rgb).all(), name
    assert m["maxabs"] <= 1e-5, (name, m)
    assert da <= 1e-5, name


def check_samples(name, label, rec, bar):
    """the records of one render against the float64 form at each record's own image position"""
    sc = A.form(name)
    ix, iy = rec[:, 4].astype(np.float64), rec[:, 5].astype(np.float64)
    if A.CASES[name]["family"] == "march":   # D: the allowance of a "march" case (what any draw of its march can do), None elsewhere
        L, D, hit, _ = sc.allowance(ix, iy)
    else:
        (L, hit, _), D = sc.samples(ix, iy), None
    band = F.band(sc, ix, iy)
    inc = ~band
    e = F.sample_error(rec[:, 0:3], L, inc, D)
    worst = int(np.argmax(np.where(inc, e, -1)))
    print("ANALYTIC-SAMPLES %s %s n %d band %.4f max_e %.3g bar %.3g at (%.2f, %.2f) got %s want %s" %
          (name, label, len(rec), band.mean(), e[inc].max(), bar, ix[worst], iy[worst], rec[worst, 0:3], L[worst]))
    if D is not None:
        # the allowance cannot hide a failure: it stays under 5 % of the sample's scale on 90 % of the samples at these positions too; sky samples carry Lv
        tight, used, sky = A.tight_share(L, D, inc), A.tightness(rec[:, 0:3], L, D, inc), inc & (hit == 0)
        print("ANALYTIC-ALLOWANCE %s %s tight share %.3f largest |got - L| / D %.3f sky samples %d with Lv %d" % (name, label, tight, used, int(sky.sum()), int((L[sky] > 0).any(-1).sum())))
        assert tight >= A.MIN_TIGHT_SHARE, (name, label, tight)
        assert np.array_equal((rec[sky, 0:3] > 0).any(-1), (L[sky] > 0).any(-1)), (name, label, "a camera ray that hits nothing does not carry the form's Lv")
    assert np.isfinite(rec[:, 0:4]).all(), name
    assert band.mean() <= A.BAND_CAP, (name, label, band.mean())
    assert np.array_equal(rec[inc, 3], hit[inc].astype(np.float32)), (name, label, "alpha is not exactly 1 on hits and 0 on misses")
    if A.CASES[name]["family"] == "geometry":            # a debug frame: 1 for every sample, misses and the band included
        assert (rec[:, 3] == 1).all(), (name, label, "a debug sample's alpha is not exactly 1")
    assert e[inc].max() <= bar, (name, label, float(e[inc].max()), bar, int((e[inc] > bar).sum()))
    return float(e[inc].max())


def test_fixtures_present():
    assert all(os.path.exists(os.path.join(GOLDEN, "analytic", n + ".npz")) for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_film_and_unjittered_samples(pkg, ref_errs, name):
    """The fixture's scene at the same unjittered samples: the film against the reference's film, every sample record (the row and column off
    the film included) against float64, and the timed kernels' records bit-identical to the counting twins'."""
    need_gpu(pkg)
    g = load(name)
    ps = pkg.ParsedScene(text=str(g["scene"]))
    assert ps.valid and ps.errors == 0
    assert ps.sample_extent == (0, A.RES + 1, 0, A.RES + 1) and ps.spp == 1
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    rec = ds.samples()
    cnt = ds.counters()
    ds.set_counting(False); ds.clear_film(); ds.render()
    timed = ds.samples()
    ds.close()
    assert cnt["bad_samples"] == 0 and cnt["camera_rays"] == (A.RES + 1) ** 2, cnt
    cx, cy = A.pixel_centres()
    assert np.array_equal(np.sort(rec[:, 4] + 1000 * rec[:, 5]), np.sort((cx + 1000 * cy).ravel().astype(np.float32)))
    check_film(name, rgb, alpha, g)
    check_samples(name, "unjittered", rec, A.bar(name, ref_errs))
    assert np.array_equal(timed, rec), (name, "the timed kernels' sample records differ from the counting twins'")


@pytest.mark.parametrize("name", NAMES)
def test_jittered_samples(pkg, ref_errs, name):
    """The same scene under stratified 2 x 2 jittered samples from the keyed seed: 16 900 positions nobody chose, same bars, the band
    recomputed at those positions under the same cap."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=A.scene_text(name, jitter=True))
    assert ps.valid and ps.errors == 0 and ps.spp == 4
    ds = pkg.DeviceScene(ps)
    ds.render()
    rec = ds.samples()
    cnt = ds.counters()
    ds.close()
    assert cnt["bad_samples"] == 0 and len(rec) == 4 * (A.RES + 1) ** 2
    frac = rec[:, 4:6] - np.floor(rec[:, 4:6])
    assert len(np.unique(frac)) > len(rec), "the samples are not jittered"
    check_samples(name, "jittered", rec, A.bar(name, ref_errs))


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_forced_flavours_give_the_same_records(pkg, name, monkeypatch):
    """The queue pipeline and both occupancy flavours of the timed megakernel give, sample by sample (matched by image position), the
    bit-identical records of the default flavour.  A debug frame always runs its own megakernel and reports pipeline 0."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=A.scene_text(name, jitter=True))
    ds = pkg.DeviceScene(ps)

    def records():
        ds.render()
        r = ds.samples()
        return r[np.lexsort((r[:, 4], r[:, 5]))]

    monkeypatch.setenv("PBRT_HIP_PIPELINE", "0")
    ds.set_counting(False)
    ref = records()
    assert len(np.unique(ref[:, 4:6], axis=0)) == len(ref)
    for occ in ("0", "1"):
        monkeypatch.setenv("PBRT_HIP_HIGH_OCC", occ)
        got = records()
        assert np.array_equal(got, ref), (name, "PBRT_HIP_HIGH_OCC=" + occ, float(np.abs(got - ref).max()))
    monkeypatch.delenv("PBRT_HIP_HIGH_OCC")
    monkeypatch.setenv("PBRT_HIP_PIPELINE", "1")
    for counting in (False, True):
        ds.set_counting(counting)
        got = records()
        assert ds.last_stats()["pipeline"] == (0 if A.CASES[name]["family"] == "geometry" else 1)
        assert np.array_equal(got, ref), (name, "PBRT_HIP_PIPELINE=1", counting, float(np.abs(got - ref).max()))
    ds.close()


F32_HALF_ULP = 2.0 ** -24      # a float32 result cannot be nearer to float64 than its own rounding


def camera_deviation(rays, cam, ix, iy):
    """(o relative to the largest |o|, d absolute) of float32 camera rays from the float64 camera at the image positions (ix, iy)"""
    o, d, mint, maxt = cam.rays(ix, iy)
    return (float(np.abs(rays["o"].astype(np.float64) - o).max() / max(np.abs(o).max(), 1e-30)), float(np.abs(rays["d"].astype(np.float64) - d).max()),
            mint.astype(np.float32), maxt.astype(np.float32))


def test_camera_rays_against_the_float64_cameras(pkg):
    """rt_camera_rays of the perspective (square and 3:2), the orthographic (with a screen window), the environment and the thin-lens camera
    (lensradius .4, focaldistance 11; the unjittered 1 x 1 sampler's lens sample is the lens centre) against the float64 cameras: o and d
    within 4 x the deviation of the REFERENCE's own rays from the same form (the probe fixtures: probe_cornell for the pinhole,
    tests/golden/analytic/probe_* for the other three), never below float32's own rounding; mint equal, maxt to float32 rounding."""
    need_gpu(pkg)
    from conftest import load_golden
    pc = load_golden("probe_cornell")
    prec = pc["records"]
    ref_cam = F.Camera("perspective", 24, 24, F.look_at((278, 273, -800), (278, 273, 0), (0, 1, 0)), fov=39.3)
    px, py = A.pixel_centres(24, 24)
    ref_rays = np.zeros(len(prec), pkg.RAY_DTYPE)
    ref_rays["o"], ref_rays["d"] = prec[:, 0:3], prec[:, 3:6]
    persp_o, persp_d, _, _ = camera_deviation(ref_rays, ref_cam, px.ravel(), py.ravel())
    assert persp_o < 1e-6 and persp_d < 1e-6, (persp_o, persp_d)      # the form is the reference's perspective camera
    wide = dict(A.CASES["light_point"]["camera"], res=(96, 64))
    todo = [("perspective 64 x 64", A.scene_text("light_point"), A.camera_form(A.CASES["light_point"]["camera"]), (64, 64), persp_o, persp_d),
            ("perspective 96 x 64", A.scene_text("light_point").replace('"integer xresolution" [64]', '"integer xresolution" [96]'), A.camera_form(wide), (96, 64),
             persp_o, persp_d)]
    for name in A.PROBES:
        g = load(name)
        todo.append((name, str(g["scene"]).replace('SurfaceIntegrator "probe"', 'SurfaceIntegrator "whitted"'), A.camera_form(A.PROBES[name]["camera"]),
                     A.PROBES[name]["camera"]["res"], float(g["dev_o"]), float(g["dev_d"])))
    for label, text, cam, (xres, yres), dev_o, dev_d in todo:
        ps = pkg.ParsedScene(text=text)
        assert ps.valid and ps.errors == 0 and (ps.width, ps.height) == (xres, yres)
        ds = pkg.DeviceScene(ps)
        n = (xres + 1) * (yres + 1)
        assert ps.n_camera_samples == n
        rays = ds.camera_rays(0, n)
        ds.close()
        ix, iy = A.pixel_centres(xres, yres)
        got_o, got_d, mint, maxt = camera_deviation(rays, cam, ix.ravel(), iy.ravel())
        bar_o, bar_d = max(A.BAR_FACTOR * dev_o, F32_HALF_ULP), max(A.BAR_FACTOR * dev_d, F32_HALF_ULP)
        print("ANALYTIC-CAMERA %s o %.3g (bar %.3g) d %.3g (bar %.3g)" % (label, got_o, bar_o, got_d, bar_d))
        assert got_o <= bar_o and got_d <= bar_d, (label, got_o, bar_o, got_d, bar_d)
        assert np.array_equal(rays["mint"], mint), label
        assert np.allclose(rays["maxt"], maxt, rtol=2 * F32_HALF_ULP * A.BAR_FACTOR, atol=0), label


@pytest.mark.parametrize("name", list(A.PROBES))
def test_probe_rays_through_every_quadric(pkg, name):
    """rt_trace_closest on the REFERENCE's own camera rays of the three camera probes (one of every quadric, partial, rotated, two under a
    non-uniform scale): outside the band of analytic_forms.ray_band (a clip edge or a silhouette within 3e-4 rad, where the device's atan2f
    may decide otherwise than glibc's) hit or miss is the reference's and t is the reference's bit for bit."""
    need_gpu(pkg)
    g = load(name)
    rec, band = g["records"], g["band"]
    assert band.mean() <= A.BAND_CAP
    ps = pkg.ParsedScene(text=str(g["scene"]).replace('SurfaceIntegrator "probe"', 'SurfaceIntegrator "whitted"'))
    ds = pkg.DeviceScene(ps)
    rays = np.zeros(len(rec), pkg.RAY_DTYPE)
    rays["o"], rays["d"], rays["mint"], rays["maxt"] = rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7]
    hits = ds.trace_closest(rays)
    own = ds.camera_rays(0, len(rec))
    ds.close()
    # the device's own camera rays start where the reference's do, bit for bit (as tests/test_gpu_parity.py holds the top-level probes)
    assert np.array_equal(own["o"], rec[:, 0:3]) and np.array_equal(own["mint"], rec[:, 6]), name
    inc = ~band
    hit = rec[:, 8] > 0
    print("ANALYTIC-PROBE %s rays %d hits %d band %.4f hit differs %d t differs %d" % (name, len(rec), int(hit.sum()), band.mean(),
          int(((hits["prim"] >= 0) != hit)[inc].sum()), int((hits["t"] != rec[:, 9])[inc & hit].sum())))
    assert np.array_equal((hits["prim"] >= 0)[inc], hit[inc])
    assert np.array_equal(hits["t"][inc & hit], rec[inc & hit, 9])
