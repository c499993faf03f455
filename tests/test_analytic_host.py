"""The proof that the float64 forms of tests/analytic_forms.py are the reference's functions: from the fixtures of tests/golden/analytic/
alone (films of the UNMODIFIED reference, tests/golden/make_analytic_golden.py) the band and ref_err are recomputed and must equal what is
stored, the band stays under its cap, the reference's film outside the band is within ref_err of the form, and every case's wrong twin
is rejected by its fixture (at least 5 % of the included samples beyond 10 x the case's bar); the "geometry" cases (SurfaceIntegrator "debug":
u, v, normals, hit mask) and the "textures" cases go through the same tests, a debug frame's alpha being 1 on every pixel; the three camera probes (orthographic,
environment and thin-lens camera, every quadric) give the forms' rays, t, hit point, normal and (u, v).  The "march" cases (volume integrators and
density media, whose marches draw random numbers) are held to the form within its allowance D: ref_err is the reference's largest excess over D; D
stays small against the sample's scale, every twin lies beyond its allowance, and the bound behind D (rule 1: Tau against the integral) is checked on
seeded rays and offsets by a plain restatement of Tau's loop.  No GPU, no package: numpy only."""
import os

import numpy as np
import pytest

import analytic_cases as A
import analytic_forms as F
from conftest import GOLDEN

NAMES = list(A.CASES)


def load(name):
    z = np.load(os.path.join(GOLDEN, "analytic", name + ".npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def measured():
    """every fixture against its form, once"""
    out = {}
    for name in NAMES:
        g = load(name)
        out[name] = (g, A.measure(name, g["rgb"], g["alpha"]))
    return out


def test_every_case_has_its_fixture_and_the_table_covers_the_families():
    have = sorted(os.path.basename(p)[:-4] for p in os.listdir(os.path.join(GOLDEN, "analytic")) if p.endswith(".npz") and not p.startswith("probe_"))
    assert have == sorted(NAMES)
    assert {c["family"] for c in A.CASES.values()} == set(A.FAMILIES)
    assert len(NAMES) >= 29
    assert sum(c["family"] == "geometry" for c in A.CASES.values()) >= 13 and sum(c["family"] == "textures" for c in A.CASES.values()) >= 13


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_the_table_s_scene_and_band_and_ref_err_are_reproduced(measured, name):
    g, m = measured[name]
    assert str(g["scene"]) == A.scene_text(name)
    assert g["rgb"].shape == (A.RES, A.RES, 3) and g["rgb"].dtype == np.float32
    assert np.array_equal(m["band"], g["band"])
    # (equal up to float64 rounding in another numpy / BLAS: ref_err is a difference of numbers of order 1 carried to 1e-16)
    # (a march case's ref_err is an excess over the allowance, |got - L| - D over the scale: the difference of two numbers 1e-2 of the scale apart)
    slack = 1e-12 if A.CASES[name]["family"] == "march" else 0.0
    assert m["band_share"] == float(g["band_share"]) and abs(m["ref_err"] - float(g["ref_err"])) <= 1e-6 * float(g["ref_err"]) + slack


@pytest.mark.parametrize("name", NAMES)
def test_band_is_under_the_cap_and_the_reference_film_is_within_ref_err(measured, name):
    g, m = measured[name]
    assert m["band_share"] <= A.BAND_CAP
    inc = ~m["band"]
    assert m["e"][inc].max() <= float(g["ref_err"]) * (1 + 1e-6)
    # alpha is exactly 1 on hits and 0 on misses outside the band; a geometry case: exactly 1 on EVERY pixel, and its `hit` channel, where it has
    # one, is the form's hit mask outside the band (analytic_cases.measure)
    assert m["alpha_equal"]
    if A.CASES[name]["family"] == "geometry":
        assert (g["alpha"] == 1).all()
    assert m["falloff_share"] >= A.CASES[name].get("min_falloff_share", 0)
    assert 0.05 <= m["hit_share"] < 1.0                       # hits and misses in every frame
    # the reference is float32: a ref_err far above its rounding would mean a term the form does not have
    assert float(g["ref_err"]) < 2e-4, float(g["ref_err"])


@pytest.mark.parametrize("name", NAMES)
def test_wrong_twin_is_rejected(measured, name):
    g, m = measured[name]
    ref_errs = {n: float(measured[n][0]["ref_err"]) for n in NAMES}
    share = A.twin_share(name, g["rgb"], m["band"], A.bar(name, ref_errs))
    assert share >= A.MIN_TWIN_SHARE, (A.CASES[name]["twin"], share)
    assert abs(share - float(g["twin_share"])) <= 1.0 / (A.RES * A.RES)
    for also in A.CASES[name].get("also", ()):
        more = A.twin_share(name, g["rgb"], m["band"], A.bar(name, ref_errs), twin=also)
        assert more >= A.MIN_TWIN_SHARE, (also, more)


MARCH = [n for n in NAMES if A.CASES[n]["family"] == "march"]


@pytest.mark.parametrize("name", MARCH)
def test_allowance_cannot_hide_a_failure(measured, name):
    """The two conditions on a march case's allowance D, on the reference's film alone: D is at most 5 % of the sample's scale on at least 90 % of
    the included samples, and every twin puts at least MIN_TWIN_SHARE of them beyond ITS allowance plus 10 x the bar.  The reference itself
    stays inside D up to float rounding (its excess is ref_err); the share of D it uses (`tightness`) is reproduced from the fixture."""
    g, m = measured[name]
    assert m["D"] is not None and (m["D"] >= 0).all() and np.isfinite(m["D"]).all()
    assert m["tight_share"] >= A.MIN_TIGHT_SHARE and abs(m["tight_share"] - float(g["tight_share"])) <= 1.0 / (A.RES * A.RES), m["tight_share"]
    # (tightness is taken where D >= 1e-3 of the scale, and the excess is at most ref_err of the scale)
    assert abs(m["tightness"] - float(g["tightness"])) <= 1e-6 and m["tightness"] <= 1.0 + float(g["ref_err"]) / 1e-3, m["tightness"]
    ref_errs = {n: float(measured[n][0]["ref_err"]) for n in NAMES}
    b = A.bar(name, ref_errs)
    assert b >= A.BAR_FACTOR * ref_errs["medium_homogeneous"] > 0
    for twin in (A.CASES[name]["twin"],) + tuple(A.CASES[name].get("also", ())):
        assert A.twin_share(name, g["rgb"], m["band"], b, twin=twin) >= A.MIN_TWIN_SHARE, twin
    # a camera ray that hits nothing has alpha 0 and carries the form's Lv: the film holds it (the sky of a "_tr" case, Le black, is black)
    sky = ~m["band"] & (g["alpha"] == 0)
    assert sky.sum() > 0.2 * A.RES * A.RES
    assert np.array_equal((g["rgb"][sky] > 0).any(-1), (m["L"][sky] > 0).any(-1))


def tau_loop(medium, o, dn, s0, s1, h, u):
    """DensityRegion::Tau (core/volume.cpp:139-157) restated: samples of Density every h from s0 + u h while s < s1, their sum times h"""
    total, s = 0.0, s0 + u * h
    while s < s1:
        total += float(medium.density(o + s * dn))
        s += h
    return total * h


@pytest.mark.parametrize("kind", ["exponential", "volumegrid"])
def test_tau_stays_within_its_bound_for_any_offset(kind):
    """Rule 1 behind every allowance, with no reference and no package: for seeded rays through the region (under a CTM) and seeded offsets u,
    Tau's loop at 17, 69 and 172 steps per ray differs from the exact integral of Density by at most h (TV + max f), and uses a good part of it;
    the exact integral (Gauss-Legendre per smooth piece) agrees with a fine midpoint sum."""
    rng = np.random.default_rng(3)
    box = dict(p0=(-2, 0, -2), p1=(2, 2.5, 2), sigma_a=.1, sigma_s=.1, v2w=A._ctm(A.VOL_CTM))
    med = (F.Medium(kind=kind, a=1.3, b=.7, updir=(.6, 2, .4), **box) if kind == "exponential" else
           F.Medium(kind=kind, nx=4, ny=3, nz=5, values=np.round(rng.random(60) * 2.0, 3), **box))
    v2w = np.linalg.inv(med.w2v)
    worst, n_rays = 0.0, 40
    for _ in range(n_rays):
        a, b = (F.xpoint(v2w, med.p0 + rng.random(3) * (med.p1 - med.p0) * [1.4, 1.4, 1.4] - .2 * (med.p1 - med.p0)) for _ in range(2))
        o, d = a - 2 * (b - a), (b - a) * rng.uniform(.3, 3)           # an unnormalised direction from outside the region
        dn, s0, s1, ok = med.clip(o, d, 0.0, np.inf)
        if not ok:
            continue
        exact, tv, fmax = med.depth(o, d, 0.0, np.inf)
        mid = s0 + (np.arange(40000) + .5) * (s1 - s0) / 40000
        assert abs(med.density(o + mid[:, None] * dn).sum() * (s1 - s0) / 40000 - exact) <= 1e-7 * max(exact, 1e-3)
        for steps in (17, 69, 172):
            h = (s1 - s0) / steps
            for u in list(rng.random(4)) + [0.0, 1 - 2.0 ** -24]:          # (the ends of genrand_real2's range too)
                err = abs(tau_loop(med, o, dn, float(s0), float(s1), float(h), float(u)) - float(exact))
                assert err <= h * (tv + fmax), (kind, steps, u, err, h * (tv + fmax))
                worst = max(worst, err / (h * (tv + fmax)))
    # (at u = 0 over a stretch where f falls, the left sum alone lies about h TV / 2 above the integral and the last cell overhangs besides: some
    # ray uses a good part of the bound, which is therefore not slack by an order of magnitude)
    assert 0.25 < worst <= 1.0, worst


def test_quadric_cases_show_the_inside_through_the_cut(measured):
    """the far root after a clipped near root is taken on a good share of every partial quadric's hits"""
    for name in NAMES:
        kind = A.CASES[name]["surfaces"][0]["shape"][0]
        if A.CASES[name]["family"] == "quadrics" and kind != "disk":
            m = measured[name][1]
            assert m["far_root_share"] >= 0.25 * m["hit_share"], (name, m["far_root_share"], m["hit_share"])


def test_cameras_agree_with_the_closed_form_of_a_pinhole():
    """the perspective form by another route: the ray through raster (x, y) of a square film is (+-tan(fov / 2) (1 - 2 x / W), ..., 1) in
    camera space; LookAt 0 0 -5  0 0 0  0 1 0 mirrors x (right = dir x up = -x)"""
    cam = F.Camera("perspective", 64, 64, F.look_at((0, 0, -5), (0, 0, 0), (0, 1, 0)), fov=60)
    o, d, mint, maxt = cam.rays(np.array([0.0, 32.0, 64.0]), np.array([32.0, 32.0, 0.0]))
    t = np.tan(np.radians(30))
    want = np.array([[t, 0, 1], [0, 0, 1], [-t, t, 1]])
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(d - want).max() < 1e-12 and np.abs(o - (np.array([0, 0, -5]) + 1e-3 * want / want[:, 2:3])).max() < 1e-9
    assert (mint == 0).all() and np.allclose(maxt * d[:, 2], 1e30)
    # a 3:2 film: the screen window is [-1.5, 1.5] x [-1, 1]
    cam = F.Camera("perspective", 96, 64, np.eye(4), fov=90)
    _, d, _, _ = cam.rays(np.array([0.0]), np.array([0.0]))
    assert np.allclose(d[0] / d[0, 2], [-1.5, 1.0, 1.0])
    cam = F.Camera("orthographic", 64, 64, np.eye(4), screen=(-2, 2, -1, 3))
    o, d, _, maxt = cam.rays(np.array([16.0]), np.array([16.0]))
    assert np.allclose(o[0], [-1, 2, 1e-3]) and np.allclose(d[0], [0, 0, 1])
    cam = F.Camera("environment", 64, 32, np.eye(4))
    _, d, _, _ = cam.rays(np.array([0.0, 16.0]), np.array([16.0, 16.0]))
    assert np.allclose(d, [[1, 0, 0], [0, 0, 1]], atol=1e-12)
    # the thin lens: the lens sample (.5, .5) is the lens centre (the pinhole's ray); from any lens point the ray passes through the pinhole
    # ray's point on the plane of focus; the square's edge midpoints and corners map onto the unit circle
    pin = F.Camera("perspective", 64, 64, np.eye(4), fov=60)
    lens = F.Camera("perspective", 64, 64, np.eye(4), fov=60, lensradius=.5, focaldistance=7)
    x, y = np.array([3.0, 40.0]), np.array([50.0, 9.0])
    po, pd, _, _ = pin.rays(x, y)
    lo, ld, _, _ = lens.rays(x, y)
    assert np.abs(lo - po).max() < 1e-15 and np.abs(ld - pd).max() < 1e-12
    lo, ld, _, _ = lens.rays(x, y, lens_u=.9, lens_v=.2)
    focus = po + ((7 - pin.hither) / pd[:, 2:3]) * pd
    assert np.abs(lo + ((7 - lo[:, 2:3]) / ld[:, 2:3]) * ld - focus).max() < 1e-12 and np.abs(lo[:, :2] - po[:, :2]).max() > .1
    dx, dy = F.concentric_sample_disk(np.array([1, .5, 0, .5, 1, 0, .5]), np.array([.5, 1, .5, 0, 1, 0, .5]))
    s = np.sqrt(.5)
    assert np.allclose(np.stack([dx, dy], 1), [[1, 0], [0, 1], [-1, 0], [0, -1], [s, s], [-s, -s], [0, 0]], atol=1e-12)


@pytest.mark.parametrize("name", list(A.PROBES))
def test_probe_fixture_agrees_with_the_float64_camera_and_intersectors(name):
    """The reference's own camera rays and closest hits (probe integrator records) of the orthographic, the environment and the thin-lens camera
    looking at one of every quadric: the stored band and deviations are reproduced; outside the band hit or miss is the form's; t, the hit point (relative
    to t), the normal (up to its sign) and (u, v) are the form's to float32 accuracy.  The bounds are float32 rounding (2^-24 = 6e-8) times
    the conditioning of a quadratic's root, an acosf / atan2f and a normalised cross product on these shapes, taken as 2^12: 2.5e-4."""
    g = load(name)
    assert str(g["scene"]) == A.scene_text(name)
    m = A.measure_probe(name, g["records"])
    assert np.array_equal(m["band"], g["band"]) and m["band_share"] <= A.BAND_CAP
    assert m["hit_equal"] and m["mint_equal"] and m["maxt_equal"]
    assert m["kinds_hit"] == sorted(["sphere", "disk", "cylinder", "cone", "paraboloid", "hyperboloid"]) and m["far_root_share"] > .2
    for k in ("dev_o", "dev_d", "dev_t", "dev_p", "dev_n", "dev_uv"):
        assert abs(m[k] - float(g[k])) <= 1e-6 * float(g[k]) + 1e-18, (k, m[k], float(g[k]))
    assert m["dev_o"] < 2e-7 and m["dev_d"] < 1e-6
    assert max(m["dev_t"], m["dev_p"], m["dev_n"], m["dev_uv"]) < 2.5e-4, m


def test_live_reference_case():
    """When oracle/_ref travelled with the tree: one case rendered now by the unmodified reference gives the fixture's film again."""
    import __graft_entry__ as g_entry
    name = "quadric_hyperboloid"
    ref = g_entry.load_ref_runner()
    if not os.path.exists(os.path.join(ref.REF_DIR, "pbrt_ref")):
        pytest.skip("oracle/_ref not on this box")
    rgb, alpha, _ = ref.run_reference(A.scene_text(name), keyed=False)
    g = load(name)
    assert np.array_equal(rgb, g["rgb"]) and np.array_equal(alpha, g["alpha"])
