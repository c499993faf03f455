"""The portable libm (pbrt-v1_amd/csrc/hip/rt_libm_portable.h) and the fixtures made with it (tests/golden/plm/), without a GPU.
  1. accuracy: each function against numpy float64 over its domain, at most 1 float ulp apart (a double evaluation rounded once: 0.5 + 2^-20);
     the edge conventions one by one; the same as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer;
  2. the phase rule and the chain: the portable-libm oracle (libpbrt_oracle_plm.so, every libm call portable) equals the plm/ film of every golden it
     covers within 1e-6 with equal ray counts -- test_oracle_golden's bar, which proves "glibc before the first camera sample, portable after";
     each plm/ film meets the loose bar against its glibc film, reference against reference (the five allow-listed cases the bar check_film gives them):
     the portable functions are an ordinary other libm; the Whitted triangle-only witness is its glibc film bit for bit, with no call counted;
  3. the fixtures are the ones make_plm_golden.sources() enumerates, made from the scene texts that are committed."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, film_metrics, load_golden
from gpu_checks import check_bar, check_counts, fixture_names
import plm_cases

sys.path.insert(0, GOLDEN)
import make_plm_golden as gen  # noqa: E402

PLM = fixture_names("plm")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ONE_ARG = [f for f in plm_cases.FUNCS if f not in plm_cases.TWO_ARGS and f != "sincosf"]


@pytest.fixture(scope="module")
def arguments(oracle):                      # (the oracle fixture has built oracle/_build/libplm.so)
    return plm_cases.arguments()


def ulps(got, want64):
    """|got - want| in float ulps of want, where want is a finite non-zero float; elsewhere got must be the rounded value itself (inf, 0, NaN)"""
    with np.errstate(all="ignore"):
        w32 = want64.astype(np.float32)
    plain = np.isfinite(w32) & (w32 != 0)
    ulp = np.maximum(np.spacing(np.abs(w32[plain])).astype(np.float64), 2.0 ** -149)
    err = np.abs(got[plain].astype(np.float64) - want64[plain]) / ulp
    rest_ok = (got[~plain] == w32[~plain]) | (np.isnan(got[~plain]) & np.isnan(w32[~plain])) | (np.abs(got[~plain].astype(np.float64) - want64[~plain]) <= 2.0 ** -149)
    return err, rest_ok


def glibc_share(fn, a, b, ours, n=1 << 15):
    """the share of the first n arguments on which glibc's function gives another float (reported, not asserted)"""
    m = C.CDLL("libm.so.6")
    f = getattr(m, fn)
    f.restype = C.c_float
    f.argtypes = [C.c_float] * (2 if fn in plm_cases.TWO_ARGS else 1)
    g = np.array([f(float(x), float(y)) if fn in plm_cases.TWO_ARGS else f(float(x)) for x, y in zip(a[:n], b[:n])], np.float32)
    return float(((g != ours[:n]) & ~(np.isnan(g) & np.isnan(ours[:n]))).mean())


@pytest.mark.parametrize("fn", [f for f in plm_cases.FUNCS if f != "sincosf"])
def test_accuracy_against_float64(arguments, fn):
    a, b = arguments[fn]
    a, b = a[:plm_cases.N_RANDOM], b[:plm_cases.N_RANDOM]          # the seeded arguments; the edges have their own test
    out, _ = plm_cases.host_eval(fn, a, b)
    err, rest_ok = ulps(out, plm_cases.float64_reference(fn, a, b))
    print("PLMACCURACY", fn, "max ulp %.6f over %d arguments, glibc differs on %.4f" % (err.max(), len(a), glibc_share(fn, a, b, out)))
    assert err.max() <= 1.0 and rest_ok.all(), (fn, float(err.max()), int((~rest_ok).sum()))


def test_sincosf_is_sinf_and_cosf(arguments):
    a, b = arguments["sincosf"]
    s, c = plm_cases.host_eval("sincosf", a, b)
    for got, fn in ((s, "sinf"), (c, "cosf")):
        want = plm_cases.host_eval(fn, a, b)[0]
        assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)]) and np.isnan(got[np.isnan(want)]).all(), fn


def test_edge_conventions(oracle):
    L = plm_cases.host_lib()
    f1 = {n: getattr(L, "plm_c_" + n) for n in ("sinf", "cosf", "acosf", "expf")}
    f2 = {n: getattr(L, "plm_c_" + n) for n in ("atan2f", "powf")}
    for f in f1.values():
        f.restype, f.argtypes = C.c_float, [C.c_float]
    for f in f2.values():
        f.restype, f.argtypes = C.c_float, [C.c_float, C.c_float]
    inf, nan, pi = float("inf"), float("nan"), float(np.float32(np.pi))
    bits = lambda x: np.float32(x).view(np.uint32)

    def same(got, want, what):
        assert (np.isnan(got) and np.isnan(want)) or bits(got) == bits(want), (what, got, want)
    for (fn, x), want in [(("sinf", 0.0), 0.0), (("sinf", -0.0), -0.0), (("cosf", 0.0), 1.0), (("sinf", inf), nan), (("cosf", -inf), nan), (("sinf", nan), nan), (("sinf", 3.0e38), 0.0),
                          (("cosf", 3.0e38), 1.0), (("acosf", 1.0), 0.0), (("acosf", -1.0), pi), (("acosf", 1.0000001), nan), (("acosf", -1.5), nan), (("acosf", nan), nan),
                          (("expf", 0.0), 1.0), (("expf", 89.0), inf), (("expf", inf), inf), (("expf", -104.0), 0.0), (("expf", -inf), 0.0), (("expf", nan), nan)]:
        same(f1[fn](x), want, (fn, x))
    # atan2f(y, x): signed zeros and every quadrant -- the quadrics add 2 pi when phi < 0, so atan2f(-0, x < 0) = -pi matters
    for (y, x), want in [((0.0, 0.0), 0.0), ((-0.0, 0.0), -0.0), ((0.0, -0.0), pi), ((-0.0, -0.0), -pi), ((0.0, 1.0), 0.0), ((-0.0, 1.0), -0.0), ((0.0, -1.0), pi), ((-0.0, -1.0), -pi),
                         ((1.0, 0.0), pi / 2), ((-1.0, -0.0), -pi / 2), ((1.0, 1.0), pi / 4), ((1.0, -1.0), 3 * np.pi / 4), ((-1.0, -1.0), -3 * np.pi / 4), ((-1.0, 1.0), -pi / 4),
                         ((1.0, inf), 0.0), ((1.0, -inf), pi), ((inf, 1.0), pi / 2), ((inf, inf), pi / 4), ((-inf, -inf), -3 * np.pi / 4), ((nan, 1.0), nan), ((1.0, nan), nan)]:
        same(f2["atan2f"](y, x), float(np.float32(want)), ("atan2f", y, x))
    for (x, y), want in [((0.0, 2.0), 0.0), ((0.0, 0.5), 0.0), ((-0.0, 3.0), -0.0), ((0.0, -1.0), inf), ((5.0, 0.0), 1.0), ((nan, 0.0), 1.0), ((0.0, 0.0), 1.0), ((1.0, nan), 1.0),
                         ((-2.0, 0.5), nan), ((-2.0, 1.5), nan), ((-2.0, 3.0), -8.0), ((-2.0, 2.0), 4.0), ((2.0, 10.0), 1024.0), ((4.0, 1.5), 8.0), ((2.0, 128.0), inf), ((2.0, -151.0), 0.0),
                         ((0.5, inf), 0.0), ((2.0, inf), inf), ((inf, -2.0), 0.0), ((-inf, 3.0), -inf), ((nan, 1.0), nan), ((2.0, nan), nan)]:
        same(f2["powf"](x, y), want, ("powf", x, y))


def test_stand_alone_program_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is missing or does not start here")
    exe = tmp_path / "plm_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O2", "-msse2", "-mfpmath=sse", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                          ["-I", os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "plm_host_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0 and "plm_host_test: ok (" in r.stdout, out
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in out, out


# ---------------------------------------------------------------- the fixtures
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, "plm", name + ".npz"))
    return z["rgb"], z["alpha"], json.loads(str(z["stats"])), str(z["source"]), str(z["scene_sha256"])


def test_fixtures_are_the_enumerated_sources():
    manifest = json.load(open(os.path.join(GOLDEN, "plm", "MANIFEST.json")))
    src = {n: (s, t) for n, s, t in gen.sources()}
    assert set(PLM) | set(manifest["refused"]) == set(src) and not set(PLM) & set(manifest["refused"])
    assert {"c2_64spp", gen.PHASE_WITNESS} | set(gen.FALLBACK) <= set(PLM) and len(PLM) >= 100
    for name in PLM:
        _, _, st, source, digest = _fixture(name)
        assert source == src[name][0] and digest == gen.sha(src[name][1]) == gen.sha(gen.scene_text(name, source)), name
        assert os.path.getsize(os.path.join(GOLDEN, "plm", name + ".npz")) < 64 * 1024
        assert (sum(st["libm_calls"].values()) == 0) == (name == gen.PHASE_WITNESS), (name, st["libm_calls"])


def test_phase_witness_is_its_glibc_film_bit_for_bit():
    rgb, alpha, st, source, _ = _fixture(gen.PHASE_WITNESS)
    g = load_golden(source)
    assert np.array_equal(rgb, g["rgb"]) and np.array_equal(alpha, g["alpha"])
    assert st["closest_rays"] == g["stats"]["closest_rays"] and st["any_rays"] == g["stats"]["any_rays"] and not any(st["libm_calls"].values())


def _oracle_film(pkg, oracle, text, portable):
    import contextlib
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    nodes, refs, bounds, info = ps.kdtree()
    with (oracle.portable_libm() if portable else contextlib.nullcontext()):
        rgb, alpha, _, cnt = oracle.render(ps, nodes, refs, bounds, info=info)
    return ps, (nodes, refs, bounds, info), rgb, alpha, cnt


def _source(name):
    return str(np.load(os.path.join(GOLDEN, "plm", name + ".npz"))["source"])


# the committed goldens that pin the oracle on the reference's glibc films within 1e-6: tests/golden/*.npz (tests/test_oracle_golden.py) and shapes/
# (tests/test_shapes_host.py).  The generated scenes (seedmix_*, c2_64spp) have no such glibc pin, so they are not asked for one here.
ORACLE_COVERS = [n for n in PLM if _source(n) and ("/" not in _source(n) or _source(n).startswith("shapes/"))]


@pytest.mark.parametrize("name", ORACLE_COVERS)
def test_portable_oracle_equals_the_portable_reference(pkg, oracle, name):
    """glibc before the first camera sample, portable after: the oracle starts from descriptors (set-up done by the host front end under glibc)
    and makes every libm call portable; the reference binary switches at the first sample.  The two films agree within 1e-6, ray for ray."""
    rgb, alpha, st, source, _ = _fixture(name)
    _, _, orgb, oalpha, cnt = _oracle_film(pkg, oracle, gen.scene_text(name, source), True)
    m = film_metrics(orgb, rgb)
    assert m["maxabs"] <= 1e-6 and np.abs(oalpha - alpha).max() <= 1e-6, (name, m)
    assert cnt["closest_rays"] == st["closest_rays"] and cnt["any_rays"] == st["any_rays"] and cnt["bad_samples"] == 0, (name, cnt, st)


@pytest.mark.parametrize("name", [n for n in PLM if n != gen.PHASE_WITNESS])
def test_portable_film_is_an_ordinary_other_libm_film(pkg, oracle, name):
    """reference against reference: the portable film against the glibc film of the same scene (the committed source fixture, or for the generated
    scenes the glibc oracle's film, which is the reference's: tests/test_oracle_golden.py) at the loose bar; the five allow-listed cases at the bar
    tests/test_gpu_parity.py gives them under device libm (no worse than the reference algorithm's own one-ulp sensitivity)."""
    import test_gpu_parity as parity
    rgb, alpha, st, source, _ = _fixture(name)
    text = gen.scene_text(name, source)
    if source:
        g = load_golden(source)
        ref_rgb, ref_alpha, ref_st = g["rgb"], g["alpha"], g["stats"]
    else:
        _, _, ref_rgb, ref_alpha, cnt = _oracle_film(pkg, oracle, text, False)
        ref_st = dict(closest_rays=cnt["closest_rays"], any_rays=cnt["any_rays"], stats={"Camera Rays Traced": st["stats"]["Camera Rays Traced"]})
    if name not in gen.FALLBACK:
        check_bar(name, rgb, alpha, ref_rgb, ref_alpha, True)
        check_counts(name, dict(closest_rays=st["closest_rays"], any_rays=st["any_rays"], camera_rays=parity_cam(st), bad_samples=0), ref_st, True)
        return
    m = film_metrics(rgb, ref_rgb)
    print(name, "fallback case under the portable libm", m)
    if not (m["frac"] >= 0.995 and m["mean_l2"] < 1e-4):
        ps, accel, _, _, _ = _oracle_film(pkg, oracle, text, False)
        s = parity.oracle_one_ulp_sensitivity(pkg, oracle, ps, accel)
        assert s["frac"] < 0.995, (name, m, s)
        assert m["frac"] >= s["frac"] - 0.02 and m["mean_l2"] <= 2 * s["mean_l2"] + 1e-5, (name, m, s)


def parity_cam(st):
    from conftest import stat_int
    return stat_int(st["stats"]["Camera Rays Traced"])[0]


# ---------------------------------------------------------------- the spot lights' LightToWorld (rt_scene_set_light_transforms)
def test_host_hands_out_the_spot_lights_light_to_world(pkg):
    """pbrt_host_light_to_world: NULL without a spot light; else 9 floats per light, zeros for the other lights, and for a spot light the matrix
    whose product with RtLight::world_to_light is the identity to float precision (it is CreateLight's product, not that inverse)."""
    H = pkg.host_lib()
    ps = pkg.ParsedScene(text=load_golden("whitted_point")["scene"])
    assert not H.pbrt_host_light_to_world(ps._h, ps.frame)
    ps.close()
    ps = pkg.ParsedScene(text=load_golden("bidir/bidir_spot_distant_grid_ld")["scene"])
    ptr = H.pbrt_host_light_to_world(ps._h, ps.frame)
    assert ptr
    m = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(ps.n_lights, 3, 3)).copy()
    tab = H.pbrt_host_lights(ps.scene_desc)
    kinds = [pkg.RT_LIGHT_NAMES[tab[i].type] for i in range(ps.n_lights)]
    assert "spot" in kinds
    for i, kind in enumerate(kinds):
        if kind != "spot":
            assert not m[i].any(), (i, kind)
            continue
        w2l = np.array(list(tab[i].world_to_light), np.float64).reshape(3, 3)
        assert np.abs(w2l @ m[i].astype(np.float64) - np.eye(3)).max() < 1e-5, (i, m[i])
    ps.close()
