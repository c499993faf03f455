"""The fixtures of tests/golden/medium/ (the reference's answers to medium queries, tests/golden/make_medium_golden.py) against the float64 forms of
tests/medium_forms.py, on the CPU: the stored ref_err is the forms' distance from the reference and nothing else, the exclusion rule stays under the
project's cap, the discrete outputs agree, every region is entered, each deliberately wrong twin of the forms is told apart; the march guard
compiled for the host; and the library's side of the two calls: the header's declarations, the exported symbols, the ctypes structure, the kernel's
resource report and the wrapper's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import analytic_cases as A
import medium_cases as MC
from conftest import GOLDEN, ROOT

CASES = list(MC.CASES)
_memo = {}


def fixture(name):
    if name not in _memo:
        z = np.load(os.path.join(GOLDEN, "medium", name + ".npz"))
        fx = {k: z[k] for k in z.files}
        _memo[name] = (fx, MC.ref_err(name, fx, fx["answers"], int(fx["seed"])))
    return _memo[name]


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_what_the_generator_makes_of_the_case(name):
    fx, _ = fixture(name)
    assert str(fx["scene"]) == MC.scene_text(name) and int(fx["seed"]) == MC.SEED
    q = MC.queries(name)
    for k, v in q.items():
        assert v.dtype == fx[k].dtype and np.array_equal(v, fx[k], equal_nan=True), (name, k)
    n = len(fx["p"])
    assert n <= 4096 and fx["answers"].shape == (n, 32) and fx["answers"].dtype == np.float32
    assert os.path.getsize(os.path.join(GOLDEN, "medium", name + ".npz")) < 320 * 1024
    rays = fx["rays"]
    length = np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=-1)
    assert (np.abs(length - 1) > .05).mean() > .8                          # unnormalised directions
    assert np.isinf(rays[:, 7]).sum() > n // 4 and (rays[:, 6] > rays[:, 7]).sum() > 10


@pytest.mark.parametrize("name", CASES)
def test_ref_err_is_the_references_distance_from_the_float64_forms(name):
    """recomputed here and equal to what the fixture stores; small enough that the forms lack no term; the left-out share is the stored one and under
    the cap; hit and the draws are the forms' on every included query; the region is entered; no march takes more than about 64 Tau samples"""
    fx, (err, left_out, w) = fixture(name)
    inc = ~w["excluded"]
    print("MEDIUM-FORM %s left out %.4f %s" % (name, left_out, {k: "%.3g" % v for k, v in err.items()}))
    assert left_out <= A.BAND_CAP and left_out == pytest.approx(float(fx["left_out"]), abs=1e-12)
    for i, k in enumerate(MC.OUTPUTS):
        assert err[k] == pytest.approx(float(fx["ref_err"][i]), rel=1e-6, abs=1e-12), (name, k)
        assert err[k] < 2e-3, (name, k, err[k])
    for k in MC.DISCRETE:
        assert np.array_equal(MC.answer(fx["answers"], k)[inc], w[k][inc]), (name, k)
    assert not MC.coverage(name, fx, w)
    assert w["tau_samples"].max() <= 64 and w["draws_lv"].max() <= 64
    # points on both sides of every face of the extent, outside the band
    ins = w["sigma_t"].any(-1) if name != "grid" else None
    if ins is not None:
        assert (ins & inc).sum() > 200 and (~ins & inc).sum() > 200


@pytest.mark.parametrize("name,twin", [(n, t) for n in CASES for t in (MC.CASES[n]["twin"],) + tuple(MC.CASES[n].get("also", ()))])
def test_a_wrong_twin_of_the_forms_exceeds_the_bar(name, twin):
    """the reference's answers against the forms with one term deliberately wrong (analytic_forms.Medium's twins): some output is beyond ten times
    the bar the device is held to, so the fixture can tell the two apart"""
    fx, (err, _, w) = fixture(name)
    inc = ~w["excluded"]
    median = np.median([fixture(c)[0]["ref_err"] for c in CASES], axis=0)
    wrong = MC.errors(fx["answers"], MC.evaluate(name, fx, int(fx["seed"]), twin=twin), inc)
    over = {k: wrong[k] / (A.BAR_FACTOR * max(err[k], float(median[i]))) for i, k in enumerate(MC.OUTPUTS)}
    print("MEDIUM-TWIN %s %s: error over bar %s" % (name, twin, {k: "%.3g" % v for k, v in over.items()}))
    assert max(over.values()) > 10, (name, twin, over)


def test_march_guard_compiled_for_the_host(tmp_path):
    """tests/medium_guard_host.cpp: rt::march_advances at t = 3e8 with step 10, at t = 0, at negative t, at inf / NaN, against the loop itself on
    seeded intervals, and rt::march_caps at the 2^20 and 65536 limits"""
    exe = tmp_path / "medium_guard_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip"),
                           os.path.join(ROOT, "tests", "medium_guard_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "medium_guard_host: ok (" in r.stdout, r.stdout + r.stderr


def test_march_guard_header_needs_no_hip():
    text = open(os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip", "rt_march_guard.h")).read()
    assert "hip/hip_runtime" not in text and re.findall(r'#\s*include\s+[<"]([^>"]+)[>"]', text) == ["math.h", "rt_ray_guard.h"]


def test_python_side_matches_the_header(pkg):
    """RtMediumQuery: the header's fields in the header's order, its size and offsets as the C compiler lays them out (seven pointers, three
    4-byte host values padded to 16, twelve pointers); both symbols exported"""
    head = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    assert "int rt_medium_device(RtScene *s, uint32_t n, const RtMediumQuery *q);" in head
    assert "int rt_volume_samples_device(RtScene *s, const RtRenderDesc *rd, uint64_t first, uint32_t count, uint32_t *dev_out);" in head
    assert "is not computed" not in head and "rt_medium_device's `tr`" in head
    body = re.search(r"typedef struct RtMediumQuery \{(.*?)\} RtMediumQuery;", head, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f for f, _ in pkg.RtMediumQuery._fields_], names
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(pkg.RtMediumQuery) == 21 * ptr
    off = {n: getattr(pkg.RtMediumQuery, n).offset for n in names}
    assert [off[n] for n in ("p", "w", "wp", "rays", "u", "u_scatter", "rng")] == [i * ptr for i in range(7)]
    assert (off["seed"], off["step_size"], off["volume_integrator"]) == (7 * ptr, 7 * ptr + 4, 7 * ptr + 8)
    assert [off[n] for n in ("sigma_a", "sigma_s", "sigma_t", "lve", "phase", "hit", "t01", "tau", "tr", "lv", "draws", "status")] == [(9 + i) * ptr for i in range(12)]
    assert pkg.MEDIUM_FIELDS == ("sigma_a", "sigma_s", "sigma_t", "lve", "phase", "hit", "t01", "tau", "tr", "lv", "draws", "status")
    lib = C.CDLL(pkg.HIP_LIB)
    assert lib.rt_medium_device is not None and lib.rt_volume_samples_device is not None
    L = pkg.hip_lib()
    assert L.rt_medium_device.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(pkg.RtMediumQuery)] and L.rt_medium_device.restype == C.c_int
    assert L.rt_volume_samples_device.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    # a null scene is refused by name without a device
    assert L.rt_medium_device(None, 1, None) == -1 and b"rt_medium_device" in L.rt_last_error() and b"null scene" in L.rt_last_error()
    assert L.rt_volume_samples_device(None, None, 0, 1, None) == -1 and b"rt_volume_samples_device" in L.rt_last_error()


def test_the_kernels_resource_report(pkg):
    """lib/obj/rt_medium.resources.txt: neither kernel takes scratch or LDS"""
    text = open(os.path.join(os.path.dirname(pkg.HIP_LIB), "obj", "rt_medium.resources.txt")).read()
    for kernel in ("medium_query_kernel", "volume_samples_kernel"):
        assert kernel in text
        block = text[text.index(kernel):]
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
        lds = re.search(r"LDS Size \[bytes/block\]: (\d+)", block)
        assert scratch and lds and int(scratch.group(1)) == 0 and int(lds.group(1)) == 0, block[:1200]


@pytest.mark.parametrize("name", CASES)
def test_parsed_scene_has_the_cases_medium(pkg, name):
    ps = pkg.ParsedScene(text=MC.product_text(MC.scene_text(name)))
    assert ps.valid and ps.errors == 0
    view = ps.render_view()
    assert view["seed"] == MC.SEED and view["volume_integrator"] == pkg.VOLUME_EMISSION and view["step_size"] == np.float32(MC.CASES[name]["stepsize"])


def test_wrapper_refuses_wrong_tensors_before_the_library(pkg):
    """DeviceScene.medium's own checks need no device: dtype, shape, contiguity, missing inputs and unknown fields raise ValueError (a scene object
    that was never opened stands in: the checks come before anything touches it)"""
    import torch
    ds = object.__new__(pkg.DeviceScene)
    p, rays, u = torch.zeros((8, 3)), torch.zeros((8, 8)), torch.zeros(8)
    for kw, word in ((dict(p=p.double(), fields=("sigma_a",)), "float32"),
                     (dict(p=p[:, :2].contiguous(), fields=("sigma_a",)), "shape"),
                     (dict(p=torch.zeros(8), fields=("sigma_a",)), "shape"),
                     (dict(rays=rays[:, :7].contiguous(), fields=("hit",)), "shape"),
                     (dict(rays=rays.t().contiguous().t(), fields=("hit",)), "contiguous"),
                     (dict(rays=rays, p=p[:4].contiguous(), fields=("sigma_a",)), "shape"),
                     (dict(rays=rays, fields=("sigma_a",)), "p: needed"),
                     (dict(p=p, fields=("phase",)), "w, wp: needed"),
                     (dict(p=p, w=p, fields=("phase",)), "w, wp: needed"),
                     (dict(p=p, fields=("hit",)), "rays: needed"),
                     (dict(rays=rays, fields=("tau",)), "u: needed"),
                     (dict(rays=rays, u=u, fields=("lv",)), "u_scatter: needed"),
                     (dict(rays=rays, u=torch.zeros((8, 1)), fields=("tau",)), "shape"),
                     (dict(rays=rays, u=u.double(), fields=("tau",)), "float32"),
                     (dict(rays=rays, rng=torch.zeros((8, 2)), fields=("tr",)), "dtype"),
                     (dict(rays=rays, fields=("nope",)), "unknown field"),
                     (dict(rays=rays, fields=()), "at least one"),
                     (dict(rays=np.zeros((8, 8), np.float32), fields=("hit",)), "torch tensor"),
                     (dict(rays=rays, fields=("hit",)), "device memory"),
                     (dict(p=p, fields=("sigma_a",)), "device memory")):
        with pytest.raises(ValueError) as e:
            ds.medium(**kw)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ValueError):
        ds.volume_samples(-1, 4)
