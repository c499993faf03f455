"""Film::AddSample for radiances in device memory (rt_film_add_device / rt_sample_positions_device, DeviceScene.add_samples /
sample_positions_device), the part that needs no GPU: the declared and exported surface, the wrappers' argument checks, plan_film_add as a
stand-alone program under the sanitizers (tests/film_add_host_test.cpp), the float32 restatement the GPU tests compare with
(tests/film_add_forms.py) against the frozen CPU oracle, and the compiler's resource report of the new unit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import film_add_forms as forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
UNIT = "rt_film_add"


def declared(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_and_library_exports_both_calls(pkg):
    text = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    code = declared(text)
    assert re.search(r"\bint\s+rt_sample_positions_device\s*\(\s*RtScene\s*\*\s*s\s*,\s*const\s+RtRenderDesc\s*\*\s*rd\s*,\s*uint64_t\s+first\s*,\s*uint32_t\s+count\s*,"
                     r"\s*float\s*\*\s*dev_xy\s*\)\s*;", code)
    assert re.search(r"\bint\s+rt_film_add_device\s*\(\s*RtScene\s*\*\s*s\s*,\s*const\s+RtRenderDesc\s*\*\s*rd\s*,\s*const\s+float\s*\*\s*dev_L\s*,\s*uint64_t\s+first\s*,"
                     r"\s*uint32_t\s+n\s*\)\s*;", code)
    # in the block of the device-ray calls, behind rt_radiance_device; the header says what chunks in another order give
    block = text[text.index("Rays and hits in DEVICE memory"):text.index("int rt_scene_get_stream(")]
    assert block.index("int rt_radiance_device(") < block.index("int rt_sample_positions_device(") < block.index("int rt_film_add_device(")
    assert "another order" in block and "last bit" in block
    lib = C.CDLL(pkg.HIP_LIB)
    assert hasattr(lib, "rt_sample_positions_device") and hasattr(lib, "rt_film_add_device")
    L = pkg.hip_lib()
    assert L.rt_sample_positions_device.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    assert L.rt_film_add_device.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
    assert L.rt_sample_positions_device.restype == C.c_int and L.rt_film_add_device.restype == C.c_int


def test_a_null_scene_is_refused_by_name_without_a_device(pkg):
    L = pkg.hip_lib()
    assert L.rt_film_add_device(None, None, None, 0, 1) == -1
    assert b"rt_film_add_device" in L.rt_last_error() and b"null scene" in L.rt_last_error()
    assert L.rt_sample_positions_device(None, None, 0, 1, None) == -1
    assert b"rt_sample_positions_device" in L.rt_last_error() and b"null scene" in L.rt_last_error()


def test_add_samples_refuses_bad_tensors_before_any_library_call(pkg, monkeypatch):
    import torch
    calls = []

    class Trap:
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError("library call " + name)
    monkeypatch.setattr(pkg, "_hip", Trap())
    ds = pkg.DeviceScene.__new__(pkg.DeviceScene)       # no handle: a library call would fail, the checks come first
    ds._s = None
    good = torch.zeros((6, 4), dtype=torch.float32)
    bad = {"dtype": torch.zeros((6, 4), dtype=torch.float64), "shape [n, 3]": torch.zeros((6, 3), dtype=torch.float32),
           "one dimension": torch.zeros(24, dtype=torch.float32), "not contiguous": torch.zeros((6, 8), dtype=torch.float32)[:, ::2],
           "a CPU tensor": good, "a numpy array": np.zeros((6, 4), np.float32)}
    assert bad["not contiguous"].shape == (6, 4) and not bad["not contiguous"].is_contiguous()
    for what, t in bad.items():
        for kw in ({}, {"first": 3}):
            with pytest.raises(ValueError) as e:
                ds.add_samples(t, **kw)
            assert str(e.value).startswith("L:"), (what, str(e.value))
    with pytest.raises(ValueError):
        ds.sample_positions_device(-1, 4)
    with pytest.raises(ValueError):
        ds.sample_positions_device(0, -4)
    assert calls == []


def test_torch_is_imported_inside_the_methods_only(pkg):
    src = open(os.path.join(ROOT, "pbrt-v1_amd", "__init__.py")).read()
    for head, tail, call in (("    def sample_positions_device(self", "    def add_samples(self", "rt_sample_positions_device"),
                             ("    def add_samples(self", "    def close(self):\n        if self._s:", "rt_film_add_device")):
        body = src[src.index(head):src.index(tail, src.index(head))]
        assert "import torch" in body and "wait_stream" in body and "self.parsed.render_desc" in body and call in body, head
    assert not re.search(r"^import torch|^from torch", src, flags=re.M)


def test_plan_film_add_under_sanitizers(tmp_path):
    """tests/film_add_host_test.cpp: every refusal with its words, the film rows of a range against a brute-force loop over its sample pixels, the
    staging size, n == 0"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is missing or does not start here")
    exe = tmp_path / "film_add_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O2", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                          ["-I", os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "film_add_host_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    m = re.search(r"film_add_host_test: ok \((\d+) ranges, (\d+) refusals\)", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) >= 12, out
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in out, out


# ---- the helper against the frozen CPU oracle: unjittered frames, whose image positions have a closed form
ORACLE_CASES = {
    "box_1spp": dict(xsamples=1, ysamples=1, pixel_filter="box"),
    "box_4spp": dict(xsamples=2, ysamples=2, pixel_filter="box"),
    "mitchell_1spp": dict(xsamples=1, ysamples=1, pixel_filter="mitchell"),
    "mitchell_4spp": dict(xsamples=2, ysamples=2, pixel_filter="mitchell"),
    "gaussian_1spp_crop": dict(xsamples=1, ysamples=1, pixel_filter="gaussian", crop=(0.2, 0.8, 0.3, 0.9)),
    "gaussian_4spp_crop": dict(xsamples=2, ysamples=2, pixel_filter="gaussian", crop=(0.2, 0.8, 0.3, 0.9)),
}


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_helper_weight_plane_equals_the_oracles(pkg, scenes, oracle, name):
    """accum[4] (the sum of filter weights) depends on the image positions and the filter alone: from the closed-form positions of an
    unjittered frame the helper's plane equals the oracle's bit for bit -- footprint, table index and order of accumulation"""
    text = scenes.cornell_scene(xres=24, yres=24, integrator="whitted", jitter=False, **ORACLE_CASES[name])
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    nodes, refs, bounds, info = ps.kdtree()
    want = oracle.render(ps, nodes, refs, bounds, info=info)[2]
    rd = ps.render_struct()
    xy = forms.unjittered_positions(rd)
    assert len(xy) == ps.n_camera_samples
    rec = np.concatenate([np.ones((len(xy), 4), np.float32), xy], 1)
    got, n_bad = forms.add_samples(rec, forms.film_geometry(rd))
    assert n_bad == 0 and got.shape == want.shape and want[4].max() > 0
    assert np.array_equal(got[4].view(np.uint32), want[4].view(np.uint32)), float(np.abs(got[4] - want[4]).max())
    # L = 1, alpha = 1: every plane is the weight plane
    for c in range(4):
        assert np.array_equal(got[c], got[4])


def test_helper_radiance_check():
    nan, inf = np.float32("nan"), np.float32("inf")
    rgb = np.array([[1, 2, 3], [nan, 0, 0], [0, 0, nan], [inf, inf, inf], [-inf, 0, 0], [-1, -1, -1], [-1e-6, 0, 0], [0, -2e-5, 0], [inf, -inf, 0], [0, 0, 0]], np.float32)
    out, bad = forms.checked_radiance(rgb)
    # (+inf, -inf, 0): no component is NaN and the luminance, a NaN, is neither below -1e-5 nor infinite -- the reference lets it through
    assert bad.tolist() == [False, True, True, True, True, True, False, True, False, False]
    assert (out[bad] == 0).all() and np.array_equal(out[~bad], rgb[~bad])


def parse_report(path):
    out = {}
    for block in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        num = lambda pat: int(re.search(pat, block).group(1))
        out[block.split()[0]] = dict(vgprs=num(r" VGPRs: (\d+)"), spill=num(r"VGPRs Spill: (\d+)"), scratch=num(r"ScratchSize \[bytes/lane\]: (\d+)"),
                                     occupancy=num(r"Occupancy \[waves/SIMD\]: (\d+)"), lds=num(r"LDS Size \[bytes/block\]: (\d+)"))
    return out


def test_new_units_report_exists_and_shows_no_scratch(pkg):
    pkg.build()
    assert UNIT + ".hip" in pkg.HIP_UNITS
    rep, obj = os.path.join(pkg.LIB_DIR, "obj", UNIT + ".resources.txt"), os.path.join(pkg.LIB_DIR, "obj", UNIT + ".o")
    assert os.path.exists(rep) and os.path.exists(obj) and os.path.getmtime(rep) >= os.path.getmtime(obj) - 1.0, "stale resource report for " + UNIT
    kernels = parse_report(rep)
    # both forms of the gather and the positions kernel
    assert len(kernels) == 3 and sum("film_add_kernel" in k for k in kernels) == 2 and sum("sample_positions_kernel" in k for k in kernels) == 1, list(kernels)
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["lds"] <= 64 * 1024, (name, r)
