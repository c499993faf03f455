"""Radiance along caller-supplied rays in device memory (rt_radiance_device / DeviceScene.radiance), the part that needs no GPU: the declared and
exported surface, the wrapper's argument checks, the fixtures of tests/golden/radiance/, the compiler's resource reports of the three new
units and the kernel family / query plan as a stand-alone program under the sanitizers (tests/radiance_flavour_host_test.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
UNITS = {"rt_mega_rw": ("rt_mega_w", 0), "rt_mega_rd": ("rt_mega_d", 1), "rt_mega_rp": ("rt_mega_p", 2)}       # new unit -> (the Mega unit of its integrator, the integrator)
PAIR_NAMES = ("pair_path_moved_perspective", "pair_direct_medium_ortho")


def declared(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_and_library_exports_rt_radiance_device(pkg):
    text = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    assert re.search(r"\bint\s+rt_radiance_device\s*\(\s*RtScene\s*\*\s*s\s*,\s*const\s+RtRenderDesc\s*\*\s*rd\s*,\s*const\s+RtRay\s*\*\s*dev_rays\s*,\s*uint64_t\s+first\s*,"
                     r"\s*uint32_t\s+n\s*,\s*float\s*\*\s*dev_out\s*\)\s*;", declared(text))
    # in the block of the device-ray calls, behind rt_camera_rays_device
    block = text[text.index("Rays and hits in DEVICE memory"):text.index("int rt_scene_get_stream(")]
    assert block.index("int rt_camera_rays_device(") < block.index("int rt_radiance_device(")
    lib = C.CDLL(pkg.HIP_LIB)
    assert hasattr(lib, "rt_radiance_device")
    assert pkg.hip_lib().rt_radiance_device.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]


def test_refusals_need_no_device(pkg):
    """a null scene or description is named before anything touches a device"""
    L = pkg.hip_lib()
    assert L.rt_radiance_device(None, None, None, 0, 1, None) == -1 and b"null scene" in L.rt_last_error()


def bare_scene(pkg):
    ds = pkg.DeviceScene.__new__(pkg.DeviceScene)       # no handle: a library call would fail, the checks come first
    ds._s = None
    return ds


def test_radiance_refuses_bad_tensors_before_any_library_call(pkg, monkeypatch):
    import torch
    calls = []

    class Trap:
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError("library call " + name)
    monkeypatch.setattr(pkg, "_hip", Trap())
    ds = bare_scene(pkg)
    good = torch.zeros((6, 8), dtype=torch.float32)
    bad = {"dtype": torch.zeros((6, 8), dtype=torch.float64), "shape [n, 7]": torch.zeros((6, 7), dtype=torch.float32),
           "one dimension": torch.zeros(48, dtype=torch.float32), "not contiguous": torch.zeros((6, 16), dtype=torch.float32)[:, ::2],
           "a CPU tensor": good, "a numpy array": np.zeros((6, 8), np.float32)}
    assert bad["not contiguous"].shape == (6, 8) and not bad["not contiguous"].is_contiguous()
    for what, t in bad.items():
        with pytest.raises(ValueError):
            ds.radiance(t)
        with pytest.raises(ValueError):
            ds.radiance(t, first=3)
    assert calls == []


def test_torch_is_imported_inside_the_method_only(pkg):
    src = open(os.path.join(ROOT, "pbrt-v1_amd", "__init__.py")).read()
    body = src[src.index("    def radiance(self, rays, first"):src.index("    def camera_rays_device(")]
    assert "import torch" in body and "_check_ray_tensor" in body and "wait_stream" in body and "self.parsed.render_desc" in body
    assert not re.search(r"^import torch|^from torch", src, flags=re.M)


@pytest.mark.parametrize("name", PAIR_NAMES)
def test_pair_fixtures_load_and_differ_only_in_the_camera(pkg, name):
    import make_radiance_golden as M
    path = os.path.join(GOLDEN, "radiance", name + ".npz")
    assert os.path.exists(path) and os.path.getsize(path) < 64 * 1024
    z = np.load(path)
    a, b = str(z["scene_a"]), str(z["scene_b"])
    assert (a, b) == M.scene_texts(name)
    la, lb = a.splitlines(), b.splitlines()
    assert len(la) == len(lb)
    differing = [(x, y) for x, y in zip(la, lb) if x != y]
    assert 1 <= len(differing) <= 2
    for x, y in differing:
        assert re.match(r"\s*(LookAt|Camera)\b", x) and re.match(r"\s*(LookAt|Camera)\b", y), (x, y)
    assert M.camera_statements(a) != M.camera_statements(b)
    for k in ("rgb_a", "rgb_b"):
        assert z[k].shape == (32, 32, 3) and z[k].dtype == np.float32 and np.isfinite(z[k]).all() and z[k].max() > 0
    assert z["alpha_b"].shape == (32, 32)
    share = float((np.sqrt(((z["rgb_a"] - z["rgb_b"]) ** 2).sum(-1)) > 1e-3).mean())
    assert share == float(z["share"]) >= M.MIN_SHARE
    # both parse, to the same world and the same sample set
    pa, pb = pkg.ParsedScene(text=a), pkg.ParsedScene(text=b)
    assert pa.valid and pb.valid and pa.errors == 0 and pb.errors == 0
    assert pa.n_tris == pb.n_tris and pa.n_lights == pb.n_lights and pa.n_materials == pb.n_materials and pa.n_camera_samples == pb.n_camera_samples
    assert pa.integrator == pb.integrator
    ra, rb = pa.render_struct(), pb.render_struct()
    for f, _ in pkg.RtRenderDesc._fields_:
        if f != "filter_table":
            assert getattr(ra, f) == getattr(rb, f), f


def test_the_pairs_are_what_the_issue_asks_for():
    import make_radiance_golden as M
    a, b = M.scene_texts("pair_path_moved_perspective")
    assert 'SurfaceIntegrator "path"' in a and 'Camera "perspective"' in a and 'Camera "perspective"' in b and "Volume" not in a
    a, b = M.scene_texts("pair_direct_medium_ortho")
    assert 'SurfaceIntegrator "directlighting"' in a and 'Volume "homogeneous"' in a and 'Camera "perspective"' in a and 'Camera "orthographic"' in b


def parse_report(path):
    out = {}
    for block in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        num = lambda pat: int(re.search(pat, block).group(1))
        out[block.split()[0]] = dict(vgprs=num(r" VGPRs: (\d+)"), spill=num(r"VGPRs Spill: (\d+)"), scratch=num(r"ScratchSize \[bytes/lane\]: (\d+)"),
                                     occupancy=num(r"Occupancy \[waves/SIMD\]: (\d+)"), lds=num(r"LDS Size \[bytes/block\]: (\d+)"))
    return out


def template_args(symbol):
    """(COUNT, INTEG, ACCEL, VOL, MINW, EXT) of a mangled rt::render_kernel / rt::render_kernel_fixed instantiation"""
    m = re.search(r"ILb([01])ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELb([01])E", symbol)
    assert m, symbol
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("unit", list(UNITS))
def test_new_units_reports_exist_and_show_no_scratch_beyond_the_mega_ext_entries(pkg, unit):
    """eight kernels per unit over fixed::Rays, all with the EXT code; each uses no more scratch, spills no more and reaches no lower occupancy
    than the rt::render_kernel entry with the same (counting, accelerator, medium) and EXT at natural allocation"""
    pkg.build()
    mega_unit, integ = UNITS[unit]
    assert unit + ".hip" in pkg.HIP_UNITS
    rep, obj = os.path.join(pkg.LIB_DIR, "obj", unit + ".resources.txt"), os.path.join(pkg.LIB_DIR, "obj", unit + ".o")
    assert os.path.exists(rep) and os.path.exists(obj) and os.path.getmtime(rep) >= os.path.getmtime(obj) - 1.0, "stale resource report for " + unit
    rays = parse_report(rep)
    assert len(rays) == 8 and all("render_kernel_fixed" in k and "fixed4Rays" in k for k in rays), list(rays)
    mega = {template_args(k): v for k, v in parse_report(os.path.join(pkg.LIB_DIR, "obj", mega_unit + ".resources.txt")).items()}
    seen = set()
    for sym, r in rays.items():
        count, i, accel, vol, minw, ext = template_args(sym)
        assert i == integ and ext == 1 and minw < 4, sym
        seen.add((count, accel, vol))
        twins = [v for a, v in mega.items() if a[0] == count and a[2] == accel and a[3] == vol and a[5] == 1 and a[4] < 4]
        assert len(twins) == 1, (sym, len(twins))
        m = twins[0]
        assert r["scratch"] <= m["scratch"] and r["spill"] <= m["spill"] and r["occupancy"] >= m["occupancy"] and r["lds"] <= m["lds"], (sym, r, m)
    assert len(seen) == 8


def test_radiance_flavours_and_plan_under_sanitizers(tmp_path):
    """tests/radiance_flavour_host_test.cpp: flavour::Rays round-trips, fixed::Any::caller_rays is false, the planned work extent of a query of n
    rays is n, and each refusal names its reason"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is missing or does not start here")
    exe = tmp_path / "radiance_flavour_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O2", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                          ["-I", os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "radiance_flavour_host_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "radiance_flavour_host_test: ok (96 requests)" in r.stdout, out
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in out, out
