"""Frames whose geometry goes through libm, held to the STRICT bar under a shared portable libm.

The product build calls the device's libm, which differs from glibc in the last bit, so such frames are held only to the loose bar there (and five
cases to an allow-listed fallback).  Here both sides evaluate the six functions with one implementation (pbrt-v1_amd/csrc/hip/rt_libm_portable.h):
the device library built with -DRT_PORTABLE_LIBM (libpbrt_hip_plm.so) and the keyed reference whose render phase runs under the same functions
(tests/golden/plm/, tests/golden/make_plm_golden.py).  What is left of a difference is the device's own.
  1. the seven functions evaluated on the device (tests/plm_device_check.hip, built by __graft_entry__.build_plm_device_check) equal the host's
     (oracle/_build/libplm.so) bit for bit on 2^20 arguments per function and the edge list;
  2. one child process (tests/plm_render_child.py, PBRT_HIP_LIB_PATH = the variant) renders every plm/ fixture as counting twin and as timed kernel;
     each is held to check_bar / check_counts with loose=False: every pixel within 1e-5, closest_rays and any_rays equal.  With oracle/_ref present
     the child also renders four fresh mix seeds through the portable reference binary, held the same way.
A child that ends with a fault, an abort or at its time limit fails the module's fixture, and nothing else of this module starts on the device; at
most two processes (this one and one child) have the device open.
Measured on an MI355X: every film within 1e-5 (largest difference 1.9e-6), all ray counts equal.  The first run of this module found a device error
(DESIGN.md 9.2): the four fixtures with a spot light under the bidirectional integrator differed by 1-2 rays, because the device inverted WorldToLight where
the reference multiplies by its stored LightToWorld; rt_scene_set_light_transforms now carries that matrix, and these fixtures are its test.
PLM_EXPLAINED: fixtures that miss the strict bar for a NAMED property of the reference that the device departs from by design, with evidence a
reader can rerun; they are still held to the loose bar.  At most a tenth of the fixtures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import GOLDEN, ROOT
from gpu_checks import check_bar, check_counts, fixture_names, need_gpu
import plm_cases

pytestmark = pytest.mark.gpu

PLM = fixture_names("plm")
LIVE = ["live_%d" % s for s in (10000, 10001, 10002, 10003)]
# name -> (cause, evidence)
PLM_EXPLAINED = {}
FAULT_CODES = (134, 139, 124, 137, -6, -11, -9)
DEVICE_CHECK_SECONDS, RENDER_SECONDS = 120, 420


def _run(cmd, seconds, env=None):
    """a child under its own time limit; a fault, an abort or the limit is this module's failure"""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.fail("%s did not end within %d s" % (os.path.basename(cmd[-2] if len(cmd) > 2 else cmd[0]), seconds))
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode not in FAULT_CODES, (r.returncode, tail)
    assert r.returncode == 0 and "HIP error" not in tail and "illegal memory access" not in tail, (r.returncode, tail)
    return r


@pytest.fixture(scope="module")
def built(pkg):
    need_gpu(pkg)
    g_entry.build_oracle()                  # the variant, libplm.so and the device check: nothing is stale in a tree that was built before it travelled
    g_entry.build_plm_device_check()
    assert os.path.exists(g_entry.PLM_LIB) and os.path.exists(g_entry.PLM_DEVICE_CHECK)
    return pkg


@pytest.fixture(scope="module")
def device_values(built, tmp_path_factory):
    """{function: (device out, device out2, a, b)} of one run of plm_device_check"""
    d = tmp_path_factory.mktemp("plm_device")
    args = plm_cases.arguments()
    n = len(args["sinf"][0])
    with open(d / "in.bin", "wb") as f:
        np.array([n], np.int64).tofile(f)
        for fn in plm_cases.FUNCS:
            a, b = args[fn]
            assert len(a) == n and len(b) == n
            a.tofile(f); b.tofile(f)
    _run([g_entry.PLM_DEVICE_CHECK, str(d / "in.bin"), str(d / "out.bin")], DEVICE_CHECK_SECONDS)
    raw = np.fromfile(d / "out.bin", np.float32).reshape(len(plm_cases.FUNCS), 2, n)
    return {fn: (raw[i, 0], raw[i, 1]) + args[fn] for i, fn in enumerate(plm_cases.FUNCS)}


@pytest.fixture(scope="module")
def rendered(built, device_values, tmp_path_factory):
    """the child's films and counters (after the device check: had that one faulted, nothing more would start)"""
    out = tmp_path_factory.mktemp("plm_films") / "films.npz"
    env = dict(os.environ, PBRT_HIP_TUNE="1", PBRT_HIP_LIB_PATH=g_entry.PLM_LIB)
    r = _run([sys.executable, os.path.join(ROOT, "tests", "plm_render_child.py"), str(out)], RENDER_SECONDS, env)
    assert "plm_render_child: ok" in r.stdout, r.stdout[-2000:]
    z = np.load(out)
    ids = json.loads(str(z["code_ids"]))
    assert ids["variant"] != ids["product"] and ids["product"] == built.code_id(), ids
    assert json.loads(str(z["names"])) == PLM
    return z


@pytest.mark.parametrize("fn", plm_cases.FUNCS)
def test_device_equals_host_bit_for_bit(device_values, fn):
    """f64 + - *, comparisons, conversions and bit casts give the same bits on gfx950 and on the host: zero mismatches (NaN equals NaN)."""
    dev, dev2, a, b = device_values[fn]
    host, host2 = plm_cases.host_eval(fn, a, b)
    bad = (dev.view(np.uint32) != host.view(np.uint32)) & ~(np.isnan(dev) & np.isnan(host))
    bad |= (dev2.view(np.uint32) != host2.view(np.uint32)) & ~(np.isnan(dev2) & np.isnan(host2))
    print(fn, len(a), "arguments,", int(bad.sum()), "mismatches")
    i = np.flatnonzero(bad)[:8]
    assert not bad.any(), (fn, int(bad.sum()), [(float(a[k]), float(b[k]), float(dev[k]), float(host[k])) for k in i])


def _hold(name, z, ref_rgb, ref_alpha, st):
    cnt = json.loads(str(z[name + "/cnt"]))
    loose = name in PLM_EXPLAINED
    calls = st.get("libm_calls", {})
    for label, rgb, alpha in ((name, z[name + "/rgb"], z[name + "/alpha"]), (name + " timed", z[name + "/trgb"], z[name + "/talpha"])):
        d = np.abs(rgb.astype(np.float64) - ref_rgb)
        print("PLMMETRIC", json.dumps(dict(name=label, maxabs=float(d.max()), pixels_off=int((d.max(-1) > 1e-5).sum()), pixels=int(d.shape[0] * d.shape[1]),
                                           device=[cnt["closest_rays"], cnt["any_rays"]], reference=[st["closest_rays"], st["any_rays"]], libm_calls=sum(calls.values()))))
    for label, rgb, alpha in ((name, z[name + "/rgb"], z[name + "/alpha"]), (name + " timed", z[name + "/trgb"], z[name + "/talpha"])):
        check_bar(label, rgb, alpha, ref_rgb, ref_alpha, loose)
    check_counts(name, cnt, st, loose)


def test_explained_list_is_short_and_argued():
    assert len(PLM_EXPLAINED) <= len(PLM) // 10 and set(PLM_EXPLAINED) <= set(PLM)
    for name, (cause, evidence) in PLM_EXPLAINED.items():
        assert cause and evidence, name


@pytest.mark.parametrize("name", PLM)
def test_fixture_meets_the_strict_bar_under_the_shared_libm(rendered, name):
    fx = np.load(os.path.join(GOLDEN, "plm", name + ".npz"))
    _hold(name, rendered, fx["rgb"], fx["alpha"], json.loads(str(fx["stats"])))


@pytest.mark.parametrize("name", LIVE)
def test_live_mix_meets_the_strict_bar_when_the_reference_is_present(rendered, name):
    if name not in json.loads(str(rendered["live"])):
        pytest.skip("oracle/_ref not on this box")
    _hold(name, rendered, rendered[name + "/ref_rgb"], rendered[name + "/ref_alpha"], json.loads(str(rendered[name + "/stats"])))


def test_light_transforms_entry_point_refuses_bad_calls(pkg):
    """rt_scene_set_light_transforms: another light count, a matrix that is not finite and a call after the first render are refused, and say why."""
    import ctypes as C
    from conftest import load_golden
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("bidir/bidir_spot_distant_grid_ld")["scene"])
    ds = pkg.DeviceScene(ps)                                      # (has handed the matrices over once: a second call before a render replaces them)
    L = pkg.hip_lib()
    good = (C.c_float * (9 * ps.n_lights))(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * ps.n_lights))
    bad = (C.c_float * (9 * ps.n_lights))(*([float("nan")] * (9 * ps.n_lights)))
    assert L.rt_scene_set_light_transforms(ds._s, good, ps.n_lights + 1) != 0 and b"n_lights" in L.rt_last_error()
    assert L.rt_scene_set_light_transforms(ds._s, bad, ps.n_lights) != 0 and b"finite" in L.rt_last_error()
    assert L.rt_scene_set_light_transforms(ds._s, None, ps.n_lights) != 0
    assert L.rt_scene_set_light_transforms(ds._s, pkg.host_lib().pbrt_host_light_to_world(ps._h, ps.frame), ps.n_lights) == 0
    ds.render()
    assert L.rt_scene_set_light_transforms(ds._s, good, ps.n_lights) != 0 and b"rendered" in L.rt_last_error()
    ds.close()
