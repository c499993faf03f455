"""Which scenes take the scene twins of the fixed-frame kernels (pbrt-v1_amd/csrc/hip/rt_fixed_frame.h, fixed::Scene and flavour::FixedScene), on the host:
tests/fixed_scene_host_test.cpp checks scene_qualifies over every combination of the scene facts and on every frame disqualifier, the family's tables
against flavour::Fixed, and that the scene's knob (SceneFacts::scene_twins) turns a twin off in plan_schedule and never on, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer.  No GPU, no HIP header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_fixed_scene_predicate_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is missing or does not start here")
    exe = tmp_path / "fixed_scene_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                          ["-I", os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "fixed_scene_host_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "fixed_scene_host_test: ok (92 cases)" in r.stdout, out
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in out, out


def test_scene_family_is_built_and_switchable():
    hip = os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip")
    header = open(os.path.join(hip, "rt_fixed_frame.h")).read()
    for switch in ("RT_FIXED_ONE_LIGHT", "RT_FIXED_NO_SPECULAR"):             # each axis can be compiled out alone
        assert "#ifndef " + switch in header
    assert "hip/hip_runtime" not in header
    # the knob is a fact of the scene, read once where the scene's other knobs are read (scene create), not per frame
    assert '"PBRT_HIP_FIXED_SCENE"' in open(os.path.join(hip, "rt_scene.hip")).read()