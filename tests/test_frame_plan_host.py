"""What the host plans for a frame (pbrt-v1_amd/csrc/hip/rt_frame_plan.h), on the host: tests/frame_plan_host_test.cpp checks the work extent, the
sample-request tables, the scheduling policy with its knobs, the medium's march bounds and the launch (plan_launch: family and table entry) against the reference's rules and the policy as DESIGN.md
states it, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU, no HIP header: that the program compiles with
a host compiler is the proof that the header has none."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_frame_plan_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is missing or does not start here")
    exe = tmp_path / "frame_plan_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                          ["-I", HIP_DIR, os.path.join(ROOT, "tests", "frame_plan_host_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "frame_plan_host_test: ok (264 cases)" in r.stdout, out
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in out, out


def test_render_path_names_its_knobs_once():
    """rt_kernels.hip reads the render path's PBRT_HIP_* knobs in frame_knobs() and nowhere else, and the planner reads no environment"""
    text = open(os.path.join(HIP_DIR, "rt_kernels.hip")).read()
    start = text.index("static plan::FrameKnobs frame_knobs()")
    body = text[start:text.index("\n}\n", start)]
    names = set(re.findall(r'"(PBRT_HIP_\w+)"', body))
    assert names == {"PBRT_HIP_" + k for k in ("HIGH_OCC", "LEAF_MIN", "TRAV_MODE", "XCD_BANDS", "EXIT_THRESH", "PHASE_SYNC", "PIPELINE", "MEGA_TILE", "DEBUG_PIXEL",
                                               "FIXED_FRAME", "PIPE_VERTEX", "PIPE_MEM_MB", "PIPE_SLOTS", "DEBUG_NOFILM")}
    rest = text[:start] + text[start + len(body):]
    assert set(re.findall(r'"(PBRT_HIP_\w+)"', rest)) <= {"PBRT_HIP_TUNE"}
    plan = open(os.path.join(HIP_DIR, "rt_frame_plan.h")).read()
    assert "getenv" not in plan.split("#pragma once", 1)[1] and "hip/hip_runtime" not in plan
