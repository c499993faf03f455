"""Exact division by a frame constant (pbrt-v1_amd/csrc/hip/rt_fastdiv.h), on the host: tests/fastdiv_host_test.cpp checks rt::fastdiv against `/`
for every divisor from 1 to 4096 and the divisors of the benchmark's frames, on the dividends around every multiple's edge at both ends of the
32-bit range and on a million seeded random ones, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU, no
HIP header: the device computes the same expression (its multiply-high is __umulhi)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_fastdiv_against_division_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is missing or does not start here")
    exe = tmp_path / "fastdiv_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                          ["-I", os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "fastdiv_host_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "fastdiv_host_test: ok (" in r.stdout, out
    n_div = int(r.stdout.split("ok (")[1].split(" divisors")[0])
    assert n_div >= 4096 + 5, out
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in out, out
