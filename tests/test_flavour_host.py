"""Which kernel instantiation a frame runs (pbrt-v1_amd/csrc/hip/rt_flavour.h), on the host: tests/flavour_host_test.cpp enumerates every request and
checks the template arguments of the selected table entry against the selection rules, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer.  No GPU, no HIP header: the films of the flavours agree, so no rendering test can see a wrong choice."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_flavour_selection_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is missing or does not start here")
    exe = tmp_path / "flavour_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                          ["-I", os.path.join(ROOT, "pbrt-v1_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "flavour_host_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "flavour_host_test: ok (96 requests)" in r.stdout
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in out, out
