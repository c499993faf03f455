"""Generate tests/golden/medium/<case>.npz: the reference's answers to the medium queries of tests/medium_cases.py.  Runs only where the reference
sources exist.

    python tests/golden/make_medium_golden.py [case ...]

The reference answers through a plugin of this project's own text, tests/golden/medium_probe.cpp (a SurfaceIntegrator "mediumprobe" written against
the reference's public interfaces, like tests/golden/light_probe.cpp): compiled here with the flags of oracle/ref/Makefile into the git-ignored
oracle/_ref/bin, where the reference looks for its plugins, and run by oracle/_ref/pbrt_ref_keyed through oracle/ref_runner.py.  The plugin does its
work in Preprocess.  For the calls that take a Sample -- the volume integrator's Transmittance and Li -- it BUILDS the one-value sample the
integrator reads (a Sample for the probe, which requests nothing, and the scene's volume integrator: requests 0 and 1 are tau and scatter), filled
from the query record; nothing is done in Li of a camera sample.  Scene::Transmittance(ray) and Li each run under the keyed stream set to the
record's key with the record's counter burnt.  Each fixture is DATA: the scene text, the query records, the reference's answer records, ref_err --
the reference's own largest error against the float64 forms of tests/medium_forms.py per output -- and the share of queries the exclusion rule
leaves out.  The generator refuses a case whose left-out share is above analytic_cases.BAND_CAP, a region no included query enters, a discrete
output (hit, draws) that differs from the form's on an included query, a ref_err that says a form lacks a term, and a fixture above 320 KB.  The
compiled plugin is never committed."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import __graft_entry__ as g  # noqa: E402
import analytic_cases as A  # noqa: E402
import medium_cases as C  # noqa: E402

REFERENCE = "/root/reference"
OUT = os.path.join(HERE, "medium")
MAX_BYTES = 320 * 1024
# the compiler flags of oracle/ref/Makefile (the reference's own: -O2 -msse2 -mfpmath=sse -DNDEBUG)
FLAGS = ["-O2", "-msse2", "-mfpmath=sse", "-DNDEBUG", "-fPIC", "-w", "-I" + os.path.join(REFERENCE, "core"), "-I" + REFERENCE]


def build_plugin(ref_dir):
    out = os.path.join(ref_dir, "bin", "mediumprobe.so")
    subprocess.check_call(["g++"] + FLAGS + ["-shared", os.path.join(HERE, "medium_probe.cpp"), "-o", out])
    return out


def main():
    if not os.path.isdir(REFERENCE):
        raise SystemExit("the reference sources are not here: the fixtures under tests/golden/medium/ stay as they are")
    REF = g.load_ref_runner()
    build_plugin(REF.REF_DIR)
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name in C.CASES:
        if only and name not in only:
            continue
        d = tempfile.mkdtemp()
        q = C.queries(name)
        C.query_records(q).tofile(os.path.join(d, "queries.bin"))
        dump = os.path.join(d, "medium.bin")
        REF.run_reference(C.scene_text(name, os.path.join(d, "queries.bin"), dump), keyed=True, workdir=d)
        ans = np.fromfile(dump, np.float32).reshape(-1, 32)
        assert len(ans) == len(q["p"]) <= 4096, (name, ans.shape)
        err, left_out, w = C.ref_err(name, q, ans)
        inc = ~w["excluded"]
        print(name, ans.shape, "left out %.4f" % left_out, {k: "%.3g" % v for k, v in err.items()},
              "Tau samples up to %d, draws up to %d, roulette marches %d" % (w["tau_samples"].max(), w["draws_lv"].max(), (w["roulette"][inc] > 0).sum()))
        assert left_out <= A.BAND_CAP, "%s: %.4f of the queries are left out" % (name, left_out)
        missing = C.coverage(name, q, w)
        assert not missing, "%s: reached by no included query: %s" % (name, missing)
        bad = {k: int((C.answer(ans, k)[inc] != w[k][inc]).sum()) for k in C.DISCRETE}
        assert not any(bad.values()), "%s: discrete outputs differ from the form's: %s" % (name, bad)
        assert max(err.values()) < 2e-3, "%s: a form lacks a term (%s)" % (name, err)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(C.scene_text(name)), seed=np.array(C.SEED), answers=ans, left_out=np.array(left_out),
                            ref_err=np.array([err[k] for k in C.OUTPUTS]), **q)
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))
        print("  ", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
