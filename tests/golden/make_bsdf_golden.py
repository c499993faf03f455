"""Generate tests/golden/bsdf/<case>.npz: the reference's answers to the BSDF queries of tests/bsdf_cases.py.  Runs only where the reference
sources exist.

    python tests/golden/make_bsdf_golden.py [case ...]

The reference answers through a plugin of this project's own text, tests/golden/bsdf_probe.cpp (a SurfaceIntegrator "bsdfprobe" written against the
reference's public interfaces, like oracle/ref/rayfile_integrator.cpp): compiled here with the flags of oracle/ref/Makefile into the git-ignored
oracle/_ref/bin, where the reference looks for its plugins, and run by oracle/_ref/pbrt_ref_keyed through oracle/ref_runner.py (no random number
enters: the plugin does its work in Preprocess).  Each fixture is DATA: the scene text, the query records (rays, wi, u, flags), the reference's answer
records, and ref_err -- the reference's own largest error against the float64 forms of tests/bsdf_forms.py per output, with the share of queries the
exclusion rule leaves out.  The generator refuses a case whose left-out share is above analytic_cases.BAND_CAP, a hit mask that differs from the
form's outside the band, a surface no included query hits, a ref_err that says the form lacks a term, and a fixture above 320 KB.  The compiled plugin
is never committed."""
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
import bsdf_cases as C  # noqa: E402

REFERENCE = "/root/reference"
OUT = os.path.join(HERE, "bsdf")
MAX_BYTES = 320 * 1024
SEEDS = {"gallery_flat": 11, "gallery_smooth_grid": 12, "gallery_quadrics": 13, "gallery_textured": 14, "gallery_emitters": 15}
# the compiler flags of oracle/ref/Makefile (the reference's own: -O2 -msse2 -mfpmath=sse -DNDEBUG)
FLAGS = ["-O2", "-msse2", "-mfpmath=sse", "-DNDEBUG", "-fPIC", "-w", "-I" + os.path.join(REFERENCE, "core"), "-I" + REFERENCE]


def build_plugin(ref_dir):
    out = os.path.join(ref_dir, "bin", "bsdfprobe.so")
    subprocess.check_call(["g++"] + FLAGS + ["-shared", os.path.join(HERE, "bsdf_probe.cpp"), "-o", out])
    return out


def main():
    if not os.path.isdir(REFERENCE):
        raise SystemExit("the reference sources are not here: the fixtures under tests/golden/bsdf/ stay as they are")
    REF = g.load_ref_runner()
    build_plugin(REF.REF_DIR)
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name in C.CASES:
        if only and name not in only:
            continue
        d = tempfile.mkdtemp()
        q = C.queries(name, SEEDS[name])
        C.query_records(q).tofile(os.path.join(d, "queries.bin"))
        dump = os.path.join(d, "bsdf.bin")
        text = C.scene_text(name, os.path.join(d, "queries.bin"), dump)
        REF.run_reference(text, keyed=True, workdir=d)
        ans = np.fromfile(dump, np.float32).reshape(-1, 36)
        assert len(ans) == len(q["ridx"]) <= 4096, (name, ans.shape)
        err, left_out, w = C.ref_err(name, q, ans)
        inc = ~w["excluded"]
        print(name, ans.shape, "left out %.4f" % left_out, "hit share %.3f" % w["hit"].mean(), {k: "%.3g" % v for k, v in err.items()})
        assert left_out <= A.BAND_CAP, "%s: %.4f of the queries are left out" % (name, left_out)
        sc, mats, _ = C.form(name)
        surf = sc.closest(*[q["rays"].astype(np.float64)[:, s] for s in (slice(0, 3), slice(3, 6), 6, 7)])[2][q["ridx"]]
        assert sorted(np.unique(surf[inc & w["hit"]])) == list(range(len(mats))), "%s: surfaces hit %s" % (name, np.unique(surf[inc & w["hit"]]))
        assert .03 <= 1 - w["hit"].mean() <= .45, (name, w["hit"].mean())
        assert np.array_equal(C.answer(ans, "s_type")[inc], w["s_type"][inc]) and np.array_equal(C.answer(ans, "n_components")[inc], w["n_components"][inc]), name
        assert max(err.values()) < 2e-3, "%s: the form lacks a term (%s)" % (name, err)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(C.scene_text(name)), seed=np.array(SEEDS[name]), answers=ans, left_out=np.array(left_out),
                            ref_err=np.array([err[k] for k in C.OUTPUTS]), **q)
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))
        print("  ", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
