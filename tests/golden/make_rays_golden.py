"""Generate tests/golden/rays/<name>.npz: the reference's Intersection records for the camera rays of the two scenes of tests/rays_cases.py, the way
tests/golden/make_analytic_golden.py makes its camera probes.  Runs only where the reference sources exist.

    python tests/golden/make_rays_golden.py [name ...]

The UNMODIFIED reference (oracle/_ref/pbrt_ref, the non-keyed build: no random number enters these frames) renders each scene with the existing
SurfaceIntegrator "probe" plugin (oracle/ref/probe_integrator.cpp), which writes 20 floats per camera ray: o d mint maxt | hit t p nn u v | occluded.
Each fixture stores the scene text, the records, the band mask (rays_cases.ray_band: float64 geometry only -- the surface, the root or the triangle
changes within 3e-4 rad) and the reference's own deviations from the float64 forms outside the band (dev_t, dev_p, dev_n, dev_uv: what
DeviceScene.intersect is held to, times analytic_cases.BAR_FACTOR).  The generator refuses a band above analytic_cases.BAND_CAP, a hit mask that
differs from the form's outside the band, a scene one of whose surfaces no included ray hits, and a fixture above 64 KB.
Fixtures are DATA (scene text, arrays, measured numbers); no reference source text is stored."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import __graft_entry__ as g  # noqa: E402
import analytic_cases as A  # noqa: E402
import rays_cases as R  # noqa: E402

OUT = os.path.join(HERE, "rays")
MAX_BYTES = 64 * 1024


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name, case in R.CASES.items():
        if only and name not in only:
            continue
        d = tempfile.mkdtemp()
        dump = os.path.join(d, "rays.bin")
        REF.run_reference(R.scene_text(name, probe_dump=dump), keyed=False, workdir=d)
        rec = np.fromfile(dump, np.float32).reshape(-1, 20)
        xres, yres = case["camera"]["res"]
        assert len(rec) == (xres + 1) * (yres + 1) <= 33 * 33, (name, rec.shape)
        m = R.measure(name, rec)
        print(name, rec.shape, {k: v for k, v in m.items() if k != "band"})
        assert m["band_share"] <= A.BAND_CAP, "%s: band %.4f" % (name, m["band_share"])
        assert m["hit_equal"], "%s: the reference's hit mask differs from the form's outside the band" % name
        assert m["surfaces_hit"] == list(range(len(case["surfaces"]))), "%s: surfaces hit %s" % (name, m["surfaces_hit"])
        assert 0.05 <= m["hit_share"] < 1.0, (name, m["hit_share"])
        assert max(m["dev_t"], m["dev_p"], m["dev_n"], m["dev_uv"]) < 2e-4, "%s: the form lacks a term" % name
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(R.scene_text(name)), records=rec, band=m["band"],
                            **{k: np.array(m[k]) for k in ("dev_t", "dev_p", "dev_n", "dev_uv", "band_share")})
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
