"""Generate the per-sample analytic fixtures in tests/golden/analytic/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref, the
non-keyed build: no random number enters these frames) on the cases of tests/analytic_cases.py, the way tests/golden/make_materials_golden.py
does for the material fixtures.  Runs only where the reference sources exist.

    python tests/golden/make_analytic_golden.py [name ...]

Without names only the cases whose fixture is missing are rendered: the fixtures that exist stay byte for byte what they are.

Every scene is rendered with a box filter of width .5 and one unjittered sample per pixel, so the film IS the per-sample radiance at the
pixel centres.  For each case the float64 form (tests/analytic_forms.py) is evaluated at the same positions, the exclusion band is built
(analytic_forms.band: float64 geometry only) and <name>.npz stores the scene text, the film (rgb, alpha), the band mask, `ref_err` (the
reference's largest error e outside the band, analytic_forms.sample_error) and `band_share`.  The generator refuses a fixture whose band
exceeds 3 % of the samples, one whose spot light puts too few samples into the falloff zone, and one that is insensitive: the case's
wrong twin must put at least 5 % of the included samples beyond 10 x the case's bar (analytic_cases.bar) against the reference's film
(every twin of a case that names more than one: `also`).  It refuses too a hit share outside [5 %, 100 %), a ref_err of 2e-4 or more (the form
would lack a term), a debug frame ("geometry" cases) whose alpha is not 1 on every pixel or whose `hit` channel is not the form's hit mask
outside the band, and a fixture above 64 KB.
probe_ortho_quadrics.npz, probe_env_quadrics.npz and probe_lens_quadrics.npz hold the records of the probe integrator plugin (oracle/ref/probe_integrator.cpp: camera ray
and closest hit t, p, n, u, v per camera sample) for an orthographic camera with a screen window, an environment camera and a thin-lens perspective camera that look at one of
every quadric, the band of analytic_forms.ray_band and the reference's deviations from the float64 camera and intersectors.
The "march" cases (volume integrators, density media) draw random numbers, so they run on oracle/_ref/pbrt_ref_keyed (the same unmodified sources,
their random numbers keyed by camera sample) and are held to the form within its allowance D (analytic_forms.Scene.allowance): ref_err is the
reference's largest EXCESS e' over D and falls under the same 2e-4 refusal (a reference that leaves its own allowance means the form or the bound
is wrong); D must stay under 5 % of the sample's scale on 90 % of the included samples, every twin must lie beyond ITS allowance plus 10 x the bar, and the
largest |ref - L| / D is printed and stored (`tightness`).
Fixtures are DATA (scene text, arrays, measured numbers); no reference source text is stored."""
import json
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

OUT = os.path.join(HERE, "analytic")
MAX_BYTES = 64 * 1024          # what the other generators allow a fixture


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    wanted = lambda name: name in only if only else not os.path.exists(os.path.join(OUT, name + ".npz"))
    for name in A.PROBES:
        # the camera probes: the existing "probe" integrator plugin, the existing 20-float record per camera ray
        if not wanted(name):
            continue
        d = tempfile.mkdtemp()
        dump = os.path.join(d, "rays.bin")
        REF.run_reference(A.scene_text(name, probe_dump=dump), keyed=False, workdir=d)
        rec = np.fromfile(dump, np.float32).reshape(-1, 20)
        m = A.measure_probe(name, rec)
        print(name, rec.shape, {k: v for k, v in m.items() if k != "band"})
        assert m["band_share"] <= A.BAND_CAP and m["hit_equal"] and m["mint_equal"] and len(m["kinds_hit"]) == 6, name
        np.savez_compressed(os.path.join(OUT, name + ".npz"), scene=np.array(A.scene_text(name)), records=rec, band=m["band"],
                            **{k: np.array(m[k]) for k in ("dev_o", "dev_d", "dev_t", "dev_p", "dev_n", "dev_uv", "band_share")})
    done = {}
    for name in A.CASES:
        if not wanted(name):
            continue
        text = A.scene_text(name)
        march = A.CASES[name]["family"] == "march"
        rgb, alpha, st = REF.run_reference(text, keyed=march)
        assert np.isfinite(rgb).all() and st["stderr_lines"] == 0, name
        m = A.measure(name, rgb, alpha)
        print("%-28s ref_err %.3g  band %.4f  hits %.3f  Lcase %.3g  film max %.3g  far roots %.3f  falloff share %.3f" %
              (name, m["ref_err"], m["band_share"], m["hit_share"], m["lcase"], float(rgb.max()), m["far_root_share"], m["falloff_share"]))
        assert m["alpha_equal"], "%s: alpha differs from the form's hit mask outside the band (a debug frame: alpha is not 1 everywhere, or its hit channel differs)" % name
        assert 0.05 <= m["hit_share"] < 1.0 and m["ref_err"] < 2e-4, "%s: hit share %.3f, ref_err %.3g" % (name, m["hit_share"], m["ref_err"])
        assert m["band_share"] <= A.BAND_CAP, "%s: band %.4f" % (name, m["band_share"])
        assert m["falloff_share"] >= A.CASES[name].get("min_falloff_share", 0), name
        if march:
            print("%-28s allowance: D <= %.2f x scale on %.3f of the samples, largest |ref - L| / D %.3f" % ("", A.MAX_ALLOWANCE, m["tight_share"], m["tightness"]))
            assert m["tight_share"] >= A.MIN_TIGHT_SHARE, "%s: the allowance is within %.2f of the scale on only %.3f of the samples" % (name, A.MAX_ALLOWANCE, m["tight_share"])
        done[name] = (text, rgb, alpha, m, st)
    # the bars need every case's ref_err (the family median): the cases not regenerated now come from their fixtures
    ref_errs = {n: float(np.load(os.path.join(OUT, n + ".npz"))["ref_err"]) for n in A.CASES if n not in done and os.path.exists(os.path.join(OUT, n + ".npz"))}
    ref_errs.update({n: d[3]["ref_err"] for n, d in done.items()})
    for name, (text, rgb, alpha, m, st) in done.items():
        bar = A.bar(name, ref_errs)
        share = A.twin_share(name, rgb, m["band"], bar)
        print("%-28s bar %.3g  twin %-26s beyond 10 x bar on %.3f" % (name, bar, A.CASES[name]["twin"], share))
        assert share >= A.MIN_TWIN_SHARE, "%s: the wrong twin %s differs on only %.3f of the samples" % (name, A.CASES[name]["twin"], share)
        extra = {}
        if A.CASES[name]["family"] == "march":
            extra = dict(tight_share=np.array(m["tight_share"]), tightness=np.array(m["tightness"]))
        for also in A.CASES[name].get("also", ()):
            more = A.twin_share(name, rgb, m["band"], bar, twin=also)
            extra["twin_share_" + also] = np.array(more)
            print("%-28s              twin %-26s beyond 10 x bar on %.3f" % ("", also, more))
            assert more >= A.MIN_TWIN_SHARE, "%s: the wrong twin %s differs on only %.3f of the samples" % (name, also, more)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(text), rgb=rgb, alpha=alpha, band=m["band"], ref_err=np.array(m["ref_err"]),
                            band_share=np.array(m["band_share"]), twin_share=np.array(share), stats=np.array(json.dumps(st)), **extra)
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
