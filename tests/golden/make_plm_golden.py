"""Generate tests/golden/plm/: the films of the keyed reference whose render phase runs under the portable libm (oracle/_ref/pbrt_ref_keyed_plm,
oracle/ref/portable_libm.cpp) for every committed fixture that a GPU test holds to the loose bar or to the allow-listed fallback because a libm
call reaches its geometry.  The device library's -DRT_PORTABLE_LIBM build evaluates the same functions bit for bit (rt_libm_portable.h), so
tests/test_gpu_plm.py holds it to these films at the STRICT bar.  Runs only where the reference sources exist.

    python tests/golden/make_plm_golden.py

sources() enumerates the fixtures by the GPU tests' own rules (their predicates and lists are imported, not restated):
  the goldens of tests/golden/ that test_gpu_parity.libm_bound() names; mixes whose bar is "loose"; bidir/ (all); materials/, textures/ by their
  loose_bar(); density/ under the path integrator; infinite/, shapes/, debug/ by their LOOSE lists;
  seedmix_10, seedmix_11, seedmix_15: the seeded scenes behind the allow-listed mix:10 / mix:11 / mix:15 of test_gpu_parity (its _random_scene);
  c2_64spp: the Cornell path frame of BASELINE configs[1] (maxdepth 5, 8 x 8 jittered samples, mitchell, kd-tree) at 64 x 64;
  PHASE_WITNESS, a Whitted triangle-only golden: no libm call in its render phase, so its portable film must be its glibc film bit for bit.
Each <name>.npz holds rgb, alpha, stats (ray counts, StatsPrint table and `libm_calls`, the calls per function after the first camera sample), `source`
(the fixture it was made from, relative to tests/golden, or "" for the generated scenes) and `scene_sha256`; no scene text is stored twice:
scene_text(name, source) reads it from the source fixture or generates it again, and the tests check the hash.  A loose-bar source whose render phase made no libm call is refused (listed in MANIFEST.json): nothing
distinguishes its two films.  Fixtures are DATA; no reference source text is stored."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import __graft_entry__ as g  # noqa: E402

OUT = os.path.join(HERE, "plm")
PHASE_WITNESS = "whitted_glass_mirror"
SEEDED_MIXES = (10, 11, 15)
# the cases test_gpu_parity.FALLBACK_ALLOWED grants the one-ulp-sensitivity bar under device libm, by their names here
FALLBACK = ("sphere_path_soup", "quadrics_path", "seedmix_10", "seedmix_11", "seedmix_15")


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def c2_64spp_text(scenes):
    return scenes.cornell_scene(xres=64, yres=64, integrator="path", maxdepth=5, xsamples=8, ysamples=8, jitter=True, pixel_filter="mitchell",
                                accelerator="kdtree", keyed=True, count=True)


def scene_text(name, source):
    """the scene a plm fixture was rendered from: its source fixture's text, or the generated scene of that name"""
    if source:
        from conftest import load_golden
        return load_golden(source)["scene"]
    g.load_package()
    from pbrt_v1_amd import scenes
    if name == "c2_64spp":
        return c2_64spp_text(scenes)
    assert name.startswith("seedmix_"), name
    import re
    import test_gpu_parity
    text = test_gpu_parity._random_scene(scenes, np.random.default_rng(1000 + int(name[len("seedmix_"):])))
    # the reference's ray counts come from the counting wrapper around its accelerator; the product's parser takes the wrapper off again
    text, n = re.subn(r'Accelerator "(kdtree|grid)"', r'Accelerator "countaccel" "string inner" ["\1"]', text)
    assert n == 1, name
    return text


def sources():
    """[(name, source, scene text)]: source is the fixture's path under tests/golden without .npz, or "" for a generated scene."""
    import test_gpu_bidir, test_gpu_debug, test_gpu_infinite, test_gpu_materials, test_gpu_parity, test_gpu_shapes, test_gpu_textures
    from conftest import load_golden
    from gpu_checks import fixture_names
    pkg = g.load_package()
    from pbrt_v1_amd import scenes

    def integrator(text):
        ps = pkg.ParsedScene(text=text)
        try:
            return ps.integrator
        finally:
            ps.close()
    out = []
    for name in test_gpu_parity.FILMS:
        text = load_golden(name)["scene"]
        if test_gpu_parity.libm_bound(name, integrator(text)) or name == PHASE_WITNESS:
            out.append((name, name, text))
    for name in fixture_names("mixes"):
        d = load_golden("mixes/" + name)
        if str(d["bar"]) == "loose":
            out.append((name, "mixes/" + name, d["scene"]))
    rules = (("bidir", lambda n, t: True), ("materials", lambda n, t: test_gpu_materials.loose_bar(t, integrator(t))),
             ("textures", lambda n, t: test_gpu_textures.loose_bar(t, integrator(t))), ("density", lambda n, t: integrator(t) == 2),
             ("infinite", lambda n, t: n in test_gpu_infinite.LOOSE), ("shapes", lambda n, t: n in test_gpu_shapes.LOOSE),
             ("debug", lambda n, t: n in test_gpu_debug.LOOSE))
    for sub, loose in rules:
        for name in fixture_names(sub):
            text = load_golden(sub + "/" + name)["scene"]
            if loose(name, text):
                out.append((name, sub + "/" + name, text))
    for k in SEEDED_MIXES:
        out.append(("seedmix_%d" % k, "", scene_text("seedmix_%d" % k, "")))
    out.append(("c2_64spp", "", scene_text("c2_64spp", "")))
    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out


def main():
    from make_mix_golden import MAX_BYTES, save_npz
    REF = g.load_ref_runner()
    os.makedirs(OUT, exist_ok=True)
    for name in os.listdir(OUT):
        os.remove(os.path.join(OUT, name))
    refused, table = [], {}
    for name, source, text in sources():
        rgb, alpha, st = REF.run_reference(text, keyed=True, libm="portable")
        assert st["stderr_lines"] == 0 and np.isfinite(rgb).all(), name
        calls = sum(st["libm_calls"].values())
        if name == PHASE_WITNESS:
            assert calls == 0, (name, st["libm_calls"])
        elif calls == 0:
            refused.append(name)
            print(name, "REFUSED: no libm call in the render phase")
            continue
        st = {k: v for k, v in st.items() if not k.endswith("_s")}
        arrays = dict(rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st, sort_keys=True)), source=np.array(source), scene_sha256=np.array(sha(text)))
        path = os.path.join(OUT, name + ".npz")
        save_npz(path, **arrays)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (name, size)
        table[name] = dict(source=source, closest_rays=st["closest_rays"], any_rays=st["any_rays"], libm_calls=st["libm_calls"], bytes=size)
        print(name, size, "bytes,", calls, "render-phase libm calls")
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as fh:
        json.dump(dict(fixtures=table, refused=sorted(refused)), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(len(table), "fixtures,", len(refused), "refused")


if __name__ == "__main__":
    main()
