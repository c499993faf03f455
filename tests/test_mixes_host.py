"""The seeded cross-feature fixtures of tests/golden/mixes/ (tests/golden/make_mix_golden.py) on the host: every scene parses, its `features` say
what the parsed scene holds, mix_scene(seed) still writes the committed text byte for byte, the files stay small, MANIFEST.json lists every seed
tried, and the accepted fixtures meet the coverage table.  CPU only."""
import glob
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)

MIXES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "mixes", "*.npz")))
INTEGRATOR_ID = {"whitted": 0, "directlighting": 1, "path": 2, "bidirectional": 3}
STRATEGY_ID = {"all": 0, "one": 1, "weighted": 2}


@pytest.fixture(scope="module")
def gen(pkg):
    import make_mix_golden
    return make_mix_golden


def manifest():
    with open(os.path.join(GOLDEN, "mixes", "MANIFEST.json")) as fh:
        return json.load(fh)


def features(g):
    return json.loads(str(g["features"]))


def test_manifest_lists_every_seed_tried_in_order():
    m = manifest()
    seeds = m["seeds"]
    assert [s["seed"] for s in seeds] == list(range(m["tried"])) and m["accepted"] == sum(s["accepted"] for s in seeds)
    assert sorted("mix_%03d" % s["seed"] for s in seeds if s["accepted"]) == MIXES
    assert 48 <= len(MIXES) <= 64
    for s in seeds:
        assert (s["reason"] is None) == s["accepted"], s["seed"]
        if s["accepted"]:
            assert all(v >= 0.05 for v in s["shares"].values()), s["seed"]


@pytest.mark.parametrize("name", MIXES)
def test_fixture_parses_and_its_features_are_the_scene(pkg, gen, name):
    g = load_golden("mixes/" + name)
    f = features(g)
    path = os.path.join(GOLDEN, "mixes", name + ".npz")
    assert os.path.getsize(path) < gen.MAX_BYTES, os.path.getsize(path)
    text, f2 = gen.mix_scene(f["seed"])
    assert name == "mix_%03d" % f["seed"] and text == g["scene"] and f2 == f, name
    assert str(g["bar"]) == gen.bar_of(f)
    assert np.isfinite(g["rgb"]).all() and g["rgb"].shape[:2] == g["alpha"].shape and max(g["rgb"].shape[:2]) <= 40
    assert float((g["rgb"].max(axis=-1) > 0).mean()) >= 0.30
    ps = pkg.ParsedScene(text=g["scene"])
    assert ps.valid and ps.errors == 0, name
    assert (ps.width, ps.height) == (g["rgb"].shape[1], g["rgb"].shape[0])
    assert ps.integrator == INTEGRATOR_ID[f["integrator"]]
    rv = ps.render_view()
    if f["strategy"]:
        assert rv["strategy"] == STRATEGY_ID[f["strategy"]]
    # materials: the drawn ones, the matte walls / floor and the emitter's black matte; at least two different drawn ones
    types = {m["type"] for m in ps.materials()}
    assert types == set(f["materials"]) | {"matte"}, (types, f["materials"])
    assert len(set(f["materials"])) >= 2
    # lights, in any order; the emitter is one light of two triangles
    lights = ps.lights()
    assert sorted(l["type"] for l in lights) == sorted(f["lights"]), (lights, f["lights"])
    assert all(l["n_tris"] == 2 for l in lights if l["type"] == "area")
    v = ps.volume()
    if f["medium"] == "none":
        assert v is None
    else:
        assert f["integrator"] != "bidirectional"
        kind = v["density"]["kind"] if v["density"] else "homogeneous"
        assert kind == f["medium"]
        assert rv["volume_integrator"] == {"emission": 1, "single": 2}[f["volume_integrator"]] and 15 <= rv["step_size"] <= 180
        if kind == "volumegrid":
            assert [v["density"][k] for k in ("nx", "ny", "nz")] == f["grid"] and all(2 <= n <= 12 for n in f["grid"])
    assert ps.spp == f["spp"] and (f["spp"] <= 4 or (f["sampler"] == "lowdiscrepancy" and max(ps.width, ps.height) <= 28))
    assert not any(q in g["scene"] for q in ('"sphere"', '"disk"', '"cylinder"', '"cone"', '"paraboloid"', '"hyperboloid"'))
    # never a combination rt_render refuses by design
    assert f["integrator"] != "bidirectional" or lights
    if f["strategy"] == "weighted":
        assert "infinite" not in f["lights"] and not (f["medium"] != "none" and "area" in f["lights"])


def test_coverage_table(gen):
    feats = [features(load_golden("mixes/" + n)) for n in MIXES]
    assert gen.coverage_gaps(feats) == []
    # the table, spelt out once more on the main cells so that a change of coverage_gaps() cannot empty it
    def n(pred):
        return sum(1 for f in feats if pred(f))
    dens = lambda f: f["medium"] in ("exponential", "volumegrid")
    newm = lambda f: "shinymetal" in f["materials"] or "translucent" in f["materials"]
    inf = lambda f: "infinite" in f["lights"]
    for i in INTEGRATOR_ID:
        assert n(lambda f: f["integrator"] == i and "shinymetal" in f["materials"]) >= 1, i
        assert n(lambda f: f["integrator"] == i and "translucent" in f["materials"]) >= 1, i
        assert n(lambda f: f["integrator"] == i and inf(f)) >= 1, i
    for k in ("homogeneous", "exponential", "volumegrid"):
        for i in ("whitted", "directlighting", "path"):
            assert n(lambda f: f["medium"] == k and f["integrator"] == i) >= 1, (k, i)
        for v in ("emission", "single"):
            assert n(lambda f: f["medium"] == k and f["volume_integrator"] == v) >= 1, (k, v)
    for s in ("all", "one"):
        assert n(lambda f: inf(f) and f["strategy"] == s) >= 1, s
    assert n(lambda f: inf(f) and f["medium"] != "none") >= 2
    bd = lambda f: f["integrator"] == "bidirectional"
    for l in ("area", "point", "spot", "distant", "infinite"):
        assert n(lambda f: bd(f) and l in f["lights"]) >= 1, l
    for s in ("stratified", "stratified_jitter", "lowdiscrepancy", "random"):
        assert n(lambda f: bd(f) and f["sampler"] == s) >= 1, s
    for a in ("kdtree", "grid"):
        assert n(lambda f: bd(f) and f["accelerator"] == a) >= 1, a
    assert n(lambda f: bd(f) and f["camera"] in ("orthographic", "environment")) >= 1
    assert n(lambda f: dens(f) and newm(f)) >= 3 and n(lambda f: dens(f) and inf(f)) >= 3 and n(lambda f: newm(f) and inf(f)) >= 3
    assert n(lambda f: gen.bar_of(f) == "strict") >= 20
    assert n(lambda f: bd(f) and f["medium"] != "none") == 0


def test_live_seeds_are_not_committed_ones(gen):
    """tests/test_gpu_mixes.py renders seeds 10000 .. 10007 live: they draw valid scenes and are no fixture."""
    for k in range(8):
        text, f = gen.mix_scene(10_000 + k)
        assert "mix_%03d" % f["seed"] not in MIXES and text.startswith("LookAt") and text.endswith("WorldEnd\n")
