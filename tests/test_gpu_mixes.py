"""Seeded cross-feature scenes on the device against the unmodified reference: the fixtures of tests/golden/mixes/ (tests/golden/make_mix_golden.py:
density media, shinymetal / translucent, the infinite light and the bidirectional integrator drawn together with every older axis), the kernel
flavours, a two-shard split and both scene-creation paths against each other, the same scenes with a feature taken out as different films, and eight fresh seeds live when oracle/_ref travelled with the tree.
Bars are the project's (tests/gpu_checks.py), assigned by the generator from the drawn features:
  strict (Whitted / DirectLighting, no infinite light): every pixel's rgb and alpha within 1e-5, closest_rays / any_rays equal;
  loose  (path, bidirectional or an infinite light): >= 99.5 % of the pixels with per-pixel L2 < 1e-4 and mean L2 < 1e-4, alpha off on <= 0.5 % of
         the pixels, each ray count within max(4, 2e-4 * n);
  both: camera rays exact, no bad samples.  There is no allow-list: no fixture needed one."""
import json
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import GOLDEN, load_golden
from gpu_checks import (PIPELINE_ENVS, assert_flavours_agree, assert_prebuilt_agrees, assert_two_shards_agree, bar_metrics, check_bar, check_counts, differing_share,
                        fixture_names, need_gpu, render_both)

sys.path.insert(0, GOLDEN)

pytestmark = pytest.mark.gpu

MIXES = fixture_names("mixes")


def _features(name):
    return json.loads(str(np.load(os.path.join(GOLDEN, "mixes", name + ".npz"))["features"]))


# every third fixture, and every fixture with a medium (the march kernels of the queue pipeline)
FLAVOUR_CASES = [n for i, n in enumerate(MIXES) if i % 3 == 0 or _features(n)["medium"] != "none"]


def check_mix(pkg, name, text, ref_rgb, ref_alpha, st, bar):
    """counting twin and timed kernel of one scene text at the bar its features give, with the MIXMETRIC / MIXCOUNTS lines of a run's report"""
    _, rgb, alpha, cnt, trgb, talpha = render_both(pkg, text)
    for label, film, a in ((name, rgb, alpha), (name + " timed", trgb, talpha)):
        print("MIXMETRIC", json.dumps(dict(name=label, bar=bar, **bar_metrics(film, a, ref_rgb, ref_alpha))))      # (before the bar: a failing film leaves its line)
        check_bar(label, film, a, ref_rgb, ref_alpha, bar != "strict")
    print("MIXCOUNTS", json.dumps(dict(name=name, device=[cnt["closest_rays"], cnt["any_rays"]], reference=[st["closest_rays"], st["any_rays"]])))
    check_counts(name, cnt, st, bar != "strict")


def test_fixtures_present():
    assert 48 <= len(MIXES) <= 64 and len(FLAVOUR_CASES) >= len(MIXES) // 3, (len(MIXES), len(FLAVOUR_CASES))


@pytest.mark.parametrize("name", MIXES)
def test_mix_matches_reference_fixture(pkg, name):
    need_gpu(pkg)
    g = load_golden("mixes/" + name)
    check_mix(pkg, name, g["scene"], g["rgb"], g["alpha"], g["stats"], str(g["bar"]))


@pytest.mark.parametrize("name", [n for n in MIXES if json.loads(str(np.load(os.path.join(GOLDEN, "mixes", n + ".npz"))["shares"]))])
def test_the_feature_taken_out_is_another_film(pkg, name):
    """What made the generator accept the seed holds on the device too: with a drawn new feature taken out (the infinite light removed, the density
    replaced by the homogeneous region of the same constants, shinymetal / translucent replaced by matte, bidirectional replaced by path) the
    device's film is more than 1e-3 away from the fixture on at least 5 % of the pixels -- a device that ignored the feature would not pass."""
    need_gpu(pkg)
    import make_mix_golden as gen
    g = load_golden("mixes/" + name)
    f = json.loads(str(g["features"]))
    for axis, other in gen.ablations(g["scene"], f).items():
        if gen.has_no_light(other) and f["integrator"] in ("path", "bidirectional"):
            continue                                     # (no light left: the generator took the black film; bidirectional refuses such a scene)
        rgb, _, _, _ = pkg.render_text(other)
        share = differing_share(rgb, g["rgb"])
        print(name, "without", axis, "differs on", share)
        assert share >= 0.05, (name, axis, share)


@pytest.mark.parametrize("name", FLAVOUR_CASES)
def test_mix_kernel_flavours_agree(pkg, name, monkeypatch):
    """The counting twin, both PBRT_HIP_HIGH_OCC flavours, the queue pipeline (per ray, by vertex, and with 512 slots so that every slot is refilled
    many times), two shards summed into one film and rt_scene_create_prebuilt give the bit-identical film_accum(), the counting forms the same
    counters.  Bidirectional and DirectLighting "weighted" answer the pipeline switch in their megakernel form; "weighted" is one shard by design
    (tests/test_gpu_weighted.py holds the refusal)."""
    need_gpu(pkg)
    g = load_golden("mixes/" + name)
    f = json.loads(str(g["features"]))
    mega_only = f["integrator"] == "bidirectional" or f["strategy"] == "weighted"
    ps = pkg.ParsedScene(text=g["scene"])
    ds = pkg.DeviceScene(ps)
    ref, cnt_ref = assert_flavours_agree(ds, name, PIPELINE_ENVS, expect_pipeline=0 if mega_only else 1)
    ds.close()
    monkeypatch.setenv("PBRT_HIP_PIPELINE", "0")          # the megakernel also where a medium in a larger tree would take the queue pipeline
    b = assert_prebuilt_agrees(pkg, ps, ref, cnt_ref)
    if f["strategy"] != "weighted":
        assert_two_shards_agree(ps, b, ref, cnt_ref, exact=f["filter"] == "box")
    b.close()


@pytest.mark.parametrize("k", range(8))
def test_live_mixes_when_the_reference_is_present(pkg, k):
    """When oracle/_ref travelled with the tree: seed 10000 + k (never a committed one) drawn by mix_scene, rendered by the reference on this
    machine's CPU and by the device, at the bar its features give."""
    need_gpu(pkg)
    import make_mix_golden as gen
    text, f = gen.mix_scene(10_000 + k)
    bar = gen.bar_of(f)
    try:
        ref_rgb, ref_alpha, st = g_entry.load_ref_runner().run_reference(text, keyed=True)
    except FileNotFoundError:
        pytest.skip("oracle/_ref not on this box")
    assert st["stderr_lines"] == 0
    check_mix(pkg, "live_%d" % (10_000 + k), text, ref_rgb, ref_alpha, st, bar)
