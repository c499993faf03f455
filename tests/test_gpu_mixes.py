"""Seeded cross-feature scenes on the device against the unmodified reference: the fixtures of tests/golden/mixes/ (tests/golden/make_mix_golden.py:
density media, shinymetal / translucent, the infinite light and the bidirectional integrator drawn together with every older axis), the kernel
flavours, a two-shard split and both scene-creation paths against each other, the same scenes with a feature taken out as different films, and eight fresh seeds live when oracle/_ref travelled with the tree.
Bars are the project's (tests/test_gpu_materials.py, tests/test_gpu_infinite.py), assigned by the generator from the drawn features:
  strict (Whitted / DirectLighting, no infinite light): every pixel's rgb and alpha within 1e-5, closest_rays / any_rays equal;
  loose  (path, bidirectional or an infinite light): >= 99.5 % of the pixels with per-pixel L2 < 1e-4 and mean L2 < 1e-4, alpha off on <= 0.5 % of
         the pixels, ray counts within max(4, 2e-4 * n);
  both: camera rays exact, no bad samples.  There is no allow-list: no fixture needed one."""
import glob
import json
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as g_entry
from conftest import GOLDEN, film_metrics, load_golden, stat_int

sys.path.insert(0, GOLDEN)

pytestmark = pytest.mark.gpu

MIXES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "mixes", "*.npz")))
COUNTER_KEYS = ("camera_rays", "closest_rays", "any_rays", "nodes_visited", "leaf_refs", "tri_tests", "bad_samples")


def _features(name):
    return json.loads(str(np.load(os.path.join(GOLDEN, "mixes", name + ".npz"))["features"]))


# every third fixture, and every fixture with a medium (the march kernels of the queue pipeline)
FLAVOUR_CASES = [n for i, n in enumerate(MIXES) if i % 3 == 0 or _features(n)["medium"] != "none"]


def need_gpu(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")


def check_bar(name, rgb, alpha, ref_rgb, ref_alpha, bar):
    m = film_metrics(rgb, ref_rgb)
    m.update(alpha_maxabs=float(np.abs(alpha - ref_alpha).max()), alpha_off=float((np.abs(alpha - ref_alpha) > 1e-5).mean()))
    print("MIXMETRIC", json.dumps(dict(name=name, bar=bar, **m)))
    assert np.isfinite(rgb).all() and np.isfinite(alpha).all(), name
    if bar == "strict":
        assert m["maxabs"] <= 1e-5 and m["alpha_maxabs"] <= 1e-5, (name, m)
    else:
        assert m["frac"] >= 0.995 and m["mean_l2"] < 1e-4, (name, m)
        assert m["alpha_off"] <= 0.005, (name, m)
    return m


def check_counts(name, cnt, st, bar):
    print("MIXCOUNTS", json.dumps(dict(name=name, device=[cnt["closest_rays"], cnt["any_rays"]], reference=[st["closest_rays"], st["any_rays"]])))
    for k in ("closest_rays", "any_rays"):
        tol = 0 if bar == "strict" else max(4, int(2e-4 * st[k]))
        assert abs(cnt[k] - st[k]) <= tol, (name, k, cnt[k], st[k])
    cam, exact = stat_int(st["stats"]["Camera Rays Traced"])          # StatsPrint writes 17424 as "17.4k": equal where it is exact, else equal as printed
    assert (cnt["camera_rays"] == cam if exact else abs(cnt["camera_rays"] - cam) <= .0005 * cam + 50), (name, cnt["camera_rays"], cam)
    assert cnt["bad_samples"] == 0, name


def render_both(pkg, text):
    """counting twin (film + counters), then the timed kernel (film)"""
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    ds.set_counting(False); ds.clear_film(); ds.render()
    trgb, talpha = ds.film()
    ds.close()
    return rgb, alpha, cnt, trgb, talpha


def test_fixtures_present():
    assert 48 <= len(MIXES) <= 64 and len(FLAVOUR_CASES) >= len(MIXES) // 3, (len(MIXES), len(FLAVOUR_CASES))


@pytest.mark.parametrize("name", MIXES)
def test_mix_matches_reference_fixture(pkg, name):
    need_gpu(pkg)
    g = load_golden("mixes/" + name)
    bar = str(g["bar"])
    rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], bar)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], bar)
    check_counts(name, cnt, g["stats"], bar)


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
        share = float((np.sqrt(((rgb.astype(np.float64) - g["rgb"]) ** 2).sum(-1)) > 1e-3).mean())
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
    monkeypatch.setenv("PBRT_HIP_PIPELINE", "0")
    ds.render()
    assert ds.last_stats()["pipeline"] == 0
    ref = ds.film_accum()
    cnt_ref = ds.counters()
    for occ in ("0", "1"):
        monkeypatch.setenv("PBRT_HIP_HIGH_OCC", occ)
        for counting in (False, True):
            ds.set_counting(counting); ds.reset_counters(); ds.clear_film(); ds.render()
            got = ds.film_accum()
            assert np.array_equal(got, ref), (name, occ, counting, float(np.abs(got - ref).max()))
            if counting:
                c = ds.counters()
                assert [c[k] for k in COUNTER_KEYS] == [cnt_ref[k] for k in COUNTER_KEYS], (name, occ, c, cnt_ref)
    monkeypatch.delenv("PBRT_HIP_HIGH_OCC")
    for env in (dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="0"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_VERTEX="1"), dict(PBRT_HIP_PIPELINE="1", PBRT_HIP_PIPE_SLOTS="512")):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            for counting in (False, True):
                ds.set_counting(counting); ds.reset_counters(); ds.clear_film(); ds.render()
                assert ds.last_stats()["pipeline"] == (0 if mega_only else 1), (name, env)
                got = ds.film_accum()
                assert np.array_equal(got, ref), (name, env, counting, float(np.abs(got - ref).max()))
                if counting:
                    c = ds.counters()
                    assert [c[k] for k in COUNTER_KEYS] == [cnt_ref[k] for k in COUNTER_KEYS], (name, env, c, cnt_ref)
    nodes, refs = ds.accel_arrays()
    info = ds.accel_info()
    ds.close()
    # rt_scene_create_prebuilt (the multi-rank path), and on it two shards of 8 x 8-pixel tiles into one film, as the ranks' films are summed
    b = pkg.DeviceScene(ps, prebuilt=(nodes, refs, info))
    b.render()
    got = b.film_accum()
    c = b.counters()
    assert np.array_equal(got, ref), (name, "prebuilt", float(np.abs(got - ref).max()))
    assert [c[k] for k in COUNTER_KEYS] == [cnt_ref[k] for k in COUNTER_KEYS], (name, "prebuilt", c, cnt_ref)
    if f["strategy"] != "weighted":
        b.reset_counters(); b.clear_film()
        try:
            for shard in range(2):
                ps.set_shard(shard, 2, (8, 8))
                b.render()
            parts = b.film_accum(); c = b.counters()
        finally:
            ps.set_shard(0, 1, 64)
        if f["filter"] == "box":
            # the box filter gives every sample to the one pixel it lies in, and a tile holds whole pixels: a pixel's sum is formed by one shard
            assert np.array_equal(parts, ref), (name, "shards", float(np.abs(parts - ref).max()))
        else:
            assert np.allclose(parts, ref, rtol=2e-5, atol=2e-6), (name, "shards", float(np.abs(parts - ref).max()))
        for k in ("camera_rays", "closest_rays", "any_rays", "bad_samples"):
            assert c[k] == cnt_ref[k], (name, "shards", k, c[k], cnt_ref[k])
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
    rgb, alpha, cnt, trgb, talpha = render_both(pkg, text)
    name = "live_%d" % (10_000 + k)
    check_bar(name, rgb, alpha, ref_rgb, ref_alpha, bar)
    check_bar(name + " timed", trgb, talpha, ref_rgb, ref_alpha, bar)
    check_counts(name, cnt, st, bar)
