"""The scene's device memory across frames and scenes (rt_host.h RtScene: every buffer, event and the stream is an owning member): a pool, a sample
buffer and the weighted tables that regrow between two frames of one scene, and scenes created and destroyed in a row -- one of them refused
half-way through rt_scene_create -- must leave every film bit for bit what a fresh scene renders.  Fixture-sized frames (1-2 k camera samples)."""
import numpy as np
import pytest

from conftest import load_golden
from gpu_checks import need_gpu

pytestmark = pytest.mark.gpu

COUNTERS = ("camera_rays", "closest_rays", "any_rays", "nodes_visited", "leaf_refs", "tri_tests", "bad_samples")


def parsed(pkg, name):
    ps = pkg.ParsedScene(text=load_golden(name)["scene"])
    assert ps.valid and ps.errors == 0, name
    return ps


@pytest.mark.parametrize("name", ["density/dens_grid_xform_path", "textures/nested_mix_plastic_direct"])
def test_pool_regrows_between_frames(pkg, monkeypatch, name):
    """The queue pipeline's pool at 256 slots, 512, then the default (the whole frame): every step regrows the planes, the per-slot scratch (recursion
    frames / the medium's march state / the resolved-material levels behind the scene's own materials) and rebinds them; film and counters stay the megakernel's."""
    need_gpu(pkg)
    monkeypatch.delenv("PBRT_HIP_PIPE_MEM_MB", raising=False)
    ds = pkg.DeviceScene(parsed(pkg, name))
    monkeypatch.setenv("PBRT_HIP_PIPELINE", "0")
    ds.render()
    ref, cnt_ref = ds.film_accum(), ds.counters()
    assert ds.last_stats()["pipeline"] == 0 and ref.any()
    monkeypatch.setenv("PBRT_HIP_PIPELINE", "1")
    slots = []
    for knob in ("256", "512", None):
        if knob is None:
            monkeypatch.delenv("PBRT_HIP_PIPE_SLOTS")
        else:
            monkeypatch.setenv("PBRT_HIP_PIPE_SLOTS", knob)
        ds.reset_counters(); ds.clear_film(); ds.render()
        st, got, cnt = ds.last_stats(), ds.film_accum(), ds.counters()
        print(name, "PBRT_HIP_PIPE_SLOTS", knob, "slots", st["slots"], "iterations", st["iterations"], cnt)
        assert st["pipeline"] == 1, (name, knob)
        slots.append(st["slots"])
        assert np.array_equal(got, ref), (name, knob, float(np.abs(got - ref).max()))
        for k in COUNTERS:
            assert cnt[k] == cnt_ref[k], (name, knob, k, cnt[k], cnt_ref[k])
    ds.close()
    assert slots[0] < slots[1] < slots[2], slots


def test_sample_buffer_regrows_after_a_shard(pkg, monkeypatch):
    """bidir/bidir_cornell: shard 0 of 2 (8 x 8-pixel tiles) sizes the sample buffer for half the frame; the whole frame that follows on the same scene regrows
    it (and is gathered from it) and must be a fresh scene's film."""
    need_gpu(pkg)
    monkeypatch.delenv("PBRT_HIP_PIPE_MEM_MB", raising=False)
    ps = parsed(pkg, "bidir/bidir_cornell")
    fresh = pkg.DeviceScene(ps)
    fresh.render()
    ref = fresh.film_accum()
    fresh.close()
    ds = pkg.DeviceScene(ps)
    try:
        ps.set_shard(0, 2, (8, 8))
        ds.bind_film(); ds.clear_film(); ds.render()
        part = ds.film_accum()
    finally:
        ps.set_shard(0, 1, 64)
    ds.clear_film(); ds.render()
    got = ds.film_accum()
    ds.close()
    assert ref.any() and part.any() and not np.array_equal(part, ref)
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())


def test_weighted_tables_are_reused(pkg, monkeypatch):
    """materials/transl_sheet_direct_weighted (one shard by design): the first frame allocates the tables of the recurrence (point counts, survey records, picks,
    scan sums, the page-locked total), the second reuses them; both are a fresh scene's film."""
    need_gpu(pkg)
    monkeypatch.delenv("PBRT_HIP_PIPE_MEM_MB", raising=False)
    ps = parsed(pkg, "materials/transl_sheet_direct_weighted")
    fresh = pkg.DeviceScene(ps)
    fresh.render()
    ref, points = fresh.film_accum(), fresh.last_stats()["weighted_points"]
    fresh.close()
    ds = pkg.DeviceScene(ps)
    ds.render()
    first = ds.film_accum()
    ds.clear_film(); ds.render()
    second, st = ds.film_accum(), ds.last_stats()
    ds.close()
    assert ref.any() and points > 0 and st["weighted_points"] == points
    assert np.array_equal(first, ref) and np.array_equal(second, first), (float(np.abs(first - ref).max()), float(np.abs(second - first).max()))


def test_scenes_created_and_destroyed_in_a_row(pkg):
    """textures/shiny_medium_direct three times -- create, render, close -- then an rt_scene_create that fails AFTER its uploads (an unknown material type: the
    half-built scene is released by the same destructors), then the scene once more: every film is the first one's."""
    need_gpu(pkg)
    ps = parsed(pkg, "textures/shiny_medium_direct")
    films = []
    for _ in range(3):
        ds = pkg.DeviceScene(ps)
        ds.render()
        films.append(ds.film_accum())
        ds.close()
    tab = pkg.host_lib().pbrt_host_materials(ps.scene_desc)
    keep = tab[0].type
    try:
        tab[0].type = 7
        with pytest.raises(pkg.RtError) as e:
            pkg.DeviceScene(ps)
        assert "unknown material type" in str(e.value), str(e.value)
    finally:
        tab[0].type = keep
    ds = pkg.DeviceScene(ps)
    ds.render()
    films.append(ds.film_accum())
    ds.close()
    assert films[0].any()
    for i, f in enumerate(films[1:], 1):
        assert np.array_equal(f, films[0]), (i, float(np.abs(f - films[0]).max()))
