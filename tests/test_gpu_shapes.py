"""Shape "heightfield", "nurbs" and "loopsubdiv" on the device against the unmodified reference: the fixtures of tests/golden/shapes/
(tests/golden/make_shapes_golden.py), the kernel flavours, rt_scene_create_prebuilt and a two-shard split against one frame, the wrong twins as other
films.  The host refines each shape into one triangle mesh (csrc/host/shape_refine.h; tests/test_shapes_host.py pins the tessellation itself), so
these are triangle scenes: the debug, Whitted and DirectLighting fixtures are held to the strict bar of DESIGN.md 9.2 -- every pixel's rgb and alpha
within 1e-5, ray counts equal --, the path fixture to the loose one.  No allow-list.  Every frame is 24 x 24."""
import pytest

from conftest import load_golden
from gpu_checks import (PIPELINE_ENVS, assert_flavours_agree, assert_prebuilt_agrees, assert_two_shards_agree, check_bar, check_counts,
                        differing_share, fixture_names, need_gpu, render_both)

pytestmark = pytest.mark.gpu

ALL = fixture_names("shapes")
LOOSE = ("loop_umbrella_path",)                        # the path integrator's bar; every other fixture is strict
ONE_PER_SHAPE = ("hf_direct_emitter", "nurbs_pw_whitted", "loop_open_debug")
TWIN_KEPT = ("hf_debug", "nurbs_p_debug", "loop_tetra_debug")


def test_fixtures_present():
    assert len(ALL) == 11 and set(LOOSE + ONE_PER_SHAPE + TWIN_KEPT) <= set(ALL), ALL


@pytest.mark.parametrize("name", ALL)
def test_film_matches_reference_fixture(pkg, name):
    """Counting twin (film + ray counts) and timed kernel against the reference's film; the scene parses without errors into the reference's
    number of triangles ("Triangles created" counts an emitter's triangles twice: once for the primitive, once for the AreaLight's ShapeSet)."""
    need_gpu(pkg)
    g = load_golden("shapes/" + name)
    ps, rgb, alpha, cnt, trgb, talpha = render_both(pkg, g["scene"])
    assert ps.errors == 0 and ps.n_tris + ps.n_light_tris == int(g["stats"]["stats"]["Triangles created"]), (name, ps.n_tris, ps.n_light_tris)
    loose = name in LOOSE
    check_bar(name, rgb, alpha, g["rgb"], g["alpha"], loose)
    check_bar(name + " timed", trgb, talpha, g["rgb"], g["alpha"], loose)
    check_counts(name, cnt, g["stats"], loose)


@pytest.mark.parametrize("name", ONE_PER_SHAPE)
def test_flavours_prebuilt_scene_and_two_shards_agree(pkg, name):
    """Timed kernel and counting twin under both PBRT_HIP_HIGH_OCC settings and under the queue pipeline (a debug frame always runs its own
    megakernel), rt_scene_create_prebuilt, and two shards of 8 x 8 tiles summed under the box filter: the film and the counters of one frame."""
    need_gpu(pkg)
    ps = pkg.ParsedScene(text=load_golden("shapes/" + name)["scene"])
    ds = pkg.DeviceScene(ps)
    ref, cnt_ref = assert_flavours_agree(ds, name, PIPELINE_ENVS, expect_pipeline=0 if name.endswith("_debug") else 1)
    ds.close()
    b = assert_prebuilt_agrees(pkg, ps, ref, cnt_ref)
    assert_two_shards_agree(ps, b, ref, cnt_ref, exact=True)
    b.close()


@pytest.mark.parametrize("name", TWIN_KEPT)
def test_the_twin_film_is_another_film(pkg, name):
    """The device's film is as far from the reference's film of the wrong twin (nu / nv exchanged, u and v exchanged, the control mesh as a
    plain trianglemesh) as the fixture's own film is."""
    need_gpu(pkg)
    g = load_golden("shapes/" + name)
    assert float(g["twin_share"]) >= 0.05
    rgb, _, _, _ = pkg.render_text(g["scene"])
    share = differing_share(rgb, g["twin_rgb"])
    print(name, "differs from its twin", str(g["twin"]), "on", share)
    assert share >= 0.05, (name, share)
