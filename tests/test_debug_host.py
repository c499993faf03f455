"""Host front end of the debug integrator (integrators/debug.cpp:135-166): the directive and its three channel names, the codes in the order of
the reference's DebugVariable, the unknown name that becomes `zero`, the unused parameters, the name that stays an error, how the render
descriptor carries the codes, descriptor images that must not move, and the fixtures of tests/golden/debug/.  CPU only."""
import ctypes as C
import glob
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\n'
POINT = 'LightSource "point" "point from" [1 2 3]\n'
NAMES = ("u", "v", "nx", "ny", "nz", "snx", "sny", "snz", "one", "zero", "hit")        # debug.cpp:33-44
FIXTURES = ("debug_default_uv", "debug_normals_mesh", "debug_ns_reversed", "debug_quadrics_grid", "debug_one_zero", "debug_medium_emission",
            "debug_lens_gauss_crop", "debug_soup_ortho")


def parse(pkg, scenes, integrator="debug", params=""):
    hdr = scenes.options_block(xres=16, yres=16, integrator=integrator, integrator_params=params)
    return pkg.ParsedScene(text=hdr + "WorldBegin\n" + POINT + TRI + "WorldEnd\n")


def codes(ps):
    s = ps.render_view()["strategy"]
    return s & 0xff, (s >> 8) & 0xff, (s >> 16) & 0xff, s >> 24


def test_defaults(pkg, scenes):
    """Before the device rendered this integrator the directive was an Error ("Unable to load plugin") and the frame invalid."""
    ps = parse(pkg, scenes)
    assert ps.valid and ps.errors == 0 and ps.warnings == 0
    assert ps.integrator == pkg.RT_INTEGRATOR_DEBUG == 0x100 and ps.render_view()["integrator"] == 0x100
    assert ps.debug_channels == ("u", "v", "zero")
    assert codes(ps) == (pkg.RT_DEBUG_U, pkg.RT_DEBUG_V, pkg.RT_DEBUG_ZERO, 0)


def test_code_constants(pkg):
    assert pkg.RT_DEBUG_NAMES == NAMES
    assert [getattr(pkg, "RT_DEBUG_" + n.upper()) for n in NAMES] == list(range(11))


@pytest.mark.parametrize("position", (0, 1, 2))
def test_every_name_in_every_position(pkg, scenes, position):
    channel = ("red", "green", "blue")[position]
    for code, name in enumerate(NAMES):
        ps = parse(pkg, scenes, params='"string %s" ["%s"]' % (channel, name))
        want = [0, 1, 9]
        want[position] = code
        assert ps.valid and ps.errors == 0 and ps.warnings == 0, (channel, name)
        assert codes(ps) == tuple(want) + (0,), (channel, name)
        assert ps.debug_channels[position] == name


def test_unknown_name_becomes_zero(pkg, scenes):
    ps = parse(pkg, scenes, params='"string red" ["depth"]')
    assert ps.errors == 1 and ps.valid and ps.integrator == 0x100
    assert codes(ps) == (pkg.RT_DEBUG_ZERO, pkg.RT_DEBUG_V, pkg.RT_DEBUG_ZERO, 0)
    ps = parse(pkg, scenes, params='"string green" ["U"]')                              # the names are case-sensitive
    assert ps.errors == 1 and ps.valid and ps.debug_channels == ("u", "zero", "zero")


def test_other_parameters_are_reported_unused(pkg, scenes):
    ps = parse(pkg, scenes, params='"integer maxdepth" [3]')
    assert ps.valid and ps.errors == 0 and ps.warnings == 1 and ps.integrator == 0x100
    ps = parse(pkg, scenes, params='"integer maxdepth" [3] "string blue" ["hit"] "string strategy" ["one"]')
    assert ps.valid and ps.errors == 0 and ps.warnings == 2 and ps.debug_channels == ("u", "v", "hit")


def test_capitalised_name_stays_an_unknown_plugin(pkg, scenes):
    ps = parse(pkg, scenes, integrator="Debug")
    assert ps.errors >= 1 and not ps.valid


def test_other_integrators_have_no_channels(pkg, scenes):
    ps = parse(pkg, scenes, integrator="whitted")
    assert ps.integrator == 0 and ps.debug_channels is None


def test_descriptor_packs_the_codes(pkg, scenes):
    """strategy = red | green << 8 | blue << 16 in a descriptor of the parent commit's size and offsets; render_struct() is the descriptor itself."""
    assert C.sizeof(pkg.RtRenderDesc) == 1128                                         # sizeof(RtRenderDesc) of the parent commit's header
    assert pkg.RtRenderDesc.strategy.offset == 8 and pkg.RtRenderDesc.filter_table.offset == 92 and pkg.RtRenderDesc.shard_index.offset == 1116
    ps = parse(pkg, scenes, params='"string red" ["snz"] "string green" ["hit"] "string blue" ["nx"]')
    rd = ps.render_struct()
    assert rd.integrator == 0x100 and rd.strategy == (7 | 10 << 8 | 2 << 16)
    assert (rd.x_res, rd.y_res, rd.shard_count) == (16, 16, 1)
    rd.strategy = 11
    assert ps.render_view()["strategy"] == 11 and ps.debug_channels == ("?", "u", "u")
    # the serialised frame carries kind, maxDepth and strategy as before: another set of channels is another image of the same length
    a = parse(pkg, scenes).serialize()
    b = parse(pkg, scenes, params='"string blue" ["one"]').serialize()
    assert len(a) == len(b) and a != b


def test_existing_descriptors_do_not_move(pkg):
    """serialize() of scenes that were there before: the SHA-256 values tests/test_materials_host.py and tests/test_bidir_host.py pin."""
    for name, sha in (("plastic_whitted", "6044150839fb80d1951125c816b42add70272de79f9a50c541c793ee4519e1c3"),
                      ("direct_spot_area", "b9e1e8fc003a80bcb82cad4a2546f75c81447be404622824f5f72055e07469f9")):
        ps = pkg.ParsedScene(text=load_golden(name)["scene"])
        assert ps.errors == 0 and hashlib.sha256(ps.serialize()).hexdigest() == sha, name


def test_fixtures_present():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "debug", "*.npz")))
    assert names == sorted(FIXTURES), names
    for name in names:
        p = os.path.join(GOLDEN, "debug", name + ".npz")
        z = np.load(p)
        assert os.path.getsize(p) < 64 * 1024, p
        assert float(z["twin_share"]) >= 0.05, (p, float(z["twin_share"]))
        assert np.isfinite(z["rgb"]).all() and np.isfinite(z["alpha"]).all() and z["rgb"].shape[:2] == z["alpha"].shape, p
        assert np.abs(z["alpha"] - 1).max() <= 1e-6, p                                # debug.cpp:69: alpha is 1 on the misses too
        if name in ("debug_default_uv", "debug_normals_mesh", "debug_quadrics_grid"):
            assert z["twin_rgb"].shape == z["rgb"].shape and np.isfinite(z["twin_rgb"]).all(), p


def test_fixture_scenes_parse_without_errors(pkg):
    for name in FIXTURES:
        ps = pkg.ParsedScene(text=load_golden("debug/" + name)["scene"])
        assert ps.valid and ps.errors == 0 and ps.warnings == 0 and ps.integrator == 0x100 and ps.n_lights >= 1, name
        assert all(c in NAMES for c in ps.debug_channels), name
