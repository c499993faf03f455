"""Host front end of the bidirectional integrator (integrators/bidirectional.cpp:211-213: a factory that reads no parameter): the directive, its
unused parameters, the names that stay errors, a descriptor image that must not move, and the fixtures of tests/golden/bidir/.  CPU only."""
import glob
import hashlib
import os

import numpy as np

from conftest import GOLDEN, load_golden

TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\n'
POINT = 'LightSource "point" "point from" [1 2 3]\n'


def parse(pkg, scenes, integrator, params=""):
    hdr = scenes.options_block(xres=16, yres=16, integrator=integrator, integrator_params=params)
    return pkg.ParsedScene(text=hdr + "WorldBegin\n" + POINT + TRI + "WorldEnd\n")


def test_bidirectional_is_a_surface_integrator(pkg, scenes):
    """Before the device rendered this integrator the directive was an Error ("Unable to load plugin") and the frame invalid."""
    ps = parse(pkg, scenes, "bidirectional")
    assert ps.valid and ps.errors == 0 and ps.warnings == 0
    assert ps.integrator == 3 and ps.render_view()["integrator"] == 3


def test_options_block_gives_no_maxdepth(scenes):
    assert 'SurfaceIntegrator "bidirectional" \n' in scenes.options_block(integrator="bidirectional")


def test_every_parameter_is_reported_unused(pkg, scenes):
    """The reference's factory looks nothing up, so ParamSet::ReportUnused names every parameter given -- maxdepth too."""
    ps = parse(pkg, scenes, "bidirectional", '"integer maxdepth" [3]')
    assert ps.valid and ps.errors == 0 and ps.warnings == 1 and ps.integrator == 3
    ps = parse(pkg, scenes, "bidirectional", '"integer maxdepth" [3] "string strategy" ["one"]')
    assert ps.valid and ps.errors == 0 and ps.warnings == 2 and ps.integrator == 3


def test_other_names_stay_errors(pkg, scenes):
    for name in ("Bidirectional", "igi"):
        ps = parse(pkg, scenes, name)
        assert ps.errors >= 1 and not ps.valid, name


def test_existing_descriptor_does_not_move(pkg):
    """serialize() of a scene that was there before gives the SHA-256 of the image the parent commit gave (tests/test_infinite_host.py holds the same value)."""
    ps = pkg.ParsedScene(text=load_golden("direct_spot_area")["scene"])
    assert ps.errors == 0 and ps.integrator == 1
    assert hashlib.sha256(ps.serialize()).hexdigest() == "b9e1e8fc003a80bcb82cad4a2546f75c81447be404622824f5f72055e07469f9"


def test_fixtures_present():
    names = sorted(glob.glob(os.path.join(GOLDEN, "bidir", "*.npz")))
    assert len(names) >= 8, names
    for p in names:
        z = np.load(p)
        assert os.path.getsize(p) < 64 * 1024, p
        assert float(z["path_share"]) >= 0.05, (p, float(z["path_share"]))
        assert z["rgb"].shape[0] in (24, 32) and np.isfinite(z["rgb"]).all()


def test_fixture_scenes_parse_without_errors(pkg):
    for p in sorted(glob.glob(os.path.join(GOLDEN, "bidir", "*.npz"))):
        name = os.path.basename(p)[:-4]
        ps = pkg.ParsedScene(text=load_golden("bidir/" + name)["scene"])
        assert ps.valid and ps.errors == 0 and ps.warnings == 0 and ps.integrator == 3 and ps.n_lights >= 1, name
