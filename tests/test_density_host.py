"""Host front end of the density media (Volume "exponential" / "volumegrid": volumes/exponential.cpp:54-69, volumes/volumegrid.cpp:85-110,
pbrtVolume api.cpp:403-409): parameters and defaults, the CTM as world_to_volume, the factory errors, the one-region rule, and the
descriptor images that must not move.  CPU only."""
import numpy as np
import pytest


def text_with(scenes, world):
    hdr = scenes.options_block(xres=16, yres=16, integrator="whitted", volume_integrator='"single" "float stepsize" [40]')
    return hdr + 'WorldBegin\nLightSource "point" "point from" [278 500 200] "color I" [100000 100000 100000]\n' + world + "WorldEnd\n"


def parse(pkg, scenes, world, quiet=True):
    return pkg.ParsedScene(text=text_with(scenes, world), quiet=quiet)


def test_exponential_defaults(pkg, scenes):
    ps = parse(pkg, scenes, 'Volume "exponential"\n')
    assert ps.valid and ps.errors == 0 and ps.warnings == 0
    v = ps.volume()
    assert v["p0"] == [0, 0, 0] and v["p1"] == [1, 1, 1] and v["sigma_a"] == [0, 0, 0] and v["sigma_s"] == [0, 0, 0]
    assert v["le"] == [0, 0, 0] and v["g"] == 0
    assert v["density"] == {"kind": "exponential", "a": 1.0, "b": 1.0, "updir": [0.0, 1.0, 0.0]}
    assert np.array_equal(v["world_to_volume"], np.eye(4, dtype=np.float32))


def test_exponential_parameters_and_updir_normalisation(pkg, scenes):
    ps = parse(pkg, scenes, 'Volume "exponential" "float a" [2.5] "float b" [.125] "vector updir" [3 4 0] "color sigma_a" [.1 .2 .3] '
                            '"color sigma_s" [.4 .5 .6] "color Le" [1 2 3] "float g" [-.25] "point p0" [5 6 7] "point p1" [-1 10 2]\n')
    assert ps.errors == 0 and ps.warnings == 0
    v = ps.volume()
    d = v["density"]
    assert d["kind"] == "exponential" and d["a"] == 2.5 and d["b"] == 0.125
    inv = np.float32(1) / np.sqrt(np.float32(25))                    # Normalize: v * (1.f / Length())
    assert d["updir"] == [float(np.float32(3) * inv), float(np.float32(4) * inv), 0.0]
    assert v["p0"] == [-1, 6, 2] and v["p1"] == [5, 10, 7]          # BBox(p0, p1) takes the per-axis min / max
    assert np.allclose(v["sigma_a"], [.1, .2, .3]) and np.allclose(v["sigma_s"], [.4, .5, .6]) and v["le"] == [1, 2, 3] and v["g"] == -0.25


def test_ctm_becomes_world_to_volume(pkg, scenes):
    for kind, extra in (("exponential", ""), ("volumegrid", ' "float density" [1]')):
        ps = parse(pkg, scenes, 'AttributeBegin\nTranslate 10 20 30\nScale 2 4 8\nVolume "%s"%s\nAttributeEnd\n' % (kind, extra))
        m = ps.volume()["world_to_volume"]
        want = np.array([[.5, 0, 0, -5], [0, .25, 0, -5], [0, 0, .125, -3.75], [0, 0, 0, 1]], np.float32)
        assert np.allclose(m, want, atol=1e-6), (kind, m)


def test_volumegrid_parameters(pkg, scenes):
    vals = np.arange(2 * 3 * 4, dtype=np.float32) * 0.25
    ps = parse(pkg, scenes, 'Volume "volumegrid" "integer nx" [2] "integer ny" [3] "integer nz" [4] "point p1" [10 20 30] "float density" [%s]\n'
               % " ".join(repr(float(x)) for x in vals))
    assert ps.errors == 0 and ps.warnings == 0
    d = ps.volume()["density"]
    assert (d["kind"], d["nx"], d["ny"], d["nz"]) == ("volumegrid", 2, 3, 4)
    assert np.array_equal(d["values"].ravel(), vals) and d["values"].shape == (4, 3, 2)     # density[z*nx*ny + y*nx + x]
    ps1 = parse(pkg, scenes, 'Volume "volumegrid" "float density" [0.5]\n')                   # nx, ny, nz default to 1
    d1 = ps1.volume()["density"]
    assert (d1["nx"], d1["ny"], d1["nz"]) == (1, 1, 1) and d1["values"].ravel().tolist() == [0.5]


def test_volumegrid_factory_errors_leave_no_region(pkg, scenes, capfd):
    ps = parse(pkg, scenes, 'Volume "volumegrid" "integer nx" [2]\n', quiet=False)
    err = capfd.readouterr().err
    assert 'No "density" values provided for volume grid?' in err and 'Parameter "nx" not used' in err     # ReportUnused after a NULL factory
    assert ps.errors == 1 and ps.valid and ps.volume() is None
    ps = parse(pkg, scenes, 'Volume "volumegrid" "integer nx" [2] "integer ny" [2] "float density" [1 2 3]\n', quiet=False)
    assert "VolumeGrid has 3 density values but nx*ny*nz = 4" in capfd.readouterr().err
    assert ps.errors == 1 and ps.valid and ps.volume() is None
    # a rejected grid is not the scene's one region: a homogeneous region after it is kept
    ps = parse(pkg, scenes, 'Volume "volumegrid" "integer nx" [2] "float density" [1]\nVolume "homogeneous" "color sigma_a" [.5 .5 .5]\n')
    assert ps.errors == 1 and ps.volume() is not None and ps.volume()["density"] is None and ps.volume()["sigma_a"] == [.5, .5, .5]


@pytest.mark.parametrize("dims", [(0, 1, 1), (-1, -1, 1), (2048, 2048, 1024), (65536, 65536, 2)])
def test_volumegrid_counts_must_be_positive_and_fit(pkg, scenes, dims, capfd):
    ps = parse(pkg, scenes, 'Volume "volumegrid" "integer nx" [%d] "integer ny" [%d] "integer nz" [%d] "float density" [1]\n' % dims, quiet=False)
    assert "is not a positive count below 2^31" in capfd.readouterr().err
    assert ps.errors == 1 and ps.valid and ps.volume() is None and not ps.density_desc()


def test_one_region_rule_unchanged(pkg, scenes, capfd):
    for first, second in (('"homogeneous"', '"exponential"'), ('"exponential"', '"homogeneous"'),
                          ('"volumegrid" "float density" [1]', '"exponential"'), ('"exponential" "float a" [3]', '"volumegrid" "float density" [1]')):
        ps = parse(pkg, scenes, "Volume %s\nVolume %s\n" % (first, second), quiet=False)
        assert "Only one volume region is supported" in capfd.readouterr().err
        assert ps.errors == 1 and ps.valid
        d = ps.volume()["density"]
        assert (d["kind"] if d else "homogeneous") == first.split('"')[1]
        if "float a" in first:
            assert d["a"] == 3.0


def test_unknown_region_still_refused(pkg, scenes, capfd):
    ps = parse(pkg, scenes, 'Volume "aggregate"\n', quiet=False)
    assert 'Unable to load plugin "aggregate"' in capfd.readouterr().err and ps.volume() is None


def test_descriptor_image_of_homogeneous_scenes_unchanged(pkg, scenes):
    """RtVolume / RtSceneDesc / rt_desc_serialize carry no trace of a density region: a scene serialises to the same bytes whichever
    kind its region is, and a homogeneous scene hands no density descriptor over."""
    common = '"color sigma_a" [.002 .002 .002] "color sigma_s" [.003 .003 .003] "point p1" [556 549 559] "color Le" [.1 .2 .3] "float g" [.2]'
    homo = scenes.cornell_scene(xres=16, yres=16, integrator="directlighting", volume_integrator='"single" "float stepsize" [40]',
                                world_kwargs=dict(extra='AttributeBegin\nRotate 10 0 1 0\nVolume "homogeneous" %s\nAttributeEnd\n' % common))
    ph = pkg.ParsedScene(text=homo)
    assert ph.valid and not ph.density_desc() and ph.volume()["density"] is None
    for other in ('"exponential" "float a" [2] "vector updir" [1 1 0]', '"volumegrid" "integer nx" [2] "float density" [1 2]'):
        pd = pkg.ParsedScene(text=homo.replace('"homogeneous"', other))
        assert pd.valid and pd.density_desc()
        assert pd.serialize() == ph.serialize()
