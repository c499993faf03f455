"""Generate the fixtures of the three refined shapes -- heightfield, nurbs, loopsubdiv -- by running the UNMODIFIED reference (oracle/_ref), the way
tests/golden/make_debug_golden.py does for the debug integrator.  Runs only where the reference sources exist.

    python tests/golden/make_shapes_golden.py [name ...]

tests/golden/shapes/<name>.npz holds the scene text, the reference's float film (rgb, alpha) at 24 x 24 with 2 x 2 jittered samples under the keyed
sampler, its ray counts / StatsPrint table (countaccel) and `twin_share`: the share of the pixels on which the reference's film of a named WRONG
twin of the same scene is more than 1e-3 (per-pixel L2) away.  The twins: the control mesh as a plain trianglemesh, one level of subdivision
less, the heightfield with nu / nv exchanged, the patch with its u and v directions exchanged over the same control points.  Three fixtures keep
the twin's film (`twin_rgb`).  tests/golden/desc_shapes/<name>.xz is ref_runner.reference_descriptors() of desc_scene(text): the same world under a
plain sampler and accelerator (and "whitted" where the fixture's integrator is "debug", which the adapter does not stand in for), i.e. the
reference's OWN refined vertices, normals, uvs and triangle order as an rt_desc_serialize image (not for loop_level0_whitted, see there).

The generator refuses a fixture whose twin share is below 5 %, any fixture with reference stderr lines (but the one line the reference writes for
every emitter of more than 16 triangles, where a fixture says so) or non-finite values, and any file of 64 KB or more.  Fixtures are DATA (inputs + expected outputs); no reference source text is stored."""
import json
import lzma
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
from pbrt_v1_amd import scenes  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "shapes")
OUT_DESC = os.path.join(HERE, "desc_shapes")
MIN_SHARE = 0.05
MAX_BYTES = 64 * 1024

LIGHT = 'LightSource "point" "point from" [278 500 100] "color I" [300000 300000 280000]\n'
FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [756 0 -200 -200 0 -200 -200 0 760 756 0 760]\n'
JIT4 = dict(xres=24, yres=24, xsamples=2, ysamples=2, jitter=True)


def obj(shape, pre="", material='"matte" "color Kd" [.5 .5 .5]', area=""):
    return 'AttributeBegin\n%s%sMaterial %s\n%s\nAttributeEnd\n' % (pre, area, material, shape.rstrip("\n"))


def world(*parts, light=True):
    return "WorldBegin\n" + (LIGHT if light else "") + "".join(parts) + "WorldEnd\n"


def channels(red, green, blue):
    return '"string red" ["%s"] "string green" ["%s"] "string blue" ["%s"]' % (red, green, blue)


def desc_scene(text):
    """The scene whose descriptors tests/golden/desc_shapes/ pins, from a fixture's scene text (tests/test_shapes_host.py applies it too)."""
    text, n = re.subn(r'Sampler "keyed" "string inner" \["(\w+)"\] "integer seed" \[\d+\]', r'Sampler "\1"', text)
    assert n == 1
    text, n = re.subn(r'Accelerator "countaccel" "string inner" \["(\w+)"\]', r'Accelerator "\1"', text)
    assert n == 1
    return re.sub(r'^SurfaceIntegrator "debug"[^\n]*$', 'SurfaceIntegrator "whitted" "integer maxdepth" [5]', text, flags=re.M)


# ---- the shapes.  Every control mesh is small; the transforms bring it in front of the camera of scenes.options_block
HF_Z = [0.0, .3, .1, .5, .2, .6, .4, .1, .5, .2, .7, .3]
HF_PRE = "Translate 470 60 420\nRotate -35 1 0 0\nRotate 20 0 0 1\nScale -380 420 260\nReverseOrientation\n"
HF_LAMP_Z = [0.0, .05, .02, .08, .03, .1, .06, .01, .04, .07, .02, .05]
HF_LAMP_PRE = "Translate 130 480 150\nRotate 90 1 0 0\nScale 300 300 120\n"
LAMP = 'AreaLightSource "area" "color L" [14 13 11] "integer nsamples" [2]\n'
WALL = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-200 0 600 756 0 600 756 600 600 -200 600 600]\n'

NURBS_P = [[x * 1.0, y * 1.0, [[0.0, .6, -.2, .3], [.5, 1.2, .8, -.1], [.1, .4, .9, .2]][y][x]] for y in range(3) for x in range(4)]
NURBS_P_KW = dict(nu=4, uorder=3, uknots=[0, 0, 0, .5, 1, 1, 1], nv=3, vorder=3, vknots=[0, 0, 0, 1, 1, 1], P=NURBS_P, u0=.1, u1=.9)
NURBS_P_TWIN = dict(nu=3, uorder=3, uknots=[0, 0, 0, 1, 1, 1], nv=4, vorder=3, vknots=[0, 0, 0, .5, 1, 1, 1], P=NURBS_P, v0=.1, v1=.9)
NURBS_P_PRE = "Translate 100 120 450\nRotate -30 1 0 0\nScale 120 170 150\n"
S2 = float(np.sqrt(.5))
CYL_PW = [1, 0, 0, 1, S2, S2, 0, S2, 0, 1, 0, 1, 1, 0, 1, 1, S2, S2, S2, S2, 0, 1, 1, 1]          # the rational quarter circle, extruded along z
CYL_KW = dict(nu=3, uorder=3, uknots=[0, 0, 0, 1, 1, 1], nv=2, vorder=2, vknots=[0, 0, 1, 1], Pw=CYL_PW)
CYL_TWIN = dict(nu=2, uorder=2, uknots=[0, 0, 1, 1], nv=3, vorder=3, vknots=[0, 0, 0, 1, 1, 1], Pw=CYL_PW)
CYL_PRE = "Translate 120 60 520\nRotate 90 1 0 0\nRotate 200 0 0 1\nScale 330 330 -420\n"

OCTA = scenes.octahedron(260.0)
OCTA_PRE = "Translate 278 230 300\nRotate 25 1 .4 .2\n"
TETRA = scenes.tetrahedron(300.0)
TETRA_PRE = "Translate 278 260 300\nRotate 40 .3 1 .2\n"
GRID = scenes.grid_mesh(3, 3, 300.0, height=lambda x, y: 60.0 * np.sin(x / 70.0) - 40.0 * np.cos(y / 90.0))
GRID_PRE = "Translate 30 60 400\nRotate -40 1 0 0\n"
FAN = scenes.fan_mesh(5, 170.0, sweep=np.pi, lift=60.0)
FAN_PRE = "Translate 470 330 350\nRotate -30 1 0 0\nRotate 15 0 1 0\n"
UMBRELLA = scenes.fan_mesh(8, 200.0, lift=130.0, closed=True)
UMB_PRE = "Translate 160 150 350\nRotate -65 1 0 0\n"
UMB2_PRE = "Translate 430 300 420\nRotate -20 1 0 0\nRotate -35 0 1 0\n"
SMALL_OCTA = scenes.octahedron(70.0)
LAMP_PRE = "Translate 278 420 250\nRotate 30 0 1 1\n"
MIRROR = '"mirror" "color Kr" [.9 .9 .9]'


def loop(mesh, n, extra=""):
    return scenes.loopsubdiv_text(mesh[0], mesh[1], n, extra)


def plain(mesh):
    return scenes.control_mesh_text(mesh[0], mesh[1])


# name -> integrator, its parameters, the world and the twin's world; `keep`: the twin's film is stored too
CONFIGS = {
    "hf_debug": dict(integrator="debug", params=channels("u", "v", "nx"),
                     world=world(obj(FLOOR), obj(scenes.heightfield_text(4, 3, HF_Z), HF_PRE)),
                     twin=world(obj(FLOOR), obj(scenes.heightfield_text(3, 4, HF_Z), HF_PRE)), twin_name="nu / nv exchanged", keep=True),
    "hf_direct_emitter": dict(integrator="directlighting", params='"string strategy" ["all"]',
                              world=world(obj(FLOOR), obj(WALL), obj(scenes.heightfield_text(4, 3, HF_LAMP_Z), HF_LAMP_PRE, area=LAMP), light=False),
                              twin=world(obj(FLOOR), obj(WALL), obj(scenes.heightfield_text(3, 4, HF_LAMP_Z), HF_LAMP_PRE, area=LAMP), light=False),
                              twin_name="nu / nv exchanged"),
    "nurbs_p_debug": dict(integrator="debug", params=channels("snx", "u", "hit"),
                          world=world(obj(FLOOR), obj(scenes.nurbs_text(**NURBS_P_KW), NURBS_P_PRE)),
                          twin=world(obj(FLOOR), obj(scenes.nurbs_text(**NURBS_P_TWIN), NURBS_P_PRE)), twin_name="u and v exchanged", keep=True),
    "nurbs_pw_whitted": dict(integrator="whitted", params="",
                             world=world(obj(FLOOR), obj(scenes.nurbs_text(**CYL_KW), CYL_PRE, '"plastic" "color Kd" [.3 .5 .7] "float roughness" [.15]')),
                             twin=world(obj(FLOOR), obj(scenes.nurbs_text(**CYL_TWIN), CYL_PRE, '"plastic" "color Kd" [.3 .5 .7] "float roughness" [.15]')),
                             twin_name="u and v exchanged"),
    "loop_octa_whitted": dict(integrator="whitted", params="",
                              world=world(obj(FLOOR), obj(loop(OCTA, 3), OCTA_PRE, '"plastic" "color Kd" [.7 .4 .3] "float roughness" [.08]')),
                              twin=world(obj(FLOOR), obj(plain(OCTA), OCTA_PRE, '"plastic" "color Kd" [.7 .4 .3] "float roughness" [.08]')),
                              twin_name="the control mesh as a trianglemesh"),
    "loop_tetra_debug": dict(integrator="debug", params=channels("snx", "sny", "snz"),
                             world=world(obj(FLOOR), obj(loop(TETRA, 2), TETRA_PRE)),
                             twin=world(obj(FLOOR), obj(plain(TETRA), TETRA_PRE)), twin_name="the control mesh as a trianglemesh", keep=True),
    "loop_open_debug": dict(integrator="debug", params=channels("snx", "snz", "v"),
                            world=world(obj(FLOOR), obj(loop(GRID, 2), GRID_PRE), obj(loop(FAN, 2), FAN_PRE)),
                            twin=world(obj(FLOOR), obj(loop(GRID, 1), GRID_PRE), obj(loop(FAN, 1), FAN_PRE)), twin_name="nlevels - 1"),
    "loop_umbrella_path": dict(integrator="path", params="", maxdepth=4,
                               world=world(obj(FLOOR), obj(WALL), obj(loop(UMBRELLA, 2), UMB_PRE, '"matte" "color Kd" [.6 .5 .3]'), obj(loop(UMBRELLA, 2), UMB2_PRE, MIRROR)),
                               twin=world(obj(FLOOR), obj(WALL), obj(plain(UMBRELLA), UMB_PRE, '"matte" "color Kd" [.6 .5 .3]'), obj(plain(UMBRELLA), UMB2_PRE, MIRROR)),
                               twin_name="the control mesh as a trianglemesh"),
    "loop_level0_whitted": dict(integrator="whitted", params="",
                                world=world(obj(FLOOR), obj(loop(OCTA, 0), OCTA_PRE, '"plastic" "color Kd" [.4 .6 .3] "float roughness" [.1]')),
                                twin=world(obj(FLOOR), obj(plain(OCTA), OCTA_PRE, '"plastic" "color Kd" [.4 .6 .3] "float roughness" [.1]')),
                                twin_name="the control mesh as a trianglemesh",
                                # no descriptor image: at nlevels <= 0 the reference's Refine writes the limit positions into the control vertices
                                # themselves (loopsubdiv.cpp:369-370 with v == vertices), and the adapter's run refines every shape twice -- once for the
                                # inner accelerator, once for the dump --, so its image is of the surface pushed twice.  The film above is of one push.
                                desc=False),
    # nlevels left to its default of 3, "scheme" given
    "loop_default_whitted": dict(integrator="whitted", params="",
                                 world=world(obj(FLOOR), obj(loop(TETRA, None, '"string scheme" ["loop"]'), TETRA_PRE, '"matte" "color Kd" [.2 .6 .8]')),
                                 twin=world(obj(FLOOR), obj(plain(TETRA), TETRA_PRE, '"matte" "color Kd" [.2 .6 .8]')),
                                 twin_name="the control mesh as a trianglemesh"),
    "loop_emitter_direct": dict(integrator="directlighting", params='"string strategy" ["all"]',
                                world=world(obj(FLOOR), obj(WALL), obj(loop(SMALL_OCTA, 1), LAMP_PRE, area=LAMP), light=False),
                                twin=world(obj(FLOOR), obj(WALL), obj(loop(SMALL_OCTA, 0), LAMP_PRE, area=LAMP), light=False), twin_name="nlevels - 1",
                                # area.cpp:50-52: "Area light geometry turned into 32 shapes; may be very inefficient." -- the one line an emitter of more
                                # than 16 triangles always gets; the twin's 8 triangles get none
                                stderr_lines=1),
}


def scene_text(name, twin=False):
    c = CONFIGS[name]
    kw = dict(keyed=True, count=True, integrator=c["integrator"], integrator_params=c["params"], maxdepth=c.get("maxdepth", 5), **JIT4)
    return scenes.options_block(**kw) + c["twin" if twin else "world"]


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    os.makedirs(OUT_DESC, exist_ok=True)
    for name, c in CONFIGS.items():
        if only and name not in only:
            continue
        text = scene_text(name)
        rgb, alpha, st = REF.run_reference(text, keyed=True)
        trgb, talpha, tst = REF.run_reference(scene_text(name, twin=True), keyed=True)
        share = float((np.sqrt(((rgb - trgb) ** 2).sum(-1)) > 1e-3).mean())
        print(name, rgb.shape, "mean", rgb.reshape(-1, 3).mean(0), "max", float(rgb.max()), "alpha", float(alpha.min()), float(alpha.max()),
              {k: st[k] for k in ("closest_rays", "any_rays")}, "triangles", st["stats"].get("Triangles created"),
              "stderr lines", st["stderr_lines"], tst["stderr_lines"], "differs from its twin on %.3f" % share)
        assert np.isfinite(rgb).all() and np.isfinite(alpha).all() and st["stderr_lines"] == c.get("stderr_lines", 0), name
        assert np.isfinite(trgb).all() and tst["stderr_lines"] == 0, name
        assert share >= MIN_SHARE, "%s: only %.3f of the pixels differ from the twin's film" % (name, share)
        extra = dict(twin_rgb=trgb) if c.get("keep") else {}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st)), twin_share=np.array(share),
                            twin=np.array(c["twin_name"]), **extra)
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))
        if not c.get("desc", True):
            continue
        desc = REF.reference_descriptors(desc_scene(text))
        dpath = os.path.join(OUT_DESC, name + ".xz")
        open(dpath, "wb").write(lzma.compress(desc, preset=9))
        print("   descriptors", len(desc), "bytes,", os.path.getsize(dpath), "compressed")
        assert os.path.getsize(dpath) < MAX_BYTES, (name, os.path.getsize(dpath))


if __name__ == "__main__":
    main()
