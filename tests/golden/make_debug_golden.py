"""Generate the debug-integrator fixtures in tests/golden/debug/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref_keyed with its debug.so
plugin under the keyed sampler, and the countaccel wrapper for ray counts), the way tests/golden/make_bidir_golden.py does for the bidirectional
integrator.  Runs only where the reference sources exist.

    python tests/golden/make_debug_golden.py [name ...]

Each <name>.npz holds the scene text, the reference's float film (rgb, alpha), its ray counts / StatsPrint table and `twin_share`: the share of the
pixels on which the reference's film of a named WRONG twin of the same scene (channels exchanged, the geometric normal where the shading normal is
asked, the medium left out ...) is more than 1e-3 (per-pixel L2) away; `twin` names the twin, and three fixtures keep its film (`twin_rgb`).  The
generator refuses a fixture whose share is below 5 % -- the frame could not tell the two apart -- and any fixture with reference stderr lines or
non-finite values.  Every scene carries a light, which the integrator ignores: without one the reference warns on stderr.  The frames are 24 x 24
at 2 x 2 samples unless said otherwise.  Fixtures are DATA (inputs + expected outputs); no reference source text is stored."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
from pbrt_v1_amd import scenes  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "debug")
MIN_SHARE = 0.05
MAX_BYTES = 64 * 1024

LIGHT = 'LightSource "point" "point from" [278 500 100] "color I" [300000 300000 280000]\n'
FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [756 0 -200 -200 0 -200 -200 0 760 756 0 760]\n'
# one half of the frame: a quad whose "uv" reach 2 and 3, and above it a tilted quad without uvs (GetUVs' defaults)
QUAD_UV = ('Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-150 -130 300 278 -130 300 278 265 300 -150 265 300] '
           '"float uv" [0 0 2 0 2 3 0 3]\n')
QUAD_PLAIN = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-150 285 500 278 285 600 278 700 600 -150 700 500]\n'
ORTHO = 'Camera "orthographic" "float screenwindow" [-300 300 -290 290]'
JIT4 = dict(xsamples=2, ysamples=2, jitter=True)


def obj(shape, pre="", material='"matte" "color Kd" [.5 .5 .5]'):
    return 'AttributeBegin\n%sMaterial %s\n%s\nAttributeEnd\n' % (pre, material, shape.rstrip("\n"))


def world(*parts):
    return "WorldBegin\n" + LIGHT + "".join(parts) + "WorldEnd\n"


def channels(red, green, blue):
    return '"string red" ["%s"] "string green" ["%s"] "string blue" ["%s"]' % (red, green, blue)


def soup(n=300, seed=77):
    """n triangles of the LCG soup, grown so that a 24 x 24 frame sees them"""
    t = scenes.lcg_soup(n, seed).astype(np.float64)
    c = t.mean(axis=1, keepdims=True)
    return scenes.soup_shape_text((c + (t - c) * 9.0).astype(np.float32))


HALF = world(obj(QUAD_UV), obj(QUAD_PLAIN))
MESH_N = obj(scenes.smooth_mesh_text(radius=170.0, nu=12, nv=8, squash=(1.0, .8, 1.0)), "Translate 278 175 300\n")
MESH_NS = obj(scenes.smooth_mesh_text(radius=190.0, nu=10, nv=6, with_s=True, squash=(1.0, .7, 1.0)), "Translate 278 250 300\nScale -1 1 1\nReverseOrientation\n")
QUADRICS = (obj('Shape "sphere" "float radius" [120] "float phimax" [250] "float zmin" [-70]', "Translate 170 300 300\nRotate 40 1 1 0\n") +
            obj('Shape "disk" "float radius" [130] "float innerradius" [40]', "Translate 400 380 350\nRotate 160 1 0.2 0\n") +
            obj('Shape "cylinder" "float radius" [70] "float zmin" [-100] "float zmax" [120]', "Translate 400 130 300\nRotate 70 1 0.3 0.2\n"))

# name -> options, the integrator's parameters, the world, the twin (as parameters, or "no volume"); `keep`: the twin's film is stored too
CONFIGS = {
    # 1. no parameters: u v zero.  Mesh uvs beyond 1 next to GetUVs' defaults; the other half of the frame sees nothing
    "debug_default_uv": dict(opts=dict(xres=24, yres=24, **JIT4), params="", world=HALF, twin=channels("v", "u", "zero"), keep=True),
    # 2. geometric against shading normal on a mesh with per-vertex N over a floor
    "debug_normals_mesh": dict(opts=dict(xres=24, yres=24, **JIT4), params=channels("nx", "snx", "hit"), world=world(obj(FLOOR), MESH_N),
                               twin=channels("nx", "nx", "hit"), keep=True),
    # 3. N and S under ReverseOrientation and a mirroring transform: the flips of both normals
    "debug_ns_reversed": dict(opts=dict(xres=24, yres=24, **JIT4), params=channels("sny", "snz", "ny"), world=world(obj(FLOOR), MESH_NS),
                              twin=channels("ny", "nz", "ny")),
    # 4. a partial sphere, an annulus and a cylinder in the grid under the lowdiscrepancy sampler: the quadrics' own (u, v) and normals
    "debug_quadrics_grid": dict(opts=dict(xres=24, yres=24, sampler="lowdiscrepancy", pixelsamples=4, accelerator="grid"), params=channels("u", "v", "nz"),
                                world=world(QUADRICS), twin=channels("v", "u", "nz"), keep=True),
    # 5. the constants, and alpha = 1 where nothing is hit
    "debug_one_zero": dict(opts=dict(xres=24, yres=24, **JIT4), params=channels("one", "zero", "sny"), world=HALF, twin=channels("hit", "zero", "sny")),
    # 6. inside an emitting homogeneous medium: Scene::Li's T * Lo + Lv
    "debug_medium_emission": dict(opts=dict(xres=24, yres=24, volume_integrator='"emission" "float stepsize" [40]', **JIT4), params=channels("u", "v", "hit"),
                                  world=dict(volume='"color Le" [.0012 .0009 .0015]'), twin="no volume"),
    # 7. a thin lens, a Gaussian filter wider than a pixel, a crop window, one random sample per pixel, an odd frame
    "debug_lens_gauss_crop": dict(opts=dict(xres=23, yres=17, sampler="random", xsamples=1, ysamples=1, pixel_filter="gaussian",
                                            filter_params='"float xwidth" [1.5] "float ywidth" [1.5]', crop=(.1, .9, .15, .95), lensradius=6.0, focaldistance=1100.0),
                                  params="", world=HALF, twin=channels("v", "u", "zero")),
    # 8. 300 small triangles under an orthographic camera
    "debug_soup_ortho": dict(opts=dict(xres=24, yres=24, **JIT4), params=channels("nx", "ny", "nz"), world=world(obj(soup())), camera=ORTHO,
                             twin=channels("u", "v", "nz")),
}


def scene_text(name, twin=False):
    c = CONFIGS[name]
    params = c["twin"] if twin and c["twin"] != "no volume" else c["params"]
    kw = dict(keyed=True, count=True, integrator="debug", integrator_params=params, **c["opts"])
    if isinstance(c["world"], dict):
        text = scenes.cornell_scene(world_kwargs=c["world"], **kw)
    else:
        text = scenes.options_block(**kw) + c["world"]
    if "camera" in c:
        text, n = re.subn(r'^Camera "perspective"[^\n]*$', c["camera"], text, flags=re.M)
        assert n == 1, n
    if twin and c["twin"] == "no volume":
        text, n = re.subn(r'^Volume "homogeneous"[^\n]*\n', "", text, flags=re.M)
        assert n == 1, n
    return text


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name, c in CONFIGS.items():
        if only and name not in only:
            continue
        text = scene_text(name)
        rgb, alpha, st = REF.run_reference(text, keyed=True)
        trgb, talpha, tst = REF.run_reference(scene_text(name, twin=True), keyed=True)
        share = float((np.sqrt(((rgb - trgb) ** 2).sum(-1)) > 1e-3).mean())
        print(name, rgb.shape, "mean", rgb.reshape(-1, 3).mean(0), "max", float(rgb.max()), "alpha", float(alpha.min()), float(alpha.max()),
              {k: st[k] for k in ("closest_rays", "any_rays")}, "stderr lines", st["stderr_lines"], tst["stderr_lines"], "differs from its twin on %.3f" % share)
        assert np.isfinite(rgb).all() and np.isfinite(alpha).all() and st["stderr_lines"] == 0, name
        assert np.isfinite(trgb).all() and tst["stderr_lines"] == 0, name
        assert share >= MIN_SHARE, "%s: only %.3f of the pixels differ from the twin's film" % (name, share)
        extra = dict(twin_rgb=trgb) if c.get("keep") else {}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st)), twin_share=np.array(share),
                            twin=np.array(c["twin"]), **extra)
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
