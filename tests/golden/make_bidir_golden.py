"""Generate the bidirectional-integrator fixtures in tests/golden/bidir/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref_keyed with its
bidirectional.so plugin under the keyed sampler, and the countaccel wrapper for ray counts), the way tests/golden/make_infinite_golden.py does for
the infinite light.  Runs only where the reference sources exist.

    python tests/golden/make_bidir_golden.py [name ...]

The fixtures live in a subdirectory: the top-level ones are also fed to the frozen CPU oracle, which does not know this integrator.
Each <name>.npz holds the scene text, the reference's float film (rgb, alpha), its ray counts / StatsPrint table and `path_share`: the share
of the pixels on which the reference's film of the SAME scene with SurfaceIntegrator "path" is more than 1e-3 (per-pixel L2) away.  The generator
refuses a fixture whose share is below 5 % -- such a frame would pass for a path-traced one -- and any fixture with reference stderr lines or
non-finite values.  The frames are 24 x 24 or 32 x 32 at 4 spp: a few thousand camera samples, of which about a fifth reach a fourth vertex.
Fixtures are DATA (inputs + expected outputs); no reference source text is stored."""
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

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bidir")
MIN_SHARE = 0.05
MAX_BYTES = 64 * 1024

SPOT = ('LightSource "spot" "point from" [400 540 120] "point to" [250 0 330] "color I" [500000 450000 380000] '
        '"float coneangle" [30] "float conedeltaangle" [10]\n')
DISTANT = 'LightSource "distant" "point from" [200 600 -300] "point to" [278 0 300] "color L" [2.5 2.4 2.1]\n'
POINT2 = 'LightSource "point" "point from" [120 300 100] "color I" [90000 85000 70000]\n'
FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [756 0 -200 -200 0 -200 -200 0 760 756 0 760]\n'
MIRROR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [60 10 420 300 10 520 300 360 520 60 360 420]\n'
PANEL = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [320 10 330 520 10 430 520 300 430 320 300 330]\n'
SHEET = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [120 40 260 440 40 260 440 330 260 120 330 260]\n'
QLIGHTS = ('AttributeBegin\nAreaLightSource "area" "color L" [12 10 6]\nMaterial "matte" "color Kd" [0 0 0]\nTranslate 150 300 300\nShape "sphere" "float radius" [40]\nAttributeEnd\n'
           'AttributeBegin\nAreaLightSource "area" "color L" [6 9 14]\nMaterial "matte" "color Kd" [.2 .2 .2]\nTranslate 420 400 250\nRotate 70 1 0 0.3\nShape "disk" "float radius" [60]\nAttributeEnd\n')


def obj(material, shape, at="0 0 0"):
    return 'AttributeBegin\nTranslate %s\nMaterial %s\n%s\nAttributeEnd\n' % (at, material, shape.rstrip("\n"))


def open_world(*parts):
    """no box: a floor plus objects under the sky"""
    return "WorldBegin\n" + "".join(parts) + "WorldEnd\n"


def ext_soup(n=300, seed=77):
    """n triangles of the LCG soup, grown so that a 24 x 24 frame sees them, in four materials (the glossy / transmitting lobes of the EXT shading set)"""
    t = scenes.lcg_soup(n, seed).astype(np.float64)
    c = t.mean(axis=1, keepdims=True)
    t = (c + (t - c) * 9.0).astype(np.float32)
    mats = ('"plastic" "color Kd" [.3 .5 .4] "color Ks" [.5 .5 .5] "float roughness" [.15]',
            '"uber" "color Kd" [.4 .3 .5] "color Ks" [.3 .3 .3] "color Kr" [.2 .2 .2] "float roughness" [.2]',
            '"shinymetal" "color Ks" [.8 .7 .3] "color Kr" [.6 .6 .7] "float roughness" [.15]',
            '"translucent" "color Kd" [.4 .5 .3] "color Ks" [.3 .3 .3] "color reflect" [.5 .5 .5] "color transmit" [.6 .6 .6] "float roughness" [.2]')
    return "".join(obj(m, scenes.soup_shape_text(t[k::4])) for k, m in enumerate(mats))


MATTE_FLOOR = obj('"matte" "color Kd" [.6 .6 .55]', FLOOR)
MIRROR_PANEL = obj('"mirror" "color Kr" [.9 .9 .9]', MIRROR)
MATTE_PANEL = obj('"matte" "color Kd" [.3 .5 .7]', PANEL)
TRANS_SHEET = obj('"translucent" "color Kd" [.5 .5 .4] "color Ks" [0 0 0] "color reflect" [.4 .4 .4] "color transmit" [.7 .7 .7]', SHEET)
BLOB = scenes.icosphere((200, 120, 250), 90, 1)
JIT4 = dict(xsamples=2, ysamples=2, jitter=True)

# name -> (options, world text or Cornell world kwargs)
CONFIGS = {
    # 1. the Cornell box with its two-triangle emitter: ShapeSet::Sample's draw between the two paths' Russian-roulette draws
    "bidir_cornell": (dict(xres=24, yres=24, **JIT4), dict()),
    # 2. a point light only, the mirror quad and a glass icosphere: specular vertices, f = 0 connections, shadow rays skipped on black products
    "bidir_point_specular": (dict(xres=24, yres=24, **JIT4), dict(point_light=True, area_light=False, mirror_quad=True, glass_sphere_tris=BLOB)),
    # 3. open world, spot + distant light, grid accelerator, lowdiscrepancy sampler: cone and disk sampling, the world's bounding sphere
    "bidir_spot_distant_grid_ld": (dict(xres=32, yres=32, sampler="lowdiscrepancy", pixelsamples=4, accelerator="grid"),
                                   open_world(SPOT, DISTANT, MATTE_FLOOR, MATTE_PANEL, obj('"matte" "color Kd" [.7 .6 .5]', MIRROR))),
    # 4. the infinite light over a floor and panels: two-point sphere sampling, many light rays that miss (nLight == 0)
    "bidir_infinite": (dict(xres=24, yres=24, **JIT4),
                       open_world('LightSource "infinite" "color L" [.7 .8 .9]\n', MATTE_FLOOR, MATTE_PANEL, obj('"matte" "color Kd" [.7 .6 .5]', MIRROR))),
    # 5. a sphere and a disk as emitters (full sphere, no phimax): Shape::Sample(u1, u2) of the quadrics
    "bidir_quadric_emitters": (dict(xres=24, yres=24, **JIT4), dict(area_light=False, extra=QLIGHTS)),
    # 6. a 300-triangle soup of plastic / uber / shinymetal / translucent under three lights, random sampler: the EXT lobes, connections through a
    #    translucent sheet, the light pick
    "bidir_soup_ext_random": (dict(xres=24, yres=24, sampler="random", xsamples=2, ysamples=2),
                              dict(point_light=True, extra=POINT2 + TRANS_SHEET + ext_soup())),
    # 7. a smooth mesh with per-vertex "N": shading vs geometric normal in G and in UniformSampleOneLight
    "bidir_mesh_n": (dict(xres=24, yres=24, **JIT4),
                     dict(extra=obj('"matte" "color Kd" [.5 .6 .7]', scenes.smooth_mesh_text(radius=170.0, nu=12, nv=8, squash=(1.0, .8, 1.0)), "278 175 300"))),
    # 8. half of the frame is empty: alpha 0 and the early return that draws nothing
    "bidir_half_empty": (dict(xres=24, yres=24, **JIT4),
                         open_world('LightSource "point" "point from" [278 500 100] "color I" [300000 300000 280000]\n',
                                    obj('"matte" "color Kd" [.6 .6 .55]', 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [278 0 0 -200 0 0 -200 0 700 278 0 700]'),
                                    obj('"matte" "color Kd" [.3 .5 .7]', 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [20 0 500 270 0 600 270 400 600 20 400 500]'))),
}


def scene_text(name, integrator="bidirectional"):
    opts, world = CONFIGS[name]
    if isinstance(world, dict):
        return scenes.cornell_scene(keyed=True, count=True, integrator=integrator, world_kwargs=world, **opts)
    return scenes.options_block(keyed=True, count=True, integrator=integrator, **opts) + world


def as_path(text):
    """The same scene under SurfaceIntegrator "path" (its default maxdepth)."""
    out, n = re.subn(r'^SurfaceIntegrator "bidirectional"[^\n]*\n', 'SurfaceIntegrator "path" \n', text, flags=re.M)
    assert n == 1, n
    return out


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name in CONFIGS:
        if only and name not in only:
            continue
        text = scene_text(name)
        rgb, alpha, st = REF.run_reference(text, keyed=True)
        prgb, palpha, pst = REF.run_reference(as_path(text), keyed=True)
        share = float((np.sqrt(((rgb - prgb) ** 2).sum(-1)) > 1e-3).mean())
        print(name, rgb.shape, "mean", float(rgb.mean()), "max", float(rgb.max()), "alpha mean", float(alpha.mean()),
              {k: st[k] for k in ("closest_rays", "any_rays")}, "stderr lines", st["stderr_lines"], "differs from the path film on %.3f" % share)
        assert np.isfinite(rgb).all() and np.isfinite(alpha).all() and st["stderr_lines"] == 0, name
        assert share >= MIN_SHARE, "%s: only %.3f of the pixels differ from the path-traced film" % (name, share)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st)), path_share=np.array(share))
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
