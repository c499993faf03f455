"""Generate the shinymetal / translucent fixtures in tests/golden/materials/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref_keyed
with its shinymetal.so / translucent.so plugins and the countaccel wrapper for ray counts), the way tests/golden/make_density_golden.py does
for the density fixtures.  Runs only where the reference sources exist.

    python tests/golden/make_materials_golden.py [name ...]

The fixtures live in a subdirectory: the top-level ones are also fed to the frozen CPU oracle, which does not know these materials.
Each <name>.npz holds the scene text, the reference's float film (rgb, alpha), its ray counts / StatsPrint table and `matte_share`:
the share of the pixels on which the reference's film of the SAME scene with the material's name replaced by "matte" (what the host
front end falls back to for a material it does not know) is more than 1e-3 (per-pixel L2) away.  The generator refuses a fixture
whose share is below 5 %: such a frame would pass on the fall-back.  The two `sheet_*` fixtures also keep that matte film
(matte_rgb, matte_alpha, matte_stats): tests/test_gpu_materials.py holds the device to both.
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

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "materials")
MIN_SHARE = 0.05

POINT = 'LightSource "point" "point from" [278 300 100] "color I" [90000 85000 70000]\n'
SPOT = ('LightSource "spot" "point from" [400 540 120] "point to" [250 0 330] "color I" [500000 450000 380000] '
        '"float coneangle" [30] "float conedeltaangle" [10]\n')
# a sheet across the whole box below the area light, tilted from y = 420 at the front to y = 380 at the back: the camera sees its underside
SHEET = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 420 0 556 420 0 556 380 559 0 380 559]\n'
# a large panel leaning back, its front towards the camera and the ceiling
PANEL = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [60 20 300 500 20 300 500 460 420 60 460 420]\n'
SPHERE = 'Shape "sphere" "float radius" [170]\n'
T_ONLY = '"translucent" "color reflect" [0 0 0] "color transmit" [.8 .8 .8] "float roughness" [.2]'
HOMOG = '"float g" [.2]'


def obj(material, shape, at="0 0 0", pre=""):
    return 'AttributeBegin\n%sTranslate %s\nMaterial %s\n%s\nAttributeEnd\n' % (pre, at, material, shape.rstrip("\n"))


def mesh(radius=170.0, **kw):
    return scenes.smooth_mesh_text(radius=radius, nu=12, nv=8, **kw)


# name -> (options, world kwargs); every world is the Cornell box of scenes.cornell_world
CONFIGS = {
    # shinymetal on a quadric, Whitted, kd-tree, area light (specular recursion through the conductor lobe)
    "shiny_sphere_whitted": (dict(xres=32, yres=32, integrator="whitted"),
                             dict(extra=obj('"shinymetal" "color Ks" [.8 .7 .3] "color Kr" [.6 .6 .7] "float roughness" [.15]', SPHERE, "278 175 300"))),
    # shinymetal on a mesh with per-vertex normals, DirectLighting "all", grid, lowdiscrepancy, spot + area light; Kr black; Ks above .999 (the clamp)
    "shiny_mesh_direct_all_grid_ld": (dict(xres=32, yres=32, integrator="directlighting", sampler="lowdiscrepancy", pixelsamples=2, accelerator="grid"),
                                      dict(extra=SPOT + obj('"shinymetal" "color Ks" [1 .9995 .6] "color Kr" [0 0 0] "float roughness" [.2]', mesh(), "278 175 300",
                                                            pre=""))),
    # shinymetal panel (triangles only), DirectLighting "one", point + area light; Ks black
    "shiny_panel_direct_one": (dict(xres=32, yres=32, integrator="directlighting", integrator_params='"string strategy" ["one"]', xsamples=2, ysamples=1, jitter=True),
                               dict(point_light=True, extra=obj('"shinymetal" "color Ks" [0 0 0] "color Kr" [.9 .8 .5] "float roughness" [.1]', PANEL))),
    # shinymetal mesh, path tracing (specularBounce through the conductor lobe)
    "shiny_mesh_path": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, jitter=True),
                        dict(extra=obj('"shinymetal" "color Ks" [.9 .6 .4] "float roughness" [.12]', mesh(120.0), "278 130 300"))),
    # the sheet between the area light and the floor, T lobes only: Whitted (the underside is lit from the far side) ...
    "sheet_whitted": (dict(xres=32, yres=32, integrator="whitted"), dict(extra=obj(T_ONLY, SHEET))),
    # ... and path tracing, 16 spp (paths continue through the sheet and light the floor)
    "sheet_path": (dict(xres=32, yres=32, integrator="path", xsamples=4, ysamples=4, jitter=True), dict(extra=obj(T_ONLY, SHEET))),
    # the sheet with all four lobes, DirectLighting "weighted", a point light below it and the area light above
    "transl_sheet_direct_weighted": (dict(xres=32, yres=32, integrator="directlighting", integrator_params='"string strategy" ["weighted"]', xsamples=2, ysamples=1,
                                          jitter=True),
                                     dict(extra=POINT + obj('"translucent" "color Kd" [.4 .5 .3] "color Ks" [.3 .3 .3] "color reflect" [.5 .5 .5] "color transmit" [.6 .6 .6] '
                                                            '"float roughness" [.15]', SHEET))),
    # "transmit" black (R lobes only) on the panel, DirectLighting "all" with two light samples, kd-tree
    "transl_panel_transmit_black_direct": (dict(xres=32, yres=32, integrator="directlighting", xsamples=2, ysamples=1, jitter=True),
                                           dict(light_nsamples=2, extra=obj('"translucent" "color Kd" [.3 .4 .6] "color Ks" [.8 .8 .8] "color reflect" [.9 .9 .9] '
                                                                            '"color transmit" [0 0 0] "float roughness" [.1]', PANEL))),
    # Kd black (glossy R and glossy T only) on the sheet, Whitted, grid accelerator, the default roughness
    "transl_sheet_kd_black_whitted_grid": (dict(xres=32, yres=32, integrator="whitted", accelerator="grid"),
                                           dict(extra=obj('"translucent" "color Kd" [0 0 0] "color transmit" [.9 .9 .9]', SHEET))),
    # "reflect" and "transmit" both black: no lobes, the surface is black and ends paths
    "transl_panel_no_lobes_path": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, jitter=True),
                                   dict(extra=obj('"translucent" "color reflect" [0 0 0] "color transmit" [0 0 0]', PANEL))),
    # a closed translucent mesh with per-vertex normals, path tracing, lowdiscrepancy
    "transl_closed_mesh_path_ld": (dict(xres=24, yres=24, integrator="path", sampler="lowdiscrepancy", pixelsamples=4),
                                   dict(extra=obj('"translucent" "color Kd" [.7 .8 .6] "color Ks" [.4 .4 .4] "color reflect" [.3 .3 .3] "color transmit" [.7 .7 .7] '
                                                  '"float roughness" [.2]', mesh(140.0), "278 150 300"))),
    # both materials next to glass and plastic, path tracing
    "mix_glass_plastic_path": (dict(xres=32, yres=32, integrator="path", xsamples=2, ysamples=2, jitter=True),
                               dict(extra=obj('"shinymetal" "color Ks" [.7 .7 .8] "color Kr" [.8 .8 .8] "float roughness" [.1]', 'Shape "sphere" "float radius" [90]', "140 95 300") +
                                    obj('"glass" "float index" [1.5]', 'Shape "sphere" "float radius" [70]', "420 75 200") +
                                    obj('"plastic" "color Kd" [.2 .5 .3] "color Ks" [.5 .5 .5] "float roughness" [.2]', mesh(80.0), "400 300 400") +
                                    obj('"translucent" "color Kd" [.8 .6 .5] "float roughness" [.15]',
                                        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [100 430 100 456 430 100 456 400 459 100 400 459]'))),
    # the T-only sheet in a homogeneous medium, DirectLighting "all", single scattering
    "sheet_medium_direct": (dict(xres=32, yres=32, integrator="directlighting", xsamples=2, ysamples=1, jitter=True, volume_integrator='"single" "float stepsize" [60]'),
                            dict(volume=HOMOG, extra=obj('"translucent" "color reflect" [.2 .2 .2] "color transmit" [.8 .8 .8] "float roughness" [.2]', SHEET))),
}
KEEP_MATTE = ("sheet_whitted", "sheet_path")


def scene_text(name):
    opts, wk = CONFIGS[name]
    return scenes.cornell_scene(keyed=True, count=True, world_kwargs=wk, **opts)


def as_matte(text):
    """The same scene with the new materials' names replaced by "matte": what the host front end falls back to for an unknown material."""
    return re.sub(r'Material "(shinymetal|translucent)"', 'Material "matte"', text)


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name in CONFIGS:
        if only and name not in only:
            continue
        text = scene_text(name)
        rgb, alpha, st = REF.run_reference(text, keyed=True)
        mrgb, malpha, mst = REF.run_reference(as_matte(text), keyed=True)
        share = float((np.sqrt(((rgb - mrgb) ** 2).sum(-1)) > 1e-3).mean())
        print(name, rgb.shape, "mean", float(rgb.mean()), "max", float(rgb.max()), {k: st[k] for k in ("closest_rays", "any_rays")}, "stderr lines", st["stderr_lines"],
              "differs from matte on %.3f" % share)
        assert np.isfinite(rgb).all() and st["stderr_lines"] == 0, name
        assert share >= MIN_SHARE, "%s: only %.3f of the pixels differ from the matte fall-back" % (name, share)
        extra = {}
        if name in KEEP_MATTE:
            extra = dict(matte_rgb=mrgb, matte_alpha=malpha, matte_stats=np.array(json.dumps(mst)))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st)),
                            matte_share=np.array(share), **extra)


if __name__ == "__main__":
    main()
