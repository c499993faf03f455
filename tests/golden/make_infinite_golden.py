"""Generate the infinite-area-light fixtures in tests/golden/infinite/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref_keyed with its
infinite.so plugin and the countaccel wrapper for ray counts), the way tests/golden/make_materials_golden.py does for the material fixtures.
Runs only where the reference sources exist.

    python tests/golden/make_infinite_golden.py [name ...]

The fixtures live in a subdirectory: the top-level ones are also fed to the frozen CPU oracle, which does not know this light.
Each <name>.npz holds the scene text, the reference's float film (rgb, alpha), its ray counts / StatsPrint table and `dark_share`: the
share of the pixels on which the reference's film of the SAME scene with the infinite light's line removed (what the host front end
rendered before it knew the light: an error and no light) is more than 1e-3 (per-pixel L2) away (a path-traced scene left without any light
is not run -- the reference's PathIntegrator indexes an empty light list -- its film is black).  The generator refuses a fixture whose
share is below 5 % -- such a frame would pass without the light -- and any fixture with reference stderr lines or non-finite values.
`inf_black` (L = 0) is exempt from the share: its film differs from the scene without the light only through the light's part in
UniformSampleOneLight, which tests/test_gpu_infinite.py asserts on the fixture's `dark_rgb`.
Every scene is built from triangles (no quadrics: the device's libm then only enters through the sampled directions).
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

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "infinite")
MIN_SHARE = 0.05
MAX_BYTES = 64 * 1024


def inf(L="1 1 1", ns=None):
    return 'LightSource "infinite" "color L" [%s]%s\n' % (L, "" if ns is None else ' "integer nsamples" [%d]' % ns)


INF_RE = re.compile(r'^LightSource "infinite".*\n', re.M)
POINT = 'LightSource "point" "point from" [278 300 100] "color I" [90000 85000 70000]\n'
SPOT = ('LightSource "spot" "point from" [400 540 120] "point to" [250 0 330] "color I" [500000 450000 380000] '
        '"float coneangle" [30] "float conedeltaangle" [10]\n')
FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [756 0 -200 -200 0 -200 -200 0 760 756 0 760]\n'
SMALL_FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [400 100 300 150 100 300 150 330 420 400 330 420]\n'   # (leaning back: the orthographic camera looks along +z)
MIRROR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [60 10 420 300 10 520 300 360 520 60 360 420]\n'
PANEL = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [320 10 330 520 10 430 520 300 430 320 300 330]\n'
HOMOG = ('Volume "homogeneous" "point p0" [0 0 0] "point p1" [556 549 559] "color sigma_a" [.002 .002 .002] '
         '"color sigma_s" [.002 .0025 .003] "float g" [.2]\n')
EXPO = ('Volume "exponential" "point p0" [0 0 0] "point p1" [556 549 559] "color sigma_a" [.002 .0025 .003] "color sigma_s" [.003 .003 .0025] '
        '"float a" [1.5] "float b" [.004] "float g" [.3]\n')


def obj(material, shape, at="0 0 0"):
    return 'AttributeBegin\nTranslate %s\nMaterial %s\n%s\nAttributeEnd\n' % (at, material, shape.rstrip("\n"))


def glass_blob(center, radius):
    return obj('"glass" "float index" [1.5]', scenes.soup_shape_text(scenes.icosphere(center, radius, subdiv=1)))


def open_world(*parts):
    """no box: a floor plus objects under the sky"""
    return "WorldBegin\n" + "".join(parts) + "WorldEnd\n"


MATTE_FLOOR = obj('"matte" "color Kd" [.6 .6 .55]', FLOOR)
MIRROR_PANEL = obj('"mirror" "color Kr" [.9 .9 .9]', MIRROR)
MATTE_PANEL = obj('"matte" "color Kd" [.3 .5 .7]', PANEL)


def ortho(text):
    return re.sub(r'Camera "perspective"[^\n]*\n', 'Camera "orthographic" "float screenwindow" [-420 420 -420 420]\n', text)


# name -> (options, world text or Cornell world kwargs, post-processing of the text)
CONFIGS = {
    # the sky alone: escaped camera and specular rays, Sample_L(p, wi, vis) with its two draws, kd-tree
    "inf_only_whitted": (dict(xres=32, yres=32, integrator="whitted"),
                         open_world(inf(".8 .9 1"), MATTE_FLOOR, MIRROR_PANEL, glass_blob((400, 110, 250), 100.0)), None),
    # both halves of EstimateDirect's MIS with four samples of the light, the shading normal of a mesh with "N" in the light's frame; grid, lowdiscrepancy
    "inf_direct_all_ns4_grid_ld": (dict(xres=32, yres=32, integrator="directlighting", sampler="lowdiscrepancy", pixelsamples=2, accelerator="grid"),
                                   open_world(inf(".9 .6 .3", 4), MATTE_FLOOR,
                                              obj('"plastic" "color Kd" [.3 .5 .4] "color Ks" [.5 .5 .5] "float roughness" [.15]',
                                                  scenes.smooth_mesh_text(radius=170.0, nu=12, nv=8, squash=(1.0, .8, 1.0)), "278 175 300")), None),
    # UniformSampleOneLight among an infinite light, the Cornell emitter (two triangles: it draws its triangle) and a point light
    "inf_plus_area_direct_one": (dict(xres=32, yres=32, integrator="directlighting", integrator_params='"string strategy" ["one"]', xsamples=2, ysamples=1, jitter=True),
                                 dict(point_light=True, extra=inf(".5 .6 .8")), None),
    # path tracing, 16 spp, maxdepth 6: Le after a specular bounce, Russian roulette and the unsampled depths behind the light's own draw
    "inf_path": (dict(xres=24, yres=24, integrator="path", maxdepth=6, xsamples=4, ysamples=4, jitter=True),
                 open_world(inf(".7 .8 .9"), MATTE_FLOOR, MIRROR_PANEL, MATTE_PANEL, glass_blob((400, 110, 200), 100.0)), None),
    # orthographic camera, most of the frame is sky: the alpha rule at pathLength == 0
    "inf_path_ortho_open": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, jitter=True),
                            open_world(inf(".4 .5 .9"), obj('"matte" "color Kd" [.7 .6 .5]', SMALL_FLOOR), glass_blob((278, 170, 300), 60.0)), ortho),
    # homogeneous medium, single scattering: Sample_L without a normal, Transmittance along unbounded shadow rays, T and Lv along escaped rays
    "inf_medium_single_direct": (dict(xres=32, yres=32, integrator="directlighting", xsamples=2, ysamples=1, jitter=True,
                                      volume_integrator='"single" "float stepsize" [60]'),
                                 open_world(inf(".9 .9 .8"), MATTE_FLOOR, MIRROR_PANEL, MATTE_PANEL, HOMOG), None),
    # exponential fog: Tau marched along unbounded shadow rays and escaped rays
    "inf_density_whitted": (dict(xres=32, yres=32, integrator="whitted", volume_integrator='"single" "float stepsize" [50]'),
                            open_world(inf(".8 .8 .9"), MATTE_FLOOR, MIRROR_PANEL, MATTE_PANEL, EXPO), None),
    # L = 0 next to a point light: alpha stays 0 on misses, the light still takes its share of "one" sampling and its draw
    "inf_black": (dict(xres=32, yres=32, integrator="directlighting", integrator_params='"string strategy" ["one"]', xsamples=2, ysamples=1, jitter=True),
                  dict(point_light=True, area_light=False, mirror_quad=True, extra=inf("0 0 0")), None),
    # the exact cases: nothing but the sky (no libm anywhere)
    "inf_empty_whitted": (dict(xres=16, yres=16, integrator="whitted", xsamples=2, ysamples=1), open_world(inf(".2 .4 .6")), None),
    "inf_empty_direct": (dict(xres=16, yres=16, integrator="directlighting", xsamples=2, ysamples=1), open_world(inf(".2 .4 .6")), None),
}
EXEMPT = ("inf_black",)


def scene_text(name):
    opts, world, post = CONFIGS[name]
    if isinstance(world, dict):
        text = scenes.cornell_scene(keyed=True, count=True, world_kwargs=world, **opts)
    else:
        text = scenes.options_block(keyed=True, count=True, **opts) + world
    return post(text) if post else text


def without_light(text):
    """The same scene with the infinite light's line removed: what the host front end rendered before it knew the light."""
    out, n = INF_RE.subn("", text)
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
        dark = without_light(text)
        if "LightSource" in dark or 'SurfaceIntegrator "path"' not in dark:
            drgb, dalpha, dst = REF.run_reference(dark, keyed=True)
        else:
            # PathIntegrator calls UniformSampleOneLight whatever the number of lights (path.cpp:99-110), which indexes lights[-1] when there is
            # none: the reference cannot render this scene.  Without a light or an emitter every radiance is zero: the dark film is black.
            drgb, dalpha, dst = np.zeros_like(rgb), np.zeros_like(alpha), {}
        share = float((np.sqrt(((rgb - drgb) ** 2).sum(-1)) > 1e-3).mean())
        print(name, rgb.shape, "mean", float(rgb.mean()), "max", float(rgb.max()), "alpha mean", float(alpha.mean()),
              {k: st[k] for k in ("closest_rays", "any_rays")}, "stderr lines", st["stderr_lines"], "differs from the dark scene on %.3f" % share)
        assert np.isfinite(rgb).all() and np.isfinite(alpha).all() and st["stderr_lines"] == 0, name
        extra = {}
        if name in EXEMPT:
            extra = dict(dark_rgb=drgb, dark_stats=np.array(json.dumps(dst)))
        else:
            assert share >= MIN_SHARE, "%s: only %.3f of the pixels differ from the scene without the light" % (name, share)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st)), dark_share=np.array(share), **extra)
        assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
