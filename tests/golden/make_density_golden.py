"""Generate the density-medium fixtures in tests/golden/density/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref_keyed with its
exponential.so / volumegrid.so plugins and the countaccel wrapper for ray counts), the way tests/golden/make_golden.py does for the
top-level fixtures.  Runs only where the reference sources exist.

    python tests/golden/make_density_golden.py [name ...]

The fixtures live in a subdirectory: the top-level ones are also fed to the frozen CPU oracle, which knows only homogeneous media.
Each <name>.npz holds the scene text (grids generated from a seed, written into the text), the reference's float film (rgb, alpha)
and its ray counts / StatsPrint table.  Fixtures are DATA (inputs + expected outputs); no reference source text is stored."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
from pbrt_v1_amd import scenes  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "density")

POINT = 'LightSource "point" "point from" [200 450 150] "color I" [120000 110000 90000]\n'
SPOT = ('LightSource "spot" "point from" [400 540 120] "point to" [250 0 330] "color I" [500000 450000 380000] '
        '"float coneangle" [30] "float conedeltaangle" [10]\n')


def grid_values(nx, ny, nz, seed):
    """Seeded densities in [0, 2) with 4 significant digits (exact in the scene text)."""
    rng = np.random.default_rng(seed)
    return np.round(rng.random(nx * ny * nz) * 2.0, 3).astype(np.float32)


def grid_volume(nx, ny, nz, seed, p0, p1, consts, xform=""):
    vals = " ".join("%.9g" % v for v in grid_values(nx, ny, nz, seed))
    return ('AttributeBegin\n%sVolume "volumegrid" "integer nx" [%d] "integer ny" [%d] "integer nz" [%d] "point p0" [%s] "point p1" [%s] %s '
            '"float density" [%s]\nAttributeEnd\n' % (xform, nx, ny, nz, scenes._fmt(p0), scenes._fmt(p1), consts, vals))


def exp_volume(p0, p1, consts, xform=""):
    return 'AttributeBegin\n%sVolume "exponential" "point p0" [%s] "point p1" [%s] %s\nAttributeEnd\n' % (xform, scenes._fmt(p0), scenes._fmt(p1), consts)


SIG = '"color sigma_a" [.002 .0025 .003] "color sigma_s" [.003 .003 .0025]'
XFORM = "Translate 278 0 280\nRotate 25 0 1 0\nRotate -10 1 0 0\nScale 1.2 .9 1.1\n"

# name -> (options, world kwargs); every world is the Cornell box of scenes.cornell_world
CONFIGS = {
    # exponential fog, single scattering, Whitted, point light (delta), kd-tree
    "dens_exp_single_whitted": (dict(xres=32, yres=32, integrator="whitted", volume_integrator='"single" "float stepsize" [50]'),
                                dict(area_light=False, point_light=True,
                                     extra=exp_volume([0, 0, 0], [556, 549, 559], SIG + ' "float a" [1.5] "float b" [.004] "float g" [.3]'))),
    # exponential with emission only, path tracing, jittered stratified
    "dens_exp_emission_path": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, jitter=True,
                                    volume_integrator='"emission" "float stepsize" [40]'),
                               dict(extra=exp_volume([20, 10, 20], [530, 530, 540], SIG + ' "color Le" [.002 .003 .004] "float b" [.003]'))),
    # a non-cubic grid (its border voxels clamp), single scattering, DirectLighting, grid accelerator, area light
    "dens_grid_single_direct_grid": (dict(xres=32, yres=32, integrator="directlighting", xsamples=2, ysamples=1, jitter=True, accelerator="grid",
                                          volume_integrator='"single" "float stepsize" [45]'),
                                     dict(extra=grid_volume(7, 5, 4, 1, [30, 20, 40], [520, 500, 530], SIG + ' "float g" [-.2]'))),
    # a grid with emission only, Whitted, spot light, lowdiscrepancy sampler
    "dens_grid_emission_whitted_ld": (dict(xres=32, yres=32, integrator="whitted", sampler="lowdiscrepancy", pixelsamples=2,
                                           volume_integrator='"emission" "float stepsize" [35]'),
                                      dict(area_light=False, extra=SPOT + grid_volume(6, 9, 5, 2, [0, 0, 0], [556, 549, 559], SIG + ' "color Le" [.004 .003 .002]'))),
    # DirectLighting "weighted" with delta lights only in exponential fog
    "dens_exp_weighted_delta": (dict(xres=32, yres=32, integrator="directlighting", integrator_params='"string strategy" ["weighted"]', xsamples=2, ysamples=1,
                                     jitter=True, volume_integrator='"single" "float stepsize" [60]'),
                                dict(area_light=False, point_light=True, extra=SPOT + exp_volume([0, 0, 0], [556, 549, 559], SIG + ' "float b" [.002]'))),
    # exponential under a rotated / scaled transform with an up direction off the axes, DirectLighting, lowdiscrepancy, grid accelerator
    "dens_exp_xform_updir_direct_ld": (dict(xres=32, yres=32, integrator="directlighting", sampler="lowdiscrepancy", pixelsamples=2, accelerator="grid",
                                            volume_integrator='"single" "float stepsize" [40]'),
                                       dict(extra=exp_volume([-200, 10, -200], [200, 450, 200], SIG + ' "float a" [2] "float b" [.006] "vector updir" [.3 1 .2] "float g" [.5]',
                                                             xform=XFORM))),
    # a grid under the rotated / scaled transform, path tracing, single scattering
    "dens_grid_xform_path": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, volume_integrator='"single" "float stepsize" [50]'),
                             dict(extra=grid_volume(5, 8, 6, 3, [-200, 10, -200], [200, 450, 200], SIG + ' "color Le" [.001 .001 .001]', xform=XFORM))),
}


def scene_text(name):
    opts, wk = CONFIGS[name]
    return scenes.cornell_scene(keyed=True, count=True, world_kwargs=wk, **opts)


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name in CONFIGS:
        if only and name not in only:
            continue
        text = scene_text(name)
        rgb, alpha, st = REF.run_reference(text, keyed=True)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st)))
        print(name, rgb.shape, "mean", float(rgb.mean()), {k: st[k] for k in ("closest_rays", "any_rays")}, "stderr lines", st["stderr_lines"])


if __name__ == "__main__":
    main()
