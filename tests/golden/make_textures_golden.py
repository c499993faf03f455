"""Generate the texture fixtures in tests/golden/textures/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref_keyed with its texture
plugins and the countaccel wrapper for ray counts), the way tests/golden/make_materials_golden.py does for the material fixtures.  Runs only
where the reference sources exist.

    python tests/golden/make_textures_golden.py [name ...]

Each <name>.npz holds the scene text, the reference's float film (rgb, alpha), its ray counts / StatsPrint table and `flat_share`: the share
of the pixels on which the reference's film of the SAME scene with the Texture statements removed and the textured parameters back at their
literals or defaults is more than 1e-3 (per-pixel L2) away.  The generator refuses a fixture whose share is below 5 %: such a frame would pass
without any texture.  It also refuses a fixture in which a mapped coordinate (uv or planar mapping) is constant at an integer over a triangle
of a textured material -- a planar checker whose edge lies in a wall's plane, say: Floor2Int would decide on rounding noise there, and the
reference would not agree with itself under another libm.
Fixtures are DATA (inputs + expected outputs); no reference source text is stored."""
import ctypes as C
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

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "textures")
MIN_SHARE = 0.05

POINT = 'LightSource "point" "point from" [278 300 100] "color I" [90000 85000 70000]\n'
SHEET = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 420 0 556 420 0 556 380 559 0 380 559]\n'
PANEL = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [60 20 300 500 20 300 500 460 420 60 460 420]\n'
PANEL_UV = PANEL.rstrip("\n") + ' "float uv" [0 0 1 0 1 1 0 1]\n'
HOMOG = '"float g" [.2]'
NONE = '"string aamode" ["none"]'


def checker(name, typ, a, b, more=""):
    lit = (lambda v: '[%s]' % v)
    kind = "color" if typ == "color" else "float"
    return 'Texture "%s" "%s" "checkerboard" "%s tex1" %s "%s tex2" %s %s %s\n' % (name, typ, kind, lit(a), kind, lit(b), NONE, more)


def obj(body, at="0 0 0", pre=""):
    return 'AttributeBegin\n%sTranslate %s\n%s\nAttributeEnd\n' % (pre, at, body.rstrip("\n"))


def mesh(radius=170.0, **kw):
    return scenes.smooth_mesh_text(radius=radius, nu=12, nv=8, **kw)


UVSCALE = '"float uscale" [5] "float vscale" [4] "float udelta" [.13] "float vdelta" [.29]'
PLANAR = '"string mapping" ["planar"] "vector v1" [.004 .006 .003] "vector v2" [-.003 .002 .007] "float udelta" [.37] "float vdelta" [.21]'

# name -> (options, world kwargs, textured walls?); every world is the Cornell box of scenes.cornell_world
CONFIGS = {
    # checker, uv mapping with scale and delta, on a mesh with "uv" (no N: flat triangles).  Whitted, kd-tree
    "chk_uv_mesh_whitted": (dict(xres=32, yres=32, integrator="whitted"),
                            dict(extra=POINT + obj(checker("chk", "color", ".8 .2 .2", ".2 .3 .8", '"float uscale" [8] "float vscale" [6] "float udelta" [.13] "float vdelta" [.29]') +
                                           'Material "matte" "texture Kd" "chk"\n' + mesh(with_n=False), "278 175 300")), False),
    # checker on plain triangles with the default uvs.  DirectLighting "all", grid, lowdiscrepancy
    "chk_default_uv_direct_all_grid_ld": (dict(xres=32, yres=32, integrator="directlighting", sampler="lowdiscrepancy", pixelsamples=2, accelerator="grid"),
                                          dict(extra=obj(checker("chk", "color", ".7 .7 .2", ".1 .4 .5", UVSCALE) + 'Material "matte" "texture Kd" "chk"\n' + PANEL)), False),
    # planar checker on the box walls.  DirectLighting "one", point light plus area light
    "planar_walls_direct_one": (dict(xres=32, yres=32, integrator="directlighting", integrator_params='"string strategy" ["one"]', xsamples=2, ysamples=1, jitter=True),
                                dict(point_light=True, extra=checker("wallchk", "color", ".73 .73 .73", ".2 .25 .6", PLANAR)), True),
    # spherical mapping on a sphere under a rotated and translated CTM (s and t stay inside one check: a bilerp shows them).  Path
    "spherical_sphere_path": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, jitter=True),
                              dict(extra=POINT + obj('Rotate 35 1 1 0\nTexture "sph" "color" "bilerp" "string mapping" ["spherical"] "color v00" [.9 .1 .1] "color v01" [.1 .8 .1] '
                                             '"color v10" [.1 .1 .9] "color v11" [.9 .9 .1]\nMaterial "matte" "texture Kd" "sph"\nShape "sphere" "float radius" [150]', "278 175 300")), False),
    # cylindrical mapping on a cylinder: t = the direction's z, two checks.  Whitted
    "cylindrical_cylinder_whitted": (dict(xres=32, yres=32, integrator="whitted"),
                                     dict(extra=POINT + obj('Rotate -70 1 0 0\n' + checker("cyl", "color", ".8 .6 .1", ".1 .5 .7", '"string mapping" ["cylindrical"]') +
                                                    'Material "matte" "texture Kd" "cyl"\nShape "cylinder" "float radius" [110] "float zmin" [-140] "float zmax" [140]', "278 200 300")), False),
    # bilerp colour and the uv texture as Kd on two smooth meshes.  Path
    "bilerp_uv_two_meshes_path": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, jitter=True),
                                  dict(extra=POINT + obj('Texture "bl" "color" "bilerp" "color v00" [.9 .2 .1] "color v01" [.1 .7 .2] "color v10" [.2 .2 .9] "color v11" [.8 .8 .1]\n'
                                                 'Material "matte" "texture Kd" "bl"\n' + mesh(130.0), "160 140 300") +
                                        obj('Texture "uvt" "color" "uv" "float uscale" [3] "float vscale" [2]\nMaterial "matte" "texture Kd" "uvt"\n' + mesh(130.0), "400 300 330")), False),
    # a nested graph: mix of a checker and a scale, amount a float bilerp; plastic Kd and Ks from it, and a textured float roughness.  DirectLighting
    "nested_mix_plastic_direct": (dict(xres=32, yres=32, integrator="directlighting", xsamples=2, ysamples=1, jitter=True),
                                  dict(extra=POINT + obj(checker("chk", "color", ".8 .3 .2", ".2 .6 .3", UVSCALE) +
                                                         checker("chk2", "color", "1 1 1", ".3 .3 .3", '"float uscale" [3] "float vscale" [7]') +
                                                         'Texture "sc" "color" "scale" "texture tex1" "chk2" "color tex2" [.5 .6 .9]\n'
                                                         'Texture "amt" "float" "bilerp" "float v00" [.1] "float v01" [.9] "float v10" [.7] "float v11" [.3]\n'
                                                         'Texture "mx" "color" "mix" "texture tex1" "chk" "texture tex2" "sc" "texture amount" "amt"\n'
                                                         'Texture "rough" "float" "bilerp" "float v00" [.05] "float v01" [.3] "float v10" [.1] "float v11" [.2]\n'
                                                         'Material "plastic" "texture Kd" "mx" "texture Ks" "mx" "texture roughness" "rough"\n' + PANEL)), False),
    # glass with checkered Kt and a checkered float index.  Whitted
    "glass_checker_whitted": (dict(xres=32, yres=32, integrator="whitted"),
                              dict(extra=POINT + obj(checker("kt", "color", ".9 .9 .9", ".9 .2 .1", '"float uscale" [6] "float vscale" [4]') +
                                             checker("ix", "float", "1.5", "1.1", '"float uscale" [3] "float vscale" [2] "float udelta" [.2]') +
                                             'Material "glass" "texture Kt" "kt" "texture index" "ix"\n' + mesh(190.0, with_n=False), "278 200 250")), False),
    # uber with checkered opacity, 1 on some checks: the transmission lobe comes and goes.  Path
    "uber_opacity_path": (dict(xres=24, yres=24, integrator="path", xsamples=2, ysamples=2, jitter=True),
                          dict(extra=obj(checker("op", "color", "1 1 1", ".3 .3 .3", UVSCALE) +
                                         'Material "uber" "color Kd" [.6 .5 .3] "color Ks" [.3 .3 .3] "color Kr" [.1 .1 .1] "texture opacity" "op" "float roughness" [.2]\n' + PANEL)), False),
    # translucent with reflect / transmit checkered to black: lobes drop per hit.  DirectLighting
    "translucent_lobes_direct": (dict(xres=32, yres=32, integrator="directlighting", xsamples=2, ysamples=1, jitter=True),
                                 dict(extra=POINT + obj(checker("rf", "color", ".6 .6 .6", "0 0 0", UVSCALE) + checker("tr", "color", "0 0 0", ".7 .7 .7", '"float uscale" [3] "float vscale" [3]') +
                                                        'Material "translucent" "color Kd" [.5 .6 .4] "color Ks" [.3 .3 .3] "texture reflect" "rf" "texture transmit" "tr" "float roughness" [.15]\n' + SHEET)), False),
    # matte with a textured sigma: Lambertian on some checks, Oren-Nayar on the others
    "matte_sigma_whitted": (dict(xres=32, yres=32, integrator="whitted"),
                            dict(point_light=True, extra=obj(checker("sg", "float", "0", "60", UVSCALE) + 'Material "matte" "color Kd" [.7 .6 .5] "texture sigma" "sg"\n' + PANEL)), False),
    # shinymetal with textured Ks inside a homogeneous medium with single scattering
    "shiny_medium_direct": (dict(xres=32, yres=32, integrator="directlighting", xsamples=2, ysamples=1, jitter=True, volume_integrator='"single" "float stepsize" [60]'),
                            dict(volume=HOMOG, extra=POINT + obj(checker("ks", "color", ".9 .7 .3", ".2 .2 .8", UVSCALE) +
                                                                 'Material "shinymetal" "texture Ks" "ks" "color Kr" [.3 .3 .3] "float roughness" [.2]\n' + PANEL)), False),
    # checkered Kd and a textured plastic next to it under DirectLighting "weighted" (count, survey and frame passes all resolve): a point light and the area light
    "chk_panel_direct_weighted": (dict(xres=32, yres=32, integrator="directlighting", integrator_params='"string strategy" ["weighted"]', xsamples=2, ysamples=1, jitter=True),
                                  dict(extra=POINT + obj(checker("chk", "color", ".8 .7 .2", ".2 .3 .7", UVSCALE) + 'Material "matte" "texture Kd" "chk"\n' + PANEL) +
                                       obj(checker("ks", "color", ".6 .6 .6", ".1 .1 .1", '"float uscale" [3] "float vscale" [3]') +
                                           'Material "plastic" "color Kd" [.3 .5 .3] "texture Ks" "ks" "float roughness" [.2]\n' + SHEET)), False),
    # a textured Kd under the bidirectional integrator
    "kd_bidirectional": (dict(xres=24, yres=24, integrator="bidirectional", xsamples=2, ysamples=2, jitter=True),
                         dict(extra=obj(checker("chk", "color", ".8 .7 .2", ".2 .3 .7", UVSCALE) + 'Material "matte" "texture Kd" "chk"\n' + PANEL_UV)), False),
    # a textured surface that is itself an area-light emitter
    "emitter_textured_whitted": (dict(xres=32, yres=32, integrator="whitted"),
                                 dict(point_light=True, extra=obj('AreaLightSource "area" "color L" [.6 .5 .4]\n' + checker("chk", "color", ".9 .8 .7", ".1 .3 .6", UVSCALE) +
                                                                  'Material "matte" "texture Kd" "chk"\n' + PANEL)), False),
}
WALL_KD = re.compile(r'"color Kd" \[0\.73 0\.73 0\.73\]')


def scene_text(name):
    opts, wk, walls = CONFIGS[name]
    text = scenes.cornell_scene(keyed=True, count=True, world_kwargs=wk, **opts)
    if walls:
        text, n = WALL_KD.subn('"texture Kd" "wallchk"', text)
        assert n == 3, n
    return text


def flat(text):
    """The same scene without its textures: the Texture statements removed, the textured parameters back at their literals or defaults."""
    text = re.sub(r'^Texture [^\n]*\n', '', text, flags=re.M)
    text = re.sub(r'\s*"texture \w+" "\w+"', '', text)
    assert "Texture" not in text and '"texture' not in text
    return text


def check_no_integer_plane(name, text):
    """Refuse a mapped coordinate that is constant at an integer over a triangle of a textured material (uv and planar mappings)."""
    ps = pkg.ParsedScene(text=text)
    assert ps.errors == 0, name
    H = pkg.host_lib()
    H.pbrt_host_tri_material.restype = C.POINTER(C.c_uint16)
    H.pbrt_host_tri_material.argtypes = [C.c_void_p]
    tm = np.ctypeslib.as_array(H.pbrt_host_tri_material(ps.scene_desc), shape=(ps.n_tris,)).copy()
    verts = ps.tri_verts().astype(np.float64)
    tex = ps.textures()
    mats = ps.materials()
    sh_idx, recs, _ = pkg.shading_records(ps)

    def nodes_of(i, acc):
        acc.add(i)
        for k in ("tex1", "tex2", "amount"):
            if k in tex[i]:
                nodes_of(tex[i][k], acc)
        return acc
    for mi, m in enumerate(mats):
        for root in m.get("textured", {}).values():
            for ni in nodes_of(root, set()):
                t = tex[ni]
                if t.get("mapping") == "planar":
                    for tri in verts[tm == mi]:
                        for vec, d in ((t["v1"], t["udelta"]), (t["v2"], t["vdelta"])):
                            c = d + tri @ np.asarray(vec, np.float64)
                            assert not (np.ptp(c) < 1e-6 and abs(c[0] - round(c[0])) < 1e-4), "%s: a planar coordinate is constant at an integer on a surface" % name
                elif t.get("mapping") == "uv":          # s = uscale * u + udelta, t = vscale * v + vdelta over the triangle's uvs (GetUVs' defaults without "uv")
                    for k in np.nonzero(tm == mi)[0]:
                        uv = recs["uv"][sh_idx[k]].reshape(3, 2).astype(np.float64) if sh_idx is not None and sh_idx[k] >= 0 else np.array([[0, 0], [1, 0], [1, 1]], np.float64)
                        for c in (t["uscale"] * uv[:, 0] + t["udelta"], t["vscale"] * uv[:, 1] + t["vdelta"]):
                            assert not (np.ptp(c) < 1e-6 and abs(c[0] - round(c[0])) < 1e-4), "%s: a uv-mapped coordinate is constant at an integer on a surface" % name
    ps.close()


def main():
    REF = g.load_ref_runner()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name in CONFIGS:
        if only and name not in only:
            continue
        text = scene_text(name)
        check_no_integer_plane(name, text)
        rgb, alpha, st = REF.run_reference(text, keyed=True)
        frgb, falpha, fst = REF.run_reference(flat(text), keyed=True)
        share = float((np.sqrt(((rgb - frgb) ** 2).sum(-1)) > 1e-3).mean())
        print(name, rgb.shape, "mean", float(rgb.mean()), "max", float(rgb.max()), {k: st[k] for k in ("closest_rays", "any_rays")}, "stderr lines", st["stderr_lines"],
              "differs from the flat scene on %.3f" % share)
        assert np.isfinite(rgb).all() and st["stderr_lines"] == 0, name
        assert share >= MIN_SHARE, "%s: only %.3f of the pixels differ from the scene without textures" % (name, share)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st)), flat_share=np.array(share))
        assert os.path.getsize(path) < 64 * 1024, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
