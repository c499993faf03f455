"""The two scenes of tests/golden/rays/ (hit geometry of caller-supplied rays: DeviceScene.intersect) and their float64 forms.

  rays_mesh_kd     a latitude / longitude mesh with per-vertex uv, N and S (scenes.smooth_mesh_text, positions squashed so that the shading normals
                   differ from the geometric ones), twice: one copy under ReverseOrientation, one under Scale -1 1 1 (a transform that swaps
                   handedness); the second emits (an area light), so the primitives' material and light indices differ.  Perspective camera, kd-tree.
  rays_mixed_grid  the same two meshes plus a partial sphere, a disk with an inner radius and a partial cylinder, each rotated, the cylinder under a
                   non-uniform scale; Accelerator "grid", orthographic camera with a screen window.

Both are rendered by the reference with the oracle-side "probe" integrator (tests/golden/make_rays_golden.py), which records Intersection::dg per
camera ray.  The forms are analytic_forms.Mesh / Quadric / Scene, built from the very arrays the scene text holds; scene_text() and form() follow
analytic_cases.scene_text / form, with an AreaLightSource line where a surface emits."""
import numpy as np

import analytic_cases as A
import analytic_forms as F

RES = 32                        # 33 x 33 camera rays (the sample extent of a 32 x 32 film under the box filter of width .5)
MESH = dict(radius=1.45, nu=10, nv=6, squash=(1.0, .75, 1.0), with_s=True)


def _mesh():
    return ("mesh", A.mesh_arrays(A.SCENES.smooth_mesh_text(**MESH)))


def _meshes():
    return [dict(shape=_mesh(), ctm=[("Translate", -1.7, .2, 0), ("Rotate", -50, 1, 0, 0), ("Rotate", 40, 0, 0, 1)], reverse=True,
                 material=("matte", dict(Kd=(.5, .5, .5)))),
            dict(shape=_mesh(), ctm=[("Translate", 1.7, -.3, .4), ("Rotate", 35, 0, 1, 0), ("Rotate", -20, 0, 0, 1), ("Scale", -1, 1, 1)], area=(2, 2, 2),
                 material=("matte", dict(Kd=(.2, .6, .3))))]


def _quadrics():
    return [dict(shape=("sphere", dict(radius=1.1, zmin=-.7, zmax=.9, phimax=260)), ctm=[("Translate", 0, 2.6, .5), ("Rotate", 70, 1, 0, 0), ("Rotate", 30, 0, 0, 1)],
                 material=("plastic", dict(Kd=(.3, .3, .6), Ks=(.4, .4, .4), roughness=.1))),
            dict(shape=("disk", dict(height=.2, radius=1.2, innerradius=.4, phimax=300)), ctm=[("Translate", -2.2, -2.6, 0), ("Rotate", 35, 1, 0, 0), ("Rotate", -15, 0, 1, 0)],
                 material=("matte", dict(Kd=(.7, .2, .2)))),
            dict(shape=("cylinder", dict(radius=.8, zmin=-1, zmax=1.2, phimax=290)), ctm=[("Translate", 2.2, -2.5, 0), ("Rotate", 60, 1, 0, 0), ("Rotate", 25, 0, 1, 0), ("Scale", 1, .7, 1)],
                 material=("mirror", dict(Kr=(.9, .9, .9))))]


CASES = {
    "rays_mesh_kd": dict(camera=dict(kind="perspective", fov=50, lookat=(.4, .6, -8, 0, 0, 0, 0, 1, 0), res=(RES, RES)), accel="kdtree", surfaces=_meshes()),
    "rays_mixed_grid": dict(camera=dict(kind="orthographic", lookat=(1, 1.5, -12, 0, 0, 0, 0, 1, 0), screenwindow=(-4.6, 4.6, -4.4, 4.4), res=(RES, RES)), accel="grid",
                            surfaces=_meshes() + _quadrics()),
}


def scene_text(name, probe_dump=None):
    """the scene file: one unjittered sample per pixel under a box filter of width .5, the "probe" integrator (replace it by "whitted" for the product)"""
    c = CASES[name]
    cam = c["camera"]
    xres, yres = cam["res"]
    extra = (' "float fov" [%s]' % A._fmt(cam["fov"])) if cam["kind"] == "perspective" else ""
    if "screenwindow" in cam:
        extra += ' "float screenwindow" [%s]' % A._fmt(cam["screenwindow"])
    out = ["LookAt %s\n" % A._fmt(cam["lookat"]), 'Camera "%s"%s\n' % (cam["kind"], extra),
           'Film "image" "integer xresolution" [%d] "integer yresolution" [%d] "string filename" ["out.exr"]\n' % (xres, yres),
           'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\n',
           'PixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n',
           'SurfaceIntegrator "probe" "string dump" ["%s"] "point target" [0 50 0]\n' % (probe_dump or "probe_rays.bin"),
           'Accelerator "%s"\nWorldBegin\n' % c["accel"]]
    for s in c["surfaces"]:
        kind, sp = s["shape"]
        out.append("AttributeBegin\n" + A._ctm_text(s.get("ctm", [])) + ("ReverseOrientation\n" if s.get("reverse") else ""))
        out.append('Material "%s" %s\n' % (s["material"][0], A._params(s["material"][1])))
        if s.get("area"):
            out.append('AreaLightSource "area" "color L" [%s]\n' % A._fmt(s["area"]))
        out.append(A._mesh_text(sp) if kind == "mesh" else 'Shape "%s" %s\n' % (kind, A._params(sp)))
        out.append("AttributeEnd\n")
    out.append("WorldEnd\n")
    return "".join(out)


def product_text(text):
    """a fixture's scene text as the product parses it: the probe integrator is the reference's plugin, any surface integrator serves"""
    return str(text).replace('SurfaceIntegrator "probe"', 'SurfaceIntegrator "whitted"')


def form(name):
    c = CASES[name]
    surfaces = []
    for s in c["surfaces"]:
        kind, sp = s["shape"]
        m = A._ctm(s.get("ctm", []))
        shape = F.Mesh(sp["P"], sp["indices"], m, uv=sp.get("uv"), N=sp.get("N"), S=sp.get("S")) if kind == "mesh" else F.Quadric(kind, m, **sp)
        surfaces.append((shape, F.Material(s["material"][0], **s["material"][1])))
    return F.Scene(A.camera_form(c["camera"]), surfaces, [])


def evaluate(sc, rec, with_band=True):
    """The float64 form on the rays of 20-float probe records: dict(hit, t, p, n, ns, u, v, idx) -- n the geometric normal, ns the shading normal
    (a quadric's is its geometric one), both up to their sign; band: ray_band of these rays (what a fixture stores) unless with_band is False."""
    o, d = rec[:, 0:3].astype(np.float64), rec[:, 3:6].astype(np.float64)
    mint, maxt = rec[:, 6].astype(np.float64), rec[:, 7].astype(np.float64)
    t, n, idx, root = sc.closest(o, d, mint, maxt)
    u, v, ns, _ = sc.details(o, d, mint, maxt, idx)
    hit = idx >= 0
    p = o + np.where(hit, t, 0.0)[:, None] * d
    return dict(hit=hit, t=t, p=p, n=n, ns=ns, u=u, v=v, idx=idx, band=ray_band(sc, o, d, mint, maxt) if with_band else None)


def ray_band(sc, o, d, mint, maxt, angle=3e-4):
    """analytic_forms.ray_band with the TRIANGLE in the outcome: the geometric normal of a mesh is its triangle's, so a ray within `angle` radians
    of a triangle's edge may read the neighbour's (the surface, the root and, on a mesh with N, the triangle must not change when the direction is
    turned by `angle` in eight directions)"""
    def sig(dd):
        _, _, idx, root = sc.closest(o, dd, mint, maxt)
        return ((idx + 1) * 2 + root) * 100003 + sc.details(o, dd, mint, maxt, idx)[3]
    s0 = sig(d)
    a = F._norm(np.cross(d, np.where(np.abs(d[..., :1]) < .6, [1.0, 0, 0], [0, 1.0, 0])))
    b = np.cross(F._norm(d), a)
    out = np.zeros(s0.shape, bool)
    for ca in (-1, 0, 1):
        for cb in (-1, 0, 1):
            if ca or cb:
                out |= sig(d + angle * np.linalg.norm(d, axis=-1, keepdims=True) * (ca * a + cb * b)) != s0
    return out


def sign_free(a, b):
    """largest component difference of two normals up to the sign of one: ReverseOrientation and a mirroring transform flip signs only"""
    return np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1))


def deviations(f, t, p, n, uv, sel, ns=None):
    """The deviations of measured hit data (float32 arrays over all rays) from the form f = evaluate(...) on the rays `sel`, as
    analytic_cases.measure_probe takes the reference's: t and p relative to t, normals (sign-free) and (u, v) absolute."""
    tt = f["t"][sel]
    out = dict(dev_t=float((np.abs(t[sel] - tt) / tt).max()),
               dev_p=float((np.abs(p[sel] - f["p"][sel]).max(-1) / tt).max()),
               dev_n=float(sign_free(n[sel].astype(np.float64), f["n"][sel]).max()),
               dev_uv=float(max(np.abs(uv[sel, 0] - f["u"][sel]).max(), np.abs(uv[sel, 1] - f["v"][sel]).max())))
    if ns is not None:
        out["dev_ns"] = float(sign_free(ns[sel].astype(np.float64), f["ns"][sel]).max())
    return out


def measure(name, rec):
    """the reference's records against the form: the band, hit agreement outside it and the recorded deviations (what the fixture stores)"""
    f = evaluate(form(name), rec)
    inc = ~f["band"]
    both = inc & f["hit"] & (rec[:, 8] > 0)
    out = deviations(f, rec[:, 9], rec[:, 10:13], rec[:, 13:16], rec[:, 16:18], both)
    kinds = sorted({getattr(form(name).surfaces[i][0], "kind", "mesh") for i in np.unique(f["idx"][both])})
    out.update(band=f["band"], band_share=float(f["band"].mean()), hit_equal=bool(np.array_equal(f["hit"][inc], rec[inc, 8] > 0)), hit_share=float(f["hit"].mean()),
               kinds_hit=kinds, surfaces_hit=sorted(int(i) for i in np.unique(f["idx"][both])))
    return out
