"""The five scenes of tests/golden/bsdf/ (BSDF queries at caller-supplied hits: DeviceScene.bsdf), their queries and their float64 forms.

  gallery_flat         eight tilted quads, one material each: matte (sigma 0 and 20), plastic, uber (opacity .6, non-black Kr: T, D, G, R), shinymetal,
                       translucent (all four lobes), mirror, glass (under ReverseOrientation and tilted, so part of it refracts out of the glass: total
                       internal reflection in frame).  kd-tree.
  gallery_smooth_grid  rays_cases' latitude / longitude mesh with per-vertex N, S and uv, positions squashed so that the shading and the geometric normal
                       disagree about the hemisphere of part of the wi; four copies: under ReverseOrientation (plastic), under Scale -1 1 1 and under Scale 1 1 -1
                       (translucent) and plain (plastic).
                       Accelerator "grid".
  gallery_quadrics     a partial sphere (plastic), a partial cylinder under a non-uniform scale (glass) and a disk with an inner radius (shinymetal): the
                       frame comes from the quadric's dpdu.
  gallery_textured     plastic, uber and translucent panels whose Kd, Ks and roughness are checkerboard (aamode none), mix and scale textures: the
                       material is resolved per hit.
  gallery_emitters     two emitting quads (one seen from its back) and two emitting spheres (one under ReverseOrientation: seen from its back), for le.

The reference answers through the plugin tests/golden/bsdf_probe.cpp (tests/golden/make_bsdf_golden.py).  scene_text() and form() follow rays_cases;
queries() makes the seeded records; evaluate() runs the float64 forms of bsdf_forms on a fixture's records and states which queries are left out."""
import numpy as np

import analytic_cases as A
import analytic_forms as F
import bsdf_forms as B
import rays_cases as R

RES = 32                        # 33 x 33 camera rays (the sample extent of a 32 x 32 film under the box filter of width .5), each used twice
REPEAT = 2
OUTPUTS = ("f", "pdf", "s_wi", "s_f", "s_pdf", "le")          # the float outputs; s_type and n_components are compared for equality
CAMERA = dict(kind="perspective", fov=46, lookat=(.3, .4, -8, 0, 0, 0, 0, 1, 0), res=(RES, RES))
UV01 = (0, 0, 1, 0, 1, 1, 0, 1)


def _quad(cx, cy, rx, ry, material, half=1.22, uv=None, **kw):
    """a square of side 2 * half about (cx, cy, 0), turned by rx degrees about x and ry about y"""
    return dict(shape=A.quad_mesh((-half, -half, 0, half, -half, 0, half, half, 0, -half, half, 0), uv=uv),
                ctm=[("Translate", cx, cy, 0), ("Rotate", rx, 1, 0, 0), ("Rotate", ry, 0, 1, 0)], material=material, **kw)


def _flat():
    return [_quad(-2.45, 2.45, 20, 15, ("matte", dict(Kd=(.7, .6, .5)))),
            _quad(0, 2.45, -25, 10, ("matte", dict(Kd=(.6, .7, .5), sigma=20))),
            _quad(2.45, 2.45, 15, -30, ("plastic", dict(Kd=(.3, .3, .6), Ks=(.4, .4, .4), roughness=.1))),
            _quad(-2.45, 0, -10, 35, ("uber", dict(Kd=(.5, .4, .3), Ks=(.4, .4, .3), Kr=(.3, .3, .35), opacity=(.6, .6, .6), roughness=.15))),
            _quad(2.45, 0, 30, 5, ("shinymetal", dict(Ks=(.8, .7, .5), Kr=(.9, .8, .6), roughness=.05))),
            _quad(-2.45, -2.45, -20, -20, ("translucent", dict(Kd=(.6, .5, .4), Ks=(.3, .3, .3), reflect=(.6, .5, .5), transmit=(.4, .5, .6), roughness=.2))),
            _quad(0, -2.45, 25, -10, ("mirror", dict(Kr=(.9, .9, .8)))),
            _quad(2.45, -2.45, -44, 12, ("glass", dict(Kr=(.9, .9, .9), Kt=(.8, .9, .9), index=1.5)), reverse=True)]


def _smooth():
    mesh = lambda: ("mesh", A.mesh_arrays(A.SCENES.smooth_mesh_text(**dict(R.MESH, radius=1.6, nu=7, nv=4))))
    plastic = ("plastic", dict(Kd=(.3, .3, .6), Ks=(.4, .4, .4), roughness=.1))
    translucent = ("translucent", dict(Kd=(.6, .5, .4), Ks=(.3, .3, .3), reflect=(.6, .5, .5), transmit=(.4, .5, .6), roughness=.2))
    return [dict(shape=mesh(), ctm=[("Translate", -1.62, 1.5, 0), ("Rotate", -50, 1, 0, 0), ("Rotate", 40, 0, 0, 1)], reverse=True, material=plastic),
            dict(shape=mesh(), ctm=[("Translate", 1.62, 1.4, .4), ("Rotate", 35, 0, 1, 0), ("Rotate", -20, 0, 0, 1), ("Scale", -1, 1, 1)], material=translucent),
            dict(shape=mesh(), ctm=[("Translate", -1.62, -1.5, .2), ("Rotate", 65, 1, 0, 0), ("Rotate", 10, 0, 1, 0), ("Scale", 1, 1, -1)], material=translucent),
            dict(shape=mesh(), ctm=[("Translate", 1.62, -1.55, 0), ("Rotate", -30, 0, 1, 0), ("Rotate", 70, 1, 0, 0)], material=plastic)]


def _quadrics():
    return [dict(shape=("sphere", dict(radius=1.5, zmin=-1.0, zmax=1.2, phimax=260)), ctm=[("Translate", -1.45, 1.2, .5), ("Rotate", 70, 1, 0, 0), ("Rotate", 30, 0, 0, 1)],
                 material=("plastic", dict(Kd=(.3, .3, .6), Ks=(.4, .4, .4), roughness=.1))),
            dict(shape=("cylinder", dict(radius=1.0, zmin=-1.3, zmax=1.5, phimax=290)), ctm=[("Translate", 1.55, .9, 0), ("Rotate", 60, 1, 0, 0), ("Rotate", 25, 0, 1, 0), ("Scale", 1, .7, 1)],
                 material=("glass", dict(Kr=(.9, .9, .9), Kt=(.8, .9, .9), index=1.5))),
            dict(shape=("disk", dict(height=.2, radius=1.9, innerradius=.5, phimax=300)), ctm=[("Translate", -.1, -1.5, 0), ("Rotate", 35, 1, 0, 0), ("Rotate", -15, 0, 1, 0)],
                 material=("shinymetal", dict(Ks=(.8, .7, .5), Kr=(.9, .8, .6), roughness=.05)))]


def _textured():
    T, tex, NONE = A.T, A.tex, A.NONE
    chk = lambda name, a, b, **kw: T(name, "color", "checkerboard", tex1=a, tex2=b, **NONE, **kw)
    rough = lambda name, **kw: T(name, "float", "checkerboard", tex1=.2, tex2=.05, **NONE, **kw)
    return [dict(_quad(-2.0, 1.3, 20, 25, ("plastic", dict(Kd=tex("p_kd"), Ks=tex("p_ks"), roughness=tex("p_r"))), half=1.9, uv=UV01),
                 textures=[chk("p_kd", (.8, .2, .2), (.2, .3, .8), uscale=5, vscale=4, udelta=.13, vdelta=.29), chk("p_c", (.5, .5, .4), (.2, .3, .3), uscale=3, vscale=3, udelta=.4),
                           T("p_ks", "color", "scale", tex1=tex("p_c"), tex2=(.9, .8, .7)), rough("p_r", uscale=2, vscale=2, udelta=.5, vdelta=-.5)]),
            dict(_quad(2.0, 1.3, -15, -25, ("uber", dict(Kd=tex("u_kd"), Ks=tex("u_ks"), Kr=(.2, .2, .25), opacity=(.7, .7, .7), roughness=tex("u_r"))), half=1.9, uv=UV01),
                 textures=[chk("u_a", (.7, .6, .2), (.2, .6, .3), uscale=4, vscale=3, udelta=.2, vdelta=.1),
                           T("u_kd", "color", "mix", tex1=tex("u_a"), tex2=(.5, .4, .6), amount=.3), chk("u_ks", (.4, .4, .3), (.15, .2, .2), uscale=2, vscale=5, udelta=.3),
                           rough("u_r", uscale=3, vscale=2, udelta=.25, vdelta=.4)]),
            dict(_quad(0, -1.9, 30, 5, ("translucent", dict(Kd=tex("t_kd"), Ks=tex("t_ks"), reflect=(.6, .5, .5), transmit=(.4, .5, .6), roughness=tex("t_r"))), half=1.9, uv=UV01),
                 textures=[chk("t_kd", (.6, .5, .4), (.3, .6, .6), uscale=5, vscale=5, udelta=.1, vdelta=.2), chk("t_c", (.3, .3, .3), (.5, .4, .3), uscale=3, vscale=4, vdelta=.35),
                           T("t_ks", "color", "scale", tex1=tex("t_c"), tex2=(.8, .9, .7)), rough("t_r", uscale=4, vscale=3, udelta=.45, vdelta=.15)])]


def _emitters():
    grey = ("matte", dict(Kd=(.5, .5, .5)))
    ball = lambda: ("sphere", dict(radius=1.5))
    return [_quad(-1.75, 1.7, 20, 25, grey, half=1.65, area=(4, 3, 2)),
            _quad(1.75, 1.7, 160, 15, grey, half=1.65, area=(2, 3, 4)),                      # turned away: the camera sees its back
            dict(shape=ball(), ctm=[("Translate", -1.7, -1.6, 0), ("Rotate", 40, 1, 0, 0)], material=grey, area=(3, 3, 1)),
            dict(shape=ball(), ctm=[("Translate", 1.7, -1.6, 0), ("Rotate", -30, 0, 1, 0)], material=grey, area=(1, 3, 3), reverse=True)]


CASES = {
    "gallery_flat": dict(camera=CAMERA, accel="kdtree", surfaces=_flat(), triangles_only=True),
    "gallery_smooth_grid": dict(camera=dict(CAMERA, lookat=(.2, .1, -7.2, 0, 0, 0, 0, 1, 0)), accel="grid", surfaces=_smooth(), triangles_only=True),
    "gallery_quadrics": dict(camera=dict(CAMERA, lookat=(.2, .2, -6.3, 0, 0, 0, 0, 1, 0)), accel="kdtree", surfaces=_quadrics(), triangles_only=False),
    "gallery_textured": dict(camera=dict(CAMERA, lookat=(.2, .1, -6.6, 0, 0, -.3, 0, 1, 0)), accel="kdtree", surfaces=_textured(), triangles_only=True),
    "gallery_emitters": dict(camera=dict(CAMERA, lookat=(.2, .1, -6.8, 0, 0, 0, 0, 1, 0)), accel="kdtree", surfaces=_emitters(), triangles_only=False),
}
# the twin each output's fixtures must tell from the truth, and the case that shows it (tests/test_bsdf_host.py)
TWINS = {"f": [("fresnel_one", "gallery_flat")],
         "pdf": [("btdf_pdf_at_wi", "gallery_flat"), ("specular_not_counted", "gallery_flat")],
         "s_wi": [("uber_order_dgtr", "gallery_flat")], "s_type": [("uber_order_dgtr", "gallery_flat")],
         "s_f": [("fresnel_one", "gallery_quadrics")], "s_pdf": [("sample_pdf_not_averaged", "gallery_textured"), ("blinn_pdf_without_zero", "gallery_flat")],
         "n_components": [("flags_any_bit", "gallery_smooth_grid")], "le": [("le_both_sides", "gallery_emitters")]}


def scene_text(name, queries="queries.bin", dump="bsdf.bin"):
    """the scene file: the frame (32 x 32, one unjittered sample per pixel) means nothing to the "bsdfprobe" integrator, which answers the query file"""
    c = CASES[name]
    cam = c["camera"]
    out = ["LookAt %s\n" % A._fmt(cam["lookat"]), 'Camera "perspective" "float fov" [%s]\n' % A._fmt(cam["fov"]),
           'Film "image" "integer xresolution" [%d] "integer yresolution" [%d] "string filename" ["out.exr"]\n' % cam["res"],
           'Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\n',
           'PixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n',
           'SurfaceIntegrator "bsdfprobe" "string queries" ["%s"] "string dump" ["%s"]\n' % (queries, dump),
           'Accelerator "%s"\nWorldBegin\n' % c["accel"]]
    for s in c["surfaces"]:
        kind, sp = s["shape"]
        out.append("AttributeBegin\n" + "".join(A._texture_text(t) for t in s.get("textures", [])))
        out.append(A._ctm_text(s.get("ctm", [])) + ("ReverseOrientation\n" if s.get("reverse") else ""))
        out.append('Material "%s" %s\n' % (s["material"][0], A._params(s["material"][1])))
        if s.get("area"):
            out.append('AreaLightSource "area" "color L" [%s]\n' % A._fmt(s["area"]))
        out.append(A._mesh_text(sp) if kind == "mesh" else 'Shape "%s" %s\n' % (kind, A._params(sp)))
        out.append("AttributeEnd\n")
    out.append("WorldEnd\n")
    return "".join(out)


def product_text(text):
    """a fixture's scene text as the product parses it: the probe integrator is the reference's plugin, any surface integrator serves"""
    import re
    return re.sub(r'SurfaceIntegrator "bsdfprobe"[^\n]*', 'SurfaceIntegrator "whitted"', str(text))


def form(name):
    """(analytic_forms.Scene for the hits, per surface (material kind, parameters with Texture objects, emitted L or None), first primitive per surface)"""
    c = CASES[name]
    surfaces, mats, first, n_prims = [], [], [], 0                 # first: (first primitive, primitives) per surface
    for s in c["surfaces"]:
        kind, sp = s["shape"]
        m = A._ctm(s.get("ctm", []))
        shape = F.Mesh(sp["P"], sp["indices"], m, uv=sp.get("uv"), N=sp.get("N"), S=sp.get("S")) if kind == "mesh" else F.Quadric(kind, m, **sp)
        made = A._textures(s.get("textures", []), None)
        kw = {k: (made[v[1]] if isinstance(v, tuple) and len(v) == 2 and v[0] == "tex" else v) for k, v in s["material"][1].items()}
        surfaces.append((shape, F.Material("matte")))
        mats.append((s["material"][0], kw, s.get("area")))
        count = len(sp["indices"]) // 3 if kind == "mesh" else 1
        first.append((n_prims, count))
        n_prims += count
    return F.Scene(A.camera_form(c["camera"]), surfaces, []), mats, first


def queries(name, seed):
    """dict(rays [R, 8], ridx [n], wi [n, 3], u [n, 3], flags [n]), float32 / int32: the camera rays of the 33 x 33 sample extent (float32 roundings of
    the float64 camera, directions renormalised), each used REPEAT times; wi uniform on the sphere; u uniform in [0, 1) -- and, on 36 queries spread
    over the frame, every combination of u1, u2 in {0, .5, 1 - 2^-24} (the concentric map's special point and its edges) and u3 in {0, 1 - 2^-24}
    (the first and the last lobe), twice; flags cycling through bsdf_forms.FLAG_CYCLE."""
    cam = A.camera_form(CASES[name]["camera"])
    iy, ix = np.mgrid[0:RES + 1, 0:RES + 1]
    o, d, mint, maxt = cam.rays(ix.ravel() + .5, iy.ravel() + .5)
    d = F._norm(d).astype(np.float32)
    d = (d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([o.astype(np.float32), d, mint.astype(np.float32)[:, None], maxt.astype(np.float32)[:, None]], 1)
    n = REPEAT * len(rays)
    rng = np.random.default_rng(seed)
    wi = F._norm(rng.standard_normal((n, 3))).astype(np.float32)
    top = np.float32(1) - np.float32(2.0 ** -24)
    u = np.minimum(rng.random((n, 3)).astype(np.float32), top)
    combos = [(a, b, c) for a in (0, .5, top) for b in (0, .5, top) for c in (0, top)] * 2
    for k, cmb in enumerate(combos):
        u[k * (n // len(combos)) + 7] = cmb
    flags = np.array([B.FLAG_CYCLE[i % len(B.FLAG_CYCLE)] for i in range(n)], np.int32)
    return dict(rays=rays, ridx=(np.arange(n) % len(rays)).astype(np.int32), wi=wi, u=u, flags=flags)


def query_records(q):
    """the plugin's input: 16 words per query (tests/golden/bsdf_probe.cpp)"""
    n = len(q["ridx"])
    rec = np.zeros((n, 16), np.float32)
    rec[:, 0:8], rec[:, 8:11], rec[:, 11:14] = q["rays"][q["ridx"]], q["wi"], q["u"]
    rec[:, 14] = q["flags"].view(np.float32)
    return rec


# the plugin's answer record (36 floats)
ANSWER = dict(hit=slice(0, 1), t=slice(1, 2), p=slice(2, 5), ng=slice(5, 8), uv=slice(8, 10), nn=slice(10, 13), dpdu=slice(13, 16), f=slice(16, 19), pdf=slice(19, 20),
              s_wi=slice(20, 23), s_f=slice(23, 26), s_pdf=slice(26, 27), s_type=slice(27, 28), n_components=slice(28, 29), le=slice(29, 32), n_lobes=slice(32, 33))
UV_EDGE = 2e-4                  # a hit this close (in u or v) to where a checkerboard changes its cell is left out: ~200 float32 roundings of a (u, v) in [0, 1]


def answer(ans, key):
    a = ans[:, ANSWER[key]]
    if key in ("s_type", "n_components", "n_lobes"):
        return np.rint(a[:, 0]).astype(np.int64)
    return a[:, 0] if a.shape[1] == 1 else a


def evaluate(name, q, ans, twin=None):
    """The float64 forms on a fixture's queries `q`, at the hits and in the frames the reference had (`ans`, its answer records: float32 inputs taken
    as they are).  -> dict(f, pdf, s_wi, s_f, s_pdf, s_type, n_components, le, prim, hit, excluded).  `excluded` never looks at an answer's BSDF
    values: the ray is in rays_cases.ray_band (the surface, the root or the triangle changes within 3e-4 rad: a quad's edge, a silhouette); wo, wi or
    the direction the form's chosen lobe draws lies within bsdf_forms.HORIZON of the geometric or the shading horizon; u3 * matchingComps is within LOBE_EDGE of an integer
    between two lobes; the refraction is within TIR_EDGE of total internal reflection; a textured hit is within UV_EDGE of a checkerboard's cell edge."""
    sc, mats, first = form(name)
    rays = q["rays"].astype(np.float64)
    o, d, mint, maxt = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    _, _, idx, _ = sc.closest(o, d, mint, maxt)
    tri = np.zeros(len(rays), np.int64)
    for i, (shape, _) in enumerate(sc.surfaces):
        if isinstance(shape, F.Mesh):
            tri = np.where(idx == i, shape.full(o, d, mint, maxt)["tri"], tri)
    band = R.ray_band(sc, o, d, mint, maxt)
    ridx = q["ridx"]
    n = len(ridx)
    surf, excluded = idx[ridx], band[ridx].copy()
    hit = answer(ans, "hit") > 0
    excluded |= hit != (surf >= 0)                  # (outside the band they agree: the generator asserts it)
    wo, wi, u, flags = -d[ridx], q["wi"].astype(np.float64), q["u"].astype(np.float64), q["flags"].astype(np.int64)
    p, uv = answer(ans, "p").astype(np.float64), answer(ans, "uv").astype(np.float64)
    nn, dpdu, ng = (answer(ans, k).astype(np.float64) for k in ("nn", "dpdu", "ng"))
    out = dict(f=np.zeros((n, 3)), pdf=np.zeros(n), s_wi=np.zeros((n, 3)), s_f=np.zeros((n, 3)), s_pdf=np.zeros(n), s_type=np.zeros(n, np.int64),
               n_components=np.zeros(n, np.int64), le=np.zeros((n, 3)))
    for s, (kind, kw, area) in enumerate(mats):
        sel = hit & (surf == s)
        if not sel.any():
            continue
        trace = dict(cells=[], wraps=[])
        vals = B.resolve(kw, p[sel], uv[sel, 0], uv[sel, 1], trace)
        for du in (-UV_EDGE, UV_EDGE):               # a checkerboard's cell under the four shifted (u, v)
            for dv in (-UV_EDGE, UV_EDGE):
                t2 = dict(cells=[], wraps=[])
                B.resolve(kw, p[sel], uv[sel, 0] + du, uv[sel, 1] + dv, t2)
                for a, b in zip(trace["cells"], t2["cells"]):
                    excluded[np.flatnonzero(sel)[a != b]] = True
        bsdf = B.Bsdf(kind, vals, nn[sel], dpdu[sel], ng[sel], twin)
        smp = bsdf.sample(wo[sel], u[sel], flags[sel])
        out["f"][sel], out["pdf"][sel] = bsdf.f(wo[sel], wi[sel], flags[sel]), bsdf.pdf(wo[sel], wi[sel], flags[sel])
        for k in ("s_wi", "s_f", "s_pdf", "s_type"):
            out[k][sel] = smp[k]
        out["n_components"][sel] = bsdf.n_components(flags[sel])
        if area is not None:
            out["le"][sel] = B.le(F.f32(area), ng[sel], wo[sel], twin)
        near = B.horizon(wo[sel], ng[sel], nn[sel]) | B.horizon(wi[sel], ng[sel], nn[sel]) | smp["near"]
        drew = np.abs(smp["drawn"]).max(-1) > 0
        with np.errstate(all="ignore"):
            near |= drew & B.horizon(np.where(drew[:, None], smp["drawn"], 1.0), ng[sel], nn[sel])
        excluded[np.flatnonzero(sel)[near]] = True
    # the reference's primitive: the surfaces in scene order, a mesh's triangles in REVERSE (Primitive::FullyRefine, core/primitive.cpp:40-53, refines
    # the last entry of its to-do list first; Scene::Intersect names no index, so this is the order of its accelerator's primitive list)
    base, count = np.asarray(first)[np.maximum(surf, 0)].T
    out.update(prim=np.where(surf >= 0, base + count - 1 - tri[ridx], -1), hit=hit, excluded=excluded)
    return out


def errors(got, want, included):
    """bsdf_forms.query_error per float output over the included queries -> {output: per-query e}"""
    return {k: B.query_error(got[k], want[k], included, unit_scale=(k == "s_wi")) for k in OUTPUTS}


def ref_err(name, q, ans, twin=None):
    """the reference's largest e against the float64 form, per float output, and the share of queries left out"""
    w = evaluate(name, q, ans, twin)
    inc = ~w["excluded"]
    e = errors({k: answer(ans, k) for k in OUTPUTS}, w, inc)
    return {k: float(e[k][inc].max()) for k in OUTPUTS}, float(w["excluded"].mean()), w
