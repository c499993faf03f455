"""The four scenes of tests/golden/lights/ (light queries at caller-supplied points: DeviceScene.light), their queries and their float64 forms.

  delta             a spot light under a rotating and translating CTM, a distant light under a CTM and a point light, listed in that order (the index
                    is not the type); the spot's queries lie in all three falloff zones.
  emitters_tri      four emitters: one triangle in the plane z = 0 under ReverseOrientation (some query points lie in that plane: pdf = 0), a
                    two-triangle quad under a handedness-swapping transform, a five-triangle fan of unequal areas (the cdf loop and its fall-through to the
                    last triangle) and a folded two-triangle "tent" that a Pdf ray crosses twice (the last hit wins).
  emitters_quadric  a sphere (points outside: the cone branch; inside: the area branch), a disk under ReverseOrientation and a cylinder.
  infinite          a point light, the infinite light and a two-triangle emitter: queried with a normal (cosine sample, z flip from the draw) and without.

Query i asks light i % n_lights: a wavefront holds every type.  Queries alternate between the form with a normal and the form without.  The reference
answers through the plugin tests/golden/light_probe.cpp (tests/golden/make_light_golden.py).  evaluate() runs the float64 forms of light_forms on a
fixture's records and states which queries are left out."""
import numpy as np

import analytic_cases as A
import analytic_forms as F
import bsdf_forms as B
import light_forms as LF

N_QUERIES = 1536
SEED = 5                        # the frame's seed ("integer seed" of the keyed sampler): the keyed stream depends on it
OUTPUTS = ("s_wi", "s_L", "s_pdf", "s_ray_o", "s_ray_d", "pdf", "le")          # the float outputs; mint, maxt, s_draws and is_delta are compared for equality
COLUMNS = {"s_wi": slice(0, 3), "s_L": slice(3, 6), "s_pdf": 6, "s_ray_o": slice(7, 10), "s_ray_d": slice(10, 13), "mint": 13, "maxt": 14, "s_draws": 15,
           "pdf": 16, "le": slice(17, 20), "is_delta": 20}
TOP = np.float32(1) - np.float32(2.0 ** -24)

QUAD = dict(P=(-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0), indices=(0, 1, 2, 0, 2, 3))
_FAN_ANGLES, _FAN_RADII = (0, 40, 100, 130, 210, 300), (1.0, .8, 1.2, .6, 1.0, .9)
FAN = dict(P=(0, 0, 0) + tuple(float(np.float32(v)) for a, r in zip(_FAN_ANGLES, _FAN_RADII) for v in (r * np.cos(np.radians(a)), r * np.sin(np.radians(a)), 0)),
           indices=tuple(v for k in range(5) for v in (0, k + 1, k + 2)))
TENT = dict(P=(-1, 1, 0, 1, 1, 0, 0, 0, -.8, 0, 0, .8), indices=(0, 1, 2, 1, 0, 3))

CASES = {
    "delta": [dict(kind="spot", ctm=[("Translate", 1, 2, -1), ("Rotate", 35, 0, 1, 0), ("Rotate", -20, 1, 0, 0)], frm=(.2, .1, 0), to=(.5, -1, .4), coneangle=32, conedelta=9,
                   color=(30, 25, 20)),
              dict(kind="distant", ctm=[("Rotate", 40, 0, 0, 1), ("Rotate", 15, 1, 0, 0)], frm=(1, 3, -1), to=(0, 0, 0), color=(3, 2.5, 2)),
              dict(kind="point", ctm=[("Translate", -1, .5, 2)], frm=(.5, 1, 0), color=(20, 30, 40))],
    "emitters_tri": [dict(kind="tri", ctm=[], reverse=True, P=(-1, -1, 0, 1.5, -.5, 0, 0, 1.2, 0), indices=(0, 1, 2), color=(4, 3, 2)),
                     dict(kind="tri", ctm=[("Translate", 3, 0, 1), ("Rotate", 30, 0, 1, 0), ("Scale", -1, 1, 1)], color=(2, 3, 4), **QUAD),
                     dict(kind="tri", ctm=[("Translate", -3, .5, .5), ("Rotate", -50, 1, 0, 0), ("Rotate", 20, 0, 0, 1)], color=(3, 3, 1), **FAN),
                     dict(kind="tri", ctm=[("Translate", 0, -3, 0)], color=(1, 3, 3), **TENT)],
    "emitters_quadric": [dict(kind="sphere", ctm=[("Translate", -2.5, 0, 0), ("Rotate", 30, 1, 0, 0)], params=dict(radius=1.0), color=(4, 3, 2)),
                         dict(kind="disk", ctm=[("Translate", 0, 1, 0), ("Rotate", 70, 1, 0, 0), ("Rotate", 20, 0, 1, 0)], reverse=True, params=dict(radius=1.2, height=.3),
                              color=(2, 3, 4)),
                         dict(kind="cylinder", ctm=[("Translate", 2.5, 0, .5), ("Rotate", -40, 0, 1, 0)], params=dict(radius=.7, zmin=-.8, zmax=1.0), color=(3, 3, 1))],
    "infinite": [dict(kind="point", ctm=[], frm=(0, 3, 0), color=(20, 30, 40)),
                 dict(kind="infinite", color=(.8, .9, 1.1)),
                 dict(kind="tri", ctm=[("Translate", 2, 0, 1), ("Rotate", 25, 1, 0, 0)], color=(2, 3, 4), **QUAD)],
}
GEN_SEEDS = {"delta": 21, "emitters_tri": 22, "emitters_quadric": 23, "infinite": 24}


# ---------------------------------------------------------------------------------------------- the scene file
def scene_text(name, queries="queries.bin", dump="light.bin"):
    """the scene file: the frame (4 x 4, one unjittered sample per pixel) means nothing to the "lightprobe" integrator, which answers the query file"""
    out = ['LookAt 0 0 -9 0 0 0 0 1 0\nCamera "perspective" "float fov" [40]\n',
           'Film "image" "integer xresolution" [4] "integer yresolution" [4] "string filename" ["out.exr"]\n',
           'Sampler "keyed" "string inner" ["stratified"] "integer seed" [%d] "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\n' % SEED,
           'PixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n',
           'SurfaceIntegrator "lightprobe" "string queries" ["%s"] "string dump" ["%s"]\n' % (queries, dump), "WorldBegin\n"]
    for l in CASES[name]:
        k = l["kind"]
        out.append("AttributeBegin\n" + A._ctm_text(l.get("ctm", [])) + ("ReverseOrientation\n" if l.get("reverse") else ""))
        if k == "point":
            out.append('LightSource "point" "point from" [%s] "color I" [%s]\n' % (A._fmt(l["frm"]), A._fmt(l["color"])))
        elif k == "spot":
            out.append('LightSource "spot" "point from" [%s] "point to" [%s] "float coneangle" [%s] "float conedeltaangle" [%s] "color I" [%s]\n'
                       % (A._fmt(l["frm"]), A._fmt(l["to"]), A._fmt(l["coneangle"]), A._fmt(l["conedelta"]), A._fmt(l["color"])))
        elif k == "distant":
            out.append('LightSource "distant" "point from" [%s] "point to" [%s] "color L" [%s]\n' % (A._fmt(l["frm"]), A._fmt(l["to"]), A._fmt(l["color"])))
        elif k == "infinite":
            out.append('LightSource "infinite" "color L" [%s] "integer nsamples" [1]\n' % A._fmt(l["color"]))
        else:
            out.append('Material "matte" "color Kd" [.5 .5 .5]\nAreaLightSource "area" "color L" [%s]\n' % A._fmt(l["color"]))
            if k == "tri":
                out.append(A._mesh_text(dict(indices=l["indices"], P=l["P"])))
            else:
                out.append('Shape "%s" %s\n' % (k, " ".join('"float %s" [%s]' % (a, A._fmt(b)) for a, b in l["params"].items())))
        out.append("AttributeEnd\n")
    # a floor far below everything: the accelerator is never empty
    out.append('AttributeBegin\nMaterial "matte" "color Kd" [.5 .5 .5]\n' + A._mesh_text(dict(indices=(0, 1, 2, 0, 2, 3), P=(-9, -9, -9, 9, -9, -9, 9, -9, 9, -9, -9, 9))) + "AttributeEnd\nWorldEnd\n")
    return "".join(out)


def product_text(text):
    """a fixture's scene text as the product parses it: the probe integrator is the reference's plugin, any surface integrator serves"""
    import re
    return re.sub(r'SurfaceIntegrator "lightprobe"[^\n]*', 'SurfaceIntegrator "directlighting"', str(text))


def world_tris(l):
    P = F.xpoint(A._ctm(l.get("ctm", [])), F.f32(l["P"]).reshape(-1, 3))
    return P[np.asarray(l["indices"], np.int64).reshape(-1, 3)]


def forms(name):
    """the float64 form of every light of the case, in scene order"""
    out = []
    for l in CASES[name]:
        k, m = l["kind"], A._ctm(l.get("ctm", []))
        if k in ("point", "spot", "distant"):
            out.append(LF.Delta(F.Light(k, l["color"], l2w=m, frm=l["frm"], to=l.get("to", (0, 0, 1)), coneangle=l.get("coneangle", 30.0), conedelta=l.get("conedelta", 5.0))))
        elif k == "infinite":
            out.append(LF.Infinite(l["color"]))
        elif k == "tri":
            out.append(LF.TriEmitter(world_tris(l), l.get("reverse", False), l["color"]))
        else:
            out.append(LF.QuadricEmitter(k, m, l.get("reverse", False), l["color"], **l["params"]))
    return out


# ---------------------------------------------------------------------------------------------- the queries
def _unit(rs, n):
    v = rs.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def queries(name, seed=None):
    """the seeded query records of a case: p, n [N, 3], light, with_normal [N] int32, u [N, 2], rng [N, 2] uint32 (key, counter), wi [N, 3]"""
    rs = np.random.RandomState(GEN_SEEDS[name] if seed is None else seed)
    lights, N = CASES[name], N_QUERIES
    nl = len(lights)
    li = (np.arange(N) % nl).astype(np.int32)
    wn = ((np.arange(N) // nl) % 2).astype(np.int32)
    p, wi = np.zeros((N, 3)), _unit(rs, N)
    for l, d in enumerate(lights):
        sel = np.nonzero(li == l)[0]
        k, m, n = d["kind"], A._ctm(d.get("ctm", [])), len(sel)
        if k == "spot":
            # points in a cone about the spot's axis, out to one and a half cone angles: all three falloff zones
            pos, axis = F.xpoint(m, F.f32(d["frm"])), F.xvec(m, F.f32(d["to"]) - F.f32(d["frm"]))
            axis = axis / np.linalg.norm(axis)
            side = np.cross(axis, [0.3, 1.0, 0.2]); side /= np.linalg.norm(side)
            up = np.cross(axis, side)
            th, ph, dist = np.radians(rs.uniform(0, 1.5 * d["coneangle"], n)), rs.uniform(0, 2 * np.pi, n), rs.uniform(.5, 6, n)
            dr = np.cos(th)[:, None] * axis + np.sin(th)[:, None] * (np.cos(ph)[:, None] * side + np.sin(ph)[:, None] * up)
            p[sel] = pos + dist[:, None] * dr
        elif k in ("point", "distant", "infinite"):
            p[sel] = rs.uniform(-4, 4, (n, 3))
        elif k == "tri":
            T = world_tris(d)
            c = T.reshape(-1, 3).mean(0)
            p[sel] = c + rs.uniform(-3, 3, (n, 3))
            if not d.get("ctm") and len(T) == 1:               # the emitter in the plane z = 0: some points in that plane, outside the triangle
                flat = sel[-(n // 10):]
                p[flat, 2] = 0.0
                p[flat, 0] = np.where(rs.uniform(size=len(flat)) < .5, -1, 1) * rs.uniform(2, 4, len(flat))
            # Pdf directions: three in five aim at a point of a triangle stretched by 1.4 about its centroid (hits, near misses), the rest anywhere
            tk = T[rs.randint(0, len(T), n)]
            b = rs.dirichlet((1, 1, 1), n)
            tgt = (b[:, :, None] * tk).sum(1)
            tgt = tk.mean(1) + 1.4 * (tgt - tk.mean(1))
            aim = rs.uniform(size=n) < .6
            wi[sel] = np.where(aim[:, None], F._norm(tgt - p[sel]), wi[sel])
        else:
            q = LF.QuadricEmitter(k, m, False, d["color"], **d["params"])
            c = F.xpoint(m, np.zeros(3))
            p[sel] = c + _unit(rs, n) * rs.uniform(1.6, 5, n)[:, None]
            if k == "sphere":                                   # three in ten inside the sphere: the area branch
                inside = sel[:3 * n // 10]
                p[inside] = c + _unit(rs, len(inside)) * (q.shape.radius * rs.uniform(0, .9, len(inside)) ** (1 / 3))[:, None]
            tgt, _ = q._uniform(rs.uniform(size=n), rs.uniform(size=n))
            tgt = c + 1.3 * (tgt - c) if k != "sphere" else tgt
            aim = rs.uniform(size=n) < .6
            wi[sel] = np.where(aim[:, None], F._norm(tgt - p[sel]), wi[sel])
    p = p.astype(np.float32)
    wi = wi.astype(np.float32)
    nrm = (_unit(rs, N) * (rs.uniform(.9, 1.1, N)[:, None] if name == "infinite" else 1.0)).astype(np.float32)
    u = rs.uniform(size=(N, 2)).astype(np.float32)
    u = np.minimum(u, TOP)
    # the special points of the sampling maps: the first queries of every light, in both forms
    special = [(np.float32(0), np.float32(0)), (np.float32(0), np.float32(.5)), (TOP, np.float32(.5)), (TOP, TOP)]
    for j, (a, b) in enumerate(special):
        for r in range(2):
            rows = slice((2 * j + r) * nl, (2 * j + r + 1) * nl)
            u[rows, 0], u[rows, 1] = a, b
    key = rs.randint(0, 1 << 20, N).astype(np.uint32)
    key[::97] = np.uint32(0xFFFFFFF0) + (np.arange(len(key[::97])) % 8).astype(np.uint32)
    rng = np.stack([key, rs.randint(0, 7, N).astype(np.uint32)], -1).astype(np.uint32)
    return dict(p=p, nrm=nrm, light=li, with_normal=wn, u=u, rng=rng, wi=wi)


def query_records(q):
    """the probe's input: 16 words per query (tests/golden/light_probe.cpp)"""
    rec = np.zeros((len(q["p"]), 16), np.float32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 8:10], rec[:, 12:15] = q["p"], q["nrm"], q["u"], q["wi"]
    iv = rec.view(np.int32)
    iv[:, 6], iv[:, 7] = q["light"], q["with_normal"]
    rec.view(np.uint32)[:, 10:12] = q["rng"]
    return rec


def answer(ans, k):
    a = ans[:, COLUMNS[k]]
    return a.astype(np.int32) if k in ("s_draws", "is_delta") else a


# ---------------------------------------------------------------------------------------------- the forms on a fixture
def evaluate(name, q, seed=SEED):
    """the float64 forms on the records `q` -> dict of the outputs of light_forms' query() over all queries, `excluded` (the band) and `tag`"""
    fs = forms(name)
    N = len(q["p"])
    draw = LF.keyed_draw(q["rng"][:, 0], q["rng"][:, 1], seed)
    out = None
    for l, f in enumerate(fs):
        for wn in (0, 1):
            sel = np.nonzero((q["light"] == l) & (q["with_normal"] == wn))[0]
            if not len(sel):
                continue
            g = lambda k: q[k][sel].astype(np.float64)
            r = f.query(g("p"), g("nrm"), bool(wn), g("u")[:, 0], g("u")[:, 1], draw[sel], g("wi"))
            if out is None:
                out = {k: np.zeros((N,) + v.shape[1:], v.dtype) for k, v in r.items()}
            for k, v in r.items():
                out[k][sel] = v
    out["excluded"] = out.pop("band")
    return out


def ref_err(name, q, ans, seed=SEED):
    """-> ({output: the reference's largest error against the forms over the included queries}, left-out share, the forms' dict)"""
    w = evaluate(name, q, seed)
    inc = ~w["excluded"]
    err = {k: float(B.query_error(answer(ans, k), w[k], inc, unit_scale=(k == "s_wi"))[inc].max()) for k in OUTPUTS}
    return err, float(w["excluded"].mean()), w


def coverage(name, q, w):
    """what the included queries reach, per light: the generator refuses a case in which a light, an emitter triangle (sampled, and hit last by a Pdf
    direction), a spot zone, a sphere branch or a side of the infinite light's flip is reached by none -> list of what is missing"""
    missing = []
    inc = ~w["excluded"]
    for l, d in enumerate(CASES[name]):
        sel = inc & (q["light"] == l)
        tag = w["tag"][sel]
        if not sel.any():
            missing.append((l, "no query"))
        if d["kind"] == "spot" and set(np.unique(tag)) != {0, 1, 2}:
            missing.append((l, "spot zones", sorted(set(np.unique(tag)))))
        if d["kind"] == "tri":
            T = len(d["indices"]) // 3
            if set(np.unique(tag // 16)) != set(range(T)):
                missing.append((l, "triangles sampled", sorted(set(np.unique(tag // 16)))))
            if set(np.unique(tag % 16)) != set(range(T + 1)):
                missing.append((l, "triangles hit last by a Pdf direction (0: a miss)", sorted(set(np.unique(tag % 16)))))
        if d["kind"] == "sphere" and set(np.unique(tag % 4)) != {1, 2}:
            missing.append((l, "sphere branches"))
        if d["kind"] in ("sphere", "disk", "cylinder") and set(np.unique(tag // 4)) != {0, 1}:
            missing.append((l, "Pdf directions that hit and that miss"))
        if d["kind"] == "infinite" and set(np.unique(w["tag"][sel & (q["with_normal"] == 1)])) != {0, 1}:
            missing.append((l, "both sides of the z flip"))
    return missing
