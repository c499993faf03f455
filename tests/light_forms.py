"""Float64 forms of what EstimateDirect asks of a light (core/transport.cpp): Light::Sample_L with a normal and without, Light::Pdf, Light::Le and
Light::IsDeltaLight, for the point, spot and distant lights (analytic_forms.Light, reused), emitters made of triangles (lights/area.cpp over
core/shape.h's ShapeSet and shapes/trianglemesh.cpp), the three quadric emitters (shapes/sphere.cpp, disk.cpp, cylinder.cpp) and the infinite light
with a constant radiance (lights/infinite.cpp).  Plain numpy, vectorised over the queries of ONE light, independent of the package; written from
the reference's text, whose file:line each function names.  Every light answers

    query(p, n, with_normal, u1, u2, draw, wi) -> dict(s_wi, s_L, s_pdf, s_ray_o, s_ray_d, mint, maxt, s_draws, pdf, le, is_delta,
                                                        band (bool: the exclusion rule), tag (int: what the query reached -- a triangle, a zone, a branch))

`draw` is the float32 value RandomFloat() returns at the query's place in its keyed stream (keyed_draw below): the one value of a query that is not
float64, because the reference compares that very float32 with its float32 cdf."""
import numpy as np

import analytic_forms as F

RAY_EPSILON = F.RAY_EPSILON
PI = np.pi
EDGE_BAND = 1e-5            # barycentric distance from an emitter triangle's edge (and relative distance from a quadric's rim) inside which a hit is undecided
COS_BAND = 1e-5             # distance of the spot's cosine from its two cone cosines
CDF_ULPS = 4                # a draw within this many float32 ulps (2^-24) of a cdf step
SILHOUETTE_BAND = 1e-3      # u1 below this: a cone sample within a thousandth of the cone's height of the sphere's silhouette
PLANE_BAND = 1e-6           # |cos| between a direction and an emitter's plane below this, but not zero: the plane is one of the triangle's edges seen edge on


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt(_dot(v, v))[..., None]


# ------------------------------------------------------------------------------------------------ the keyed stream (oracle/ref/keyed_rng.cpp)
def pcg(v):
    v = np.asarray(v, np.uint64) & 0xFFFFFFFF
    s = (v * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
    return ((w >> 22) ^ w) & 0xFFFFFFFF


def keyed_draw(key, counter, seed):
    """RandomFloat() number `counter` of the stream of camera sample `key`: (pcg(counter + pcg(key + seed * 0x9E3779B9)) & 0xffffff) / 2^24, a float32
    (core/util.cpp:377-380)"""
    base = pcg(np.asarray(key, np.uint64) + ((np.uint64(seed) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)))
    return ((pcg(np.asarray(counter, np.uint64) + base) & 0xFFFFFF).astype(np.float64) / 2.0 ** 24).astype(np.float32)


def _result(n):
    z3 = lambda: np.zeros((n, 3))
    return dict(s_wi=z3(), s_L=z3(), s_pdf=np.zeros(n), s_ray_o=z3(), s_ray_d=z3(), mint=np.zeros(n, np.float32), maxt=np.zeros(n, np.float32),
                s_draws=np.zeros(n, np.int32), pdf=np.zeros(n), le=z3(), is_delta=np.zeros(n, np.int32), band=np.zeros(n, bool), tag=np.zeros(n, np.int64))


def _segment(r, p, ps):
    """VisibilityTester::SetSegment light.h:78-80"""
    r["s_ray_o"], r["s_ray_d"] = p.copy(), ps - p
    r["mint"][:], r["maxt"][:] = np.float32(1e-3), np.float32(1) - np.float32(1e-3)


def _ray(r, p, w):
    """VisibilityTester::SetRay light.h:81-83"""
    r["s_ray_o"], r["s_ray_d"] = p.copy(), w.copy()
    r["mint"][:], r["maxt"][:] = np.float32(1e-3), np.float32(np.inf)


# ------------------------------------------------------------------------------------------------ point, spot, distant
class Delta:
    """point.cpp:55-66, spot.cpp:61-84, distant.cpp:57-67 through analytic_forms.Light: Sample_L(p, u1, u2, ...) is Sample_L(p, ...) with pdf = 1, and the
    form with a normal is the light.h:58-62 default; Pdf is 0; Le is Light::Le, black.  tag: the spot's zone (0 outside, 1 falloff, 2 full)."""

    def __init__(self, light):
        self.light = light

    def query(self, p, n, with_normal, u1, u2, draw, wi):
        r = _result(len(p))
        li, w, end, zone = self.light.sample(p)
        r["s_wi"], r["s_L"], r["s_pdf"][:] = np.array(w), np.array(li), 1.0
        if end is None:
            _ray(r, p, r["s_wi"])
        else:
            _segment(r, p, np.broadcast_to(end, p.shape))
        r["is_delta"][:] = 1
        r["tag"] = zone
        if self.light.kind == "spot":
            L = self.light
            c = _dot(_norm((-r["s_wi"]) @ L.w2l.T), L.axis)
            r["band"] = (np.abs(c - L.cos_total) < COS_BAND) | (np.abs(c - L.cos_start) < COS_BAND)
        return r


# ------------------------------------------------------------------------------------------------ emitters of triangles
class TriEmitter:
    """An emitting trianglemesh: AreaLight (area.cpp:30-57) refines it into Triangles; one triangle is the light's shape itself, several become a
    ShapeSet (shape.h:112-170) -- in the REVERSE of the mesh's order: the refinement loop (area.cpp:38-47) pops its work from the back.  `tris`:
    world-space vertices [T, 3, 3] in the mesh's order (trianglemesh.cpp:167-168 transforms them once); `reverse`: ReverseOrientation.  self.t, the
    cdf and the tags are in the set's order."""

    def __init__(self, tris, reverse, L):
        self.t, self.reverse, self.L = np.asarray(tris, np.float64)[::-1].copy(), bool(reverse), F.f32(L)
        e1, e2 = self.t[:, 1] - self.t[:, 0], self.t[:, 2] - self.t[:, 0]
        cr = np.cross(e1, e2)
        self.areas = .5 * np.linalg.norm(cr, axis=-1)                      # Triangle::Area trianglemesh.cpp:329-335
        self.area = self.areas.sum()
        self.cdf = np.cumsum(self.areas / self.area)                       # ShapeSet ctor shape.h:133-137
        self.ns = _norm(cr) * (-1.0 if self.reverse else 1.0)              # Triangle::Sample :345-347 (the handedness of the transform is in the vertices)

    def shape_pdf(self, p, wi):
        """Shape::Pdf(p, wi) shape.h:96-107 over ShapeSet::Intersect :150-156: every triangle is tested against the same ray (p, wi, RAY_EPSILON, inf)
        and the LAST one hit leaves its thit and normal.  -> pdf, band, last triangle hit (-1: none)"""
        n = len(p)
        thit, cosn, last, band = np.zeros(n), np.ones(n), np.full(n, -1, np.int64), np.zeros(n, bool)
        for k in range(len(self.t)):
            p1 = self.t[k, 0]
            e1, e2 = self.t[k, 1] - p1, self.t[k, 2] - p1
            s1 = np.cross(wi, e2)                                          # Triangle::Intersect trianglemesh.cpp:213-246
            div = _dot(s1, e1)
            with np.errstate(all="ignore"):
                d = p - p1
                b1 = _dot(d, s1) / div
                s2 = np.cross(d, e1)
                b2 = _dot(wi, s2) / div
                t = _dot(s2, e2) / div
            m = np.minimum(np.minimum(b1, b2), 1 - b1 - b2)
            hit = (div != 0) & (m >= 0) & (t >= RAY_EPSILON)
            cos_k = np.abs(_dot(wi, _norm(np.cross(e1, e2))))
            near_plane = (cos_k < PLANE_BAND) & (div != 0)
            with np.errstate(invalid="ignore"):
                band |= near_plane | ((div != 0) & (np.abs(m) < EDGE_BAND) & (t > 0)) | ((div != 0) & (m > -EDGE_BAND) & (np.abs(t - RAY_EPSILON) < 1e-5))
            thit, cosn, last = np.where(hit, t, thit), np.where(hit, cos_k, cosn), np.where(hit, k, last)
        with np.errstate(all="ignore"):
            pdf = (thit * thit * _dot(wi, wi)) / (cosn * self.area)        # DistanceSquared(p, ray(thit)) / (AbsDot(nn, -wi) * Area())
        pdf = np.where((last < 0) | (cosn == 0), 0.0, pdf)
        return pdf, band, last

    def query(self, p, n, with_normal, u1, u2, draw, wi):
        r = _result(len(p))
        T = len(self.t)
        k = np.zeros(len(p), np.int64)
        if T > 1:                                                          # ShapeSet::Sample shape.h:115-121: one RandomFloat(), the first cdf entry above it
            r["s_draws"][:] = 1
            cdf32 = self.cdf[:-1]
            k = (draw.astype(np.float64)[:, None] >= cdf32[None, :]).sum(-1)
            r["band"] |= (np.abs(draw.astype(np.float64)[:, None] - cdf32[None, :]) <= CDF_ULPS * 2.0 ** -24).any(-1)
        su = np.sqrt(u1)                                                   # UniformSampleTriangle mc.cpp:136-141
        b1, b2 = 1 - su, u2 * su
        tk = self.t[k]
        ps = b1[:, None] * tk[:, 0] + b2[:, None] * tk[:, 1] + (1 - b1 - b2)[:, None] * tk[:, 2]
        ns = self.ns[k]
        w = _norm(ps - p)                                                  # area.cpp:58-68 / :73-82: the two forms are one text
        r["s_wi"] = w
        r["s_pdf"], band, _ = self.shape_pdf(p, w)
        r["band"] |= band
        r["s_L"] = np.where((_dot(ns, -w) > 0)[:, None], self.L, 0.0)      # AreaLight::L light.h:93-96
        _segment(r, p, ps)
        r["pdf"], band, last = self.shape_pdf(p, wi)                       # area.cpp:69-72, :93-95
        r["band"] |= band
        r["tag"] = k * 16 + (last + 1)                                     # the triangle sampled, and the triangle the Pdf direction hit last (0: none)
        return r


# ------------------------------------------------------------------------------------------------ emitters on quadrics
class QuadricEmitter:
    """A sphere, disk or cylinder with an AreaLightSource (full shapes: no zmin / zmax / phimax cut on the sphere, no inner radius), under a
    rigid object-to-world matrix `o2w`.  Sample(u1, u2): sphere.cpp:38-44, disk.cpp:37-46, cylinder.cpp:37-45; the sphere's Sample(p, ...) and Pdf(p, wi):
    sphere.cpp:45-79; the others take the Shape defaults (shape.h:92-107).  tag: 1 cone branch, 2 inside branch, 0 otherwise; + 4 if the Pdf direction hits."""

    def __init__(self, kind, o2w, reverse, L, **kw):
        self.kind, self.o2w, self.reverse, self.L = kind, o2w, bool(reverse), F.f32(L)
        self.shape = F.Quadric(kind, o2w=o2w, **kw)
        s = self.shape
        if kind == "sphere":
            self.area = s.phimax * s.radius * (s.zmax - s.zmin)            # sphere.cpp:251-253
        elif kind == "disk":
            self.area = s.phimax * .5 * (s.radius ** 2 - s.inner ** 2)     # disk.cpp:124-127
        else:
            self.area = (s.zmax - s.zmin) * s.phimax * s.radius            # cylinder.cpp:180-182

    def _uniform(self, u1, u2):
        s = self.shape
        if self.kind == "disk":
            x, y = F.concentric_sample_disk(u1, u2)
            po = np.stack([x * s.radius, y * s.radius, np.full(u1.shape, s.height)], -1)
            no = np.broadcast_to(np.array([0.0, 0.0, 1.0]), po.shape)
        elif self.kind == "cylinder":
            z, t = (1 - u1) * s.zmin + u1 * s.zmax, u2 * s.phimax
            po = np.stack([s.radius * np.cos(t), s.radius * np.sin(t), z], -1)
            no = np.stack([po[:, 0], po[:, 1], np.zeros(len(z))], -1)
        else:
            z = 1 - 2 * u1                                                 # UniformSampleSphere mc.cpp:74-81
            rr, phi = np.sqrt(np.maximum(0, 1 - z * z)), 2 * PI * u2
            po = s.radius * np.stack([rr * np.cos(phi), rr * np.sin(phi), z], -1)
            no = po
        ns = _norm(F.xnormal(self.o2w, no)) * (-1.0 if self.reverse else 1.0)
        return F.xpoint(self.o2w, po), ns

    def _rim_band(self, p, w, t):
        """a hit within a band of the shape's rim: the disk's circle, the cylinder's two ends"""
        s = self.shape
        with np.errstate(all="ignore"):
            po = F.xpoint(s.w2o, p + np.where(np.isfinite(t), t, 0.0)[:, None] * w)
        if self.kind == "disk":
            dz = F.xvec(s.w2o, w)[:, 2]
            with np.errstate(all="ignore"):
                tp = (s.height - F.xpoint(s.w2o, p)[:, 2]) / dz
            pp = F.xpoint(s.w2o, p + np.where(np.isfinite(tp), tp, 0.0)[:, None] * w)
            return np.isfinite(tp) & (tp > 0) & (np.abs(np.hypot(pp[:, 0], pp[:, 1]) - s.radius) < 1e-5 * s.radius)
        if self.kind == "cylinder":
            return np.isfinite(t) & ((np.abs(po[:, 2] - s.zmin) < 1e-5) | (np.abs(po[:, 2] - s.zmax) < 1e-5) | (np.hypot(po[:, 0], po[:, 1]) < 1e-9))
        return np.zeros(len(p), bool)

    def shape_pdf(self, p, wi):
        """Shape::Pdf(p, wi) shape.h:96-107 -> pdf, band, hit"""
        t, nn, _ = self.shape.intersect(p, wi, RAY_EPSILON, np.inf)
        hit = np.isfinite(t)
        cosn = np.abs(_dot(nn, wi))
        with np.errstate(all="ignore"):
            pdf = np.where(hit & (cosn != 0), (t * t * _dot(wi, wi)) / (cosn * self.area), 0.0)
        # a direction that grazes the shape (the quadratic's discriminant near zero: the silhouette) or meets its rim is undecided
        band = self._rim_band(p, wi, t)
        if self.kind != "disk":
            s = self.shape
            oo, od = F.xpoint(s.w2o, p), F.xvec(s.w2o, wi)
            if self.kind == "cylinder":
                oo, od = oo * np.array([1.0, 1.0, 0.0]), od * np.array([1.0, 1.0, 0.0])
            A, B, C = _dot(od, od), 2 * _dot(od, oo), _dot(oo, oo) - s.radius ** 2
            with np.errstate(all="ignore"):
                band |= np.abs(B * B - 4 * A * C) < 1e-4 * np.abs(B * B)
        return pdf, band, hit

    def query(self, p, n, with_normal, u1, u2, draw, wi):
        r = _result(len(p))
        s = self.shape
        ps, ns = self._uniform(u1, u2)
        tag = np.zeros(len(p), np.int64)
        if self.kind == "sphere":
            c = F.xpoint(self.o2w, np.zeros(3))
            d2 = _dot(p - c, p - c)
            outside = ~(d2 - s.radius ** 2 < 1e-4)                         # sphere.cpp:53 (a float32 comparison: points within 1e-5 of the threshold are in the band)
            r["band"] |= np.abs(d2 - s.radius ** 2 - 1e-4) < 1e-5
            wc = _norm(c - p)
            ax = np.abs(wc[:, 0]) > np.abs(wc[:, 1])                       # CoordinateSystem geometry.h:324-334
            with np.errstate(all="ignore"):
                vx = np.where(ax[:, None], np.stack([-wc[:, 2], np.zeros(len(p)), wc[:, 0]], -1) / np.sqrt(wc[:, 0] ** 2 + wc[:, 2] ** 2)[:, None],
                              np.stack([np.zeros(len(p)), wc[:, 2], -wc[:, 1]], -1) / np.sqrt(wc[:, 1] ** 2 + wc[:, 2] ** 2)[:, None])
            vy = np.cross(wc, vx)
            with np.errstate(all="ignore"):
                cmax = np.sqrt(np.maximum(0, 1 - s.radius ** 2 / d2))
            ct = (1 - u1) * cmax + u1                                      # UniformSampleCone mc.cpp:154-161
            st, phi = np.sqrt(np.maximum(0, 1 - ct * ct)), u2 * 2 * PI
            rd = vx * (np.cos(phi) * st)[:, None] + vy * (np.sin(phi) * st)[:, None] + wc * ct[:, None]
            t, _, _ = s.intersect(p, rd, RAY_EPSILON, np.inf)
            t = np.where(np.isfinite(t), t, _dot(c - p, _norm(rd)))        # sphere.cpp:63-64
            pc = p + rd * t[:, None]
            nc = _norm(pc - c) * (-1.0 if self.reverse else 1.0)
            ps, ns = np.where(outside[:, None], pc, ps), np.where(outside[:, None], nc, ns)
            r["band"] |= outside & (u1 < SILHOUETTE_BAND)
            tag = np.where(outside, 1, 2)
        w = _norm(ps - p)
        r["s_wi"] = w
        pdf_s, band_s, _ = self.shape_pdf(p, w)
        pdf_w, band_w, hit_w = self.shape_pdf(p, wi)
        if self.kind == "sphere":
            with np.errstate(all="ignore"):
                cone = 1 / (2 * PI * (1 - cmax))                           # UniformConePdf mc.cpp:142-144
            pdf_s, pdf_w = np.where(outside, cone, pdf_s), np.where(outside, cone, pdf_w)
            band_s, band_w = band_s & ~outside, band_w & ~outside
        r["s_pdf"], r["pdf"] = pdf_s, pdf_w
        r["band"] |= band_s | band_w
        r["s_L"] = np.where((_dot(ns, -w) > 0)[:, None], self.L, 0.0)
        _segment(r, p, ps)
        r["tag"] = tag + 4 * hit_w
        return r


# ------------------------------------------------------------------------------------------------ the infinite light
class Infinite:
    """LightSource "infinite" with a constant radiance (infinite.cpp): with a normal a cosine-weighted direction about +-n whose side one RandomFloat()
    decides (:96-116), Pdf = |n . wi| / 2 pi (:117-120); without, a uniform direction and 1 / 4 pi (:121-131).  Le = L (:83-95).  tag: 1 if z was flipped."""

    def __init__(self, L):
        self.L = F.f32(L)

    def query(self, p, n, with_normal, u1, u2, draw, wi):
        r = _result(len(p))
        if with_normal:
            x, y = F.concentric_sample_disk(u1, u2)
            z = np.sqrt(np.maximum(0, 1 - x * x - y * y))
            flip = draw < np.float32(.5)
            z = np.where(flip, -z, z)
            r["s_pdf"] = np.abs(z) / (2 * PI)
            v1 = _norm(n)                                                  # CoordinateSystem(Normalize(n)) and n ITSELF in the third column (:110-113)
            ax = np.abs(v1[:, 0]) > np.abs(v1[:, 1])
            with np.errstate(all="ignore"):
                a = np.where(ax[:, None], np.stack([-v1[:, 2], np.zeros(len(p)), v1[:, 0]], -1) / np.sqrt(v1[:, 0] ** 2 + v1[:, 2] ** 2)[:, None],
                             np.stack([np.zeros(len(p)), v1[:, 2], -v1[:, 1]], -1) / np.sqrt(v1[:, 1] ** 2 + v1[:, 2] ** 2)[:, None])
            b = np.cross(v1, a)
            r["s_wi"] = a * x[:, None] + b * y[:, None] + n * z[:, None]
            r["s_draws"][:] = 1
            r["pdf"] = np.abs(_dot(n, wi)) / (2 * PI)
            r["tag"] = flip.astype(np.int64)
        else:
            z = 1 - 2 * u1
            rr, phi = np.sqrt(np.maximum(0, 1 - z * z)), 2 * PI * u2
            r["s_wi"] = np.stack([rr * np.cos(phi), rr * np.sin(phi), z], -1)
            r["s_pdf"][:] = 1 / (4 * PI)
            r["pdf"][:] = 1 / (4 * PI)
        r["s_L"] = np.broadcast_to(self.L, p.shape).copy()
        r["le"] = r["s_L"].copy()
        _ray(r, p, r["s_wi"])
        return r
