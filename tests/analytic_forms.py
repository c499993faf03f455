"""Float64 closed forms of what one Whitted camera sample computes in a scene of a few analytic surfaces lit by delta lights: cameras,
ray / quad and ray / quadric intersection, point / spot / distant lights, the BSDFs of matte, plastic, uber, shinymetal and translucent
as the reference assembles them, the mirror step and the transmittance of a homogeneous medium.  Plain numpy, vectorised over samples,
independent of the package: tests/test_analytic_host.py proves on the reference's films that these are the reference's functions,
tests/test_gpu_analytic.py holds the device's per-sample radiance to them.

Written from the formulas; the comments name the place in the reference (pbrt-v1) that fixes each convention.  Every scene parameter
is rounded to float32 first (the scene file holds floats), everything after that is float64."""
import numpy as np

RAY_EPSILON = float(np.float32(1e-3))         # core/pbrt.h:211
PI = np.pi


def f32(x):
    """a scene parameter as the file format holds it (float32), as float64"""
    return np.asarray(np.asarray(x, np.float32), np.float64)


def _norm(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return (a * b).sum(-1)


# ------------------------------------------------------------------------------------------------ transforms (4 x 4, column vectors)
def identity():
    return np.eye(4)


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = f32([x, y, z])
    return m


def scale(x, y, z):
    return np.diag(np.append(f32([x, y, z]), 1.0))


def rotate(deg, x, y, z):
    """core/transform.cpp:73-111: right-handed rotation by `deg` degrees about the normalised axis"""
    a = _norm(f32([x, y, z]))
    t = np.radians(float(f32(deg)))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.cos(t) * np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * np.outer(a, a)
    return m


def look_at(pos, look, up):
    """core/transform.cpp:113-138: the world-to-camera matrix.  right = Normalize(Cross(dir, up)) (:122), so a camera at -z that looks
    along +z with up = +y has right = -x: with raster y running down, raster x runs towards world -x."""
    pos, look, up = f32(pos), f32(look), f32(up)
    d = _norm(look - pos)
    right = _norm(np.cross(d, up))
    new_up = np.cross(right, d)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, new_up, d, pos
    return np.linalg.inv(c2w)


def compose(*ms):
    """the CTM after the statements `ms` in file order (each statement post-multiplies: core/api.cpp)"""
    out = np.eye(4)
    for m in ms:
        out = out @ m
    return out


def xpoint(m, p):
    q = p @ m[:3, :3].T + m[:3, 3]
    return q


def xvec(m, v):
    return v @ m[:3, :3].T


def xnormal(m, n):
    """a normal under `m`: the inverse transpose (core/transform.h Transform::operator()(const Normal &))"""
    return n @ np.linalg.inv(m[:3, :3])


# ------------------------------------------------------------------------------------------------ cameras
def concentric_sample_disk(u1, u2):
    """ConcentricSampleDisk (core/mc.cpp): the square [0, 1]^2 onto the unit disk, four wedges; (.5, .5) is the centre"""
    sx, sy = 2 * np.asarray(u1, np.float64) - 1, 2 * np.asarray(u2, np.float64) - 1
    with np.errstate(all="ignore"):
        r = np.where(sx >= -sy, np.where(sx > sy, sx, sy), np.where(sx <= sy, -sx, -sy))
        theta = np.where(sx >= -sy, np.where(sx > sy, np.where(sy > 0, sy / sx, 8 + sy / sx), 2 - sx / sy), np.where(sx <= sy, 4 + sy / sx, 6 - sx / sy))
    theta = np.where((sx == 0) & (sy == 0), 0.0, theta) * PI / 4
    r = np.where((sx == 0) & (sy == 0), 0.0, r)
    return r * np.cos(theta), r * np.sin(theta)


class Camera:
    """image position -> world ray (o, d, mint, maxt).  kind: "perspective" (cameras/perspective.cpp:45-79), "orthographic"
    (cameras/orthographic.cpp:48-79; no lens), "environment" (cameras/environment.cpp:48-61).  The screen window defaults to
    [-a, a] x [-1, 1] for an aspect a > 1 and [-1, 1] x [-1/a, 1/a] otherwise (perspective.cpp:93-106); RasterToScreen is
    core/camera.cpp:62-67 (raster y runs down: y = 0 is screen[3])."""

    def __init__(self, kind, xres, yres, world_to_camera, fov=90.0, hither=1e-3, yon=1e30, screen=None, lensradius=0.0, focaldistance=1e30):
        self.kind, self.xres, self.yres = kind, int(xres), int(yres)
        self.lensradius, self.focaldistance = float(f32(lensradius)), float(f32(focaldistance))
        self.c2w = np.linalg.inv(world_to_camera)
        self.hither = max(1e-4, float(f32(hither)))
        self.yon = min(float(f32(yon)), 1e30)
        self.tan_half = np.tan(np.radians(float(f32(fov))) / 2)
        a = float(np.float32(xres) / np.float32(yres))
        self.screen = f32(screen) if screen is not None else (np.array([-a, a, -1.0, 1.0]) if a > 1 else np.array([-1.0, 1.0, -1 / a, 1 / a]))

    def rays(self, ix, iy, lens_u=0.5, lens_v=0.5):
        """(lens_u, lens_v): the lens sample of the thin lens; an unjittered stratified 1 x 1 sampler gives (.5, .5), the lens centre"""
        ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
        s = self.screen
        if self.kind == "environment":
            theta, phi = PI * iy / self.yres, 2 * PI * ix / self.xres
            d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], -1)
            o = np.broadcast_to(self.c2w[:3, 3], d.shape).copy()
            return o, xvec(self.c2w, d), np.full(ix.shape, self.hither), np.full(ix.shape, self.yon)
        sx = s[0] + ix / self.xres * (s[1] - s[0])
        sy = s[3] + iy / self.yres * (s[2] - s[3])
        if self.kind == "perspective":
            # Perspective(fov, n, f) (core/transform.cpp:182-194): raster z = 0 is the plane z = hither, x' = x / (z tan(fov / 2))
            pc = np.stack([sx * self.hither * self.tan_half, sy * self.hither * self.tan_half, np.full(ix.shape, self.hither)], -1)
            d = _norm(pc)
            if self.lensradius > 0:
                # the thin lens (cameras/perspective.cpp:59-73): the point of the plane of focus that the pinhole ray meets is seen from a
                # point of the lens; the origin moves by the lens point scaled by (focaldistance - hither) / focaldistance
                lu, lv = concentric_sample_disk(np.broadcast_to(lens_u, ix.shape), np.broadcast_to(lens_v, ix.shape))
                focus = pc + ((self.focaldistance - self.hither) / d[..., 2])[..., None] * d
                k = self.lensradius * (self.focaldistance - self.hither) / self.focaldistance
                pc = pc + np.stack([lu * k, lv * k, np.zeros(ix.shape)], -1)
                d = _norm(focus - pc)
            maxt = (self.yon - self.hither) / d[..., 2]
        elif self.kind == "orthographic":
            pc = np.stack([sx, sy, np.full(ix.shape, self.hither)], -1)          # Orthographic(n, f): z' = (z - n) / (f - n)
            d = np.broadcast_to(np.array([0.0, 0.0, 1.0]), pc.shape).copy()
            maxt = np.full(ix.shape, self.yon - self.hither)
        else:
            raise ValueError(self.kind)
        return xpoint(self.c2w, pc), xvec(self.c2w, d), np.zeros(ix.shape), maxt


# ------------------------------------------------------------------------------------------------ intersectors
class Quad:
    """Four coplanar world-space corners P0..P3 as the two triangles (0 1 2) (0 2 3) of a `trianglemesh`.  The geometric normal is
    Normalize(Cross(dpdu, dpdv)) with the default uvs (0,0) (1,0) (1,1) (shapes/trianglemesh.cpp:199-221): along (P0 - P2) x (P1 - P2);
    only its line matters to every BSDF here but glass.  The inner diagonal is no edge: a hit is a hit of the convex quad."""

    def __init__(self, corners, o2w=None):
        p = f32(corners).reshape(4, 3)
        self.p = xpoint(o2w, p) if o2w is not None else p
        self.n = _norm(np.cross(self.p[0] - self.p[2], self.p[1] - self.p[2]))

    def intersect(self, o, d, mint, maxt):
        """-> t (inf where missed), n, root (0)"""
        dn = _dot(d, self.n)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = _dot(self.p[0] - o, self.n) / dn
        ph = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
        centre = self.p.mean(0)
        edge = np.full(t.shape, np.inf)
        for i in range(4):
            a, b = self.p[i], self.p[(i + 1) % 4]
            inward = _norm(np.cross(self.n, b - a))
            inward = inward if _dot(centre - a, inward) > 0 else -inward
            edge = np.minimum(edge, _dot(ph - a, inward))
        ok = np.isfinite(t) & (t >= mint) & (t <= maxt) & (edge >= 0)
        t = np.where(ok, t, np.inf)
        return t, np.broadcast_to(self.n, d.shape), np.zeros(t.shape, np.int64)


class Quadric:
    """The six quadrics under an arbitrary object-to-world matrix.  The ray goes to object space unnormalised (so t is the world
    parameter), the quadratic is solved, and the roots go through the reference's rule (shapes/sphere.cpp:102-141, cylinder.cpp:66-104,
    cone.cpp:54-96, paraboloid.cpp:58-97, hyperboloid.cpp:80-133): the nearer root inside [mint, maxt], and when the clip (z range,
    phi > phimax) rejects it, the far root if that was not it already.  The disk (shapes/disk.cpp:64-85) is a plane with radii and phimax.
    The geometric normal is the gradient of the implicit form under the inverse transpose, renormalised (the hyperboloid's: see
    intersect); its sign (ReverseOrientation,
    a handedness swap: core/shape.cpp:49) changes no BSDF value here."""

    def __init__(self, kind, o2w=None, twin=None, **kw):
        self.kind, self.twin = kind, twin                 # twin: a deliberately wrong variant (tests only)
        self.o2w = np.eye(4) if o2w is None else o2w
        self.w2o = np.linalg.inv(self.o2w)
        g = lambda k, dflt: float(f32(kw.get(k, dflt)))
        self.phimax = np.radians(min(max(g("phimax", 360.0), 0.0), 360.0))
        if kind == "sphere":
            self.radius = g("radius", 1.0)
            z0, z1 = g("zmin", -self.radius), g("zmax", self.radius)
            self.zmin = min(max(min(z0, z1), -self.radius), self.radius)
            self.zmax = min(max(max(z0, z1), -self.radius), self.radius)
        elif kind == "disk":
            self.height, self.radius, self.inner = g("height", 0.0), g("radius", 1.0), g("innerradius", 0.0)
            if twin == "inner_radius_ignored":
                self.inner = 0.0
        elif kind == "cylinder":
            self.radius = g("radius", 1.0)
            z0, z1 = g("zmin", -1.0), g("zmax", 1.0)
            self.zmin, self.zmax = min(z0, z1), max(z0, z1)
        elif kind == "cone":
            self.radius, self.height = g("radius", 1.0), g("height", 1.0)
            self.zmin, self.zmax = 0.0, self.height
        elif kind == "paraboloid":
            self.radius = g("radius", 1.0)
            z0, z1 = g("zmin", 0.0), g("zmax", 1.0)
            self.zmin, self.zmax = min(z0, z1), max(z0, z1)
        elif kind == "hyperboloid":
            p1, p2 = f32(kw.get("p1", (0, 0, 0))), f32(kw.get("p2", (1, 1, 1)))
            self.zmin, self.zmax = min(p1[2], p2[2]), max(p1[2], p2[2])
            if p2[2] == 0:
                p1, p2 = p2, p1
            self.p1, self.p2 = p1, p2
            pp = p1.copy()
            while True:                                                      # hyperboloid.cpp:58-70
                pp = pp + 2 * (p2 - p1)
                xy1, xy2 = pp[0] ** 2 + pp[1] ** 2, p2[0] ** 2 + p2[1] ** 2
                with np.errstate(all="ignore"):
                    a = (1 / xy1 - pp[2] ** 2 / (xy1 * p2[2] ** 2)) / (1 - xy2 * pp[2] ** 2 / (xy1 * p2[2] ** 2))
                if np.isfinite(a):
                    break
            self.a, self.c = a, (a * xy2 - 1) / p2[2] ** 2
        else:
            raise ValueError(kind)

    def _phi(self, p):
        if self.kind == "hyperboloid":
            v = (p[..., 2] - self.p1[2]) / (self.p2[2] - self.p1[2])
            pr = (1 - v)[..., None] * self.p1 + v[..., None] * self.p2
            phi = np.arctan2(pr[..., 0] * p[..., 1] - p[..., 0] * pr[..., 1], p[..., 0] * pr[..., 0] + p[..., 1] * pr[..., 1])
        else:
            phi = np.arctan2(p[..., 1], p[..., 0])
        return np.where(phi < 0, phi + 2 * PI, phi)

    def uv(self, p_world):
        """(u, v) of a world-space hit point: u = phi / phimax, v by kind (sphere.cpp:146-148, disk.cpp:86-88, cylinder.cpp:106-107,
        cone.cpp:99-100, paraboloid.cpp:101-102, hyperboloid.cpp:107, :130)"""
        p = xpoint(self.w2o, p_world)
        z = p[..., 2]
        with np.errstate(all="ignore"):
            if self.kind == "sphere":
                th = lambda c: np.arccos(np.clip(c / self.radius, -1, 1))
                v = (th(z) - th(self.zmin)) / (th(self.zmax) - th(self.zmin))
            elif self.kind == "disk":
                v = 1 - (np.hypot(p[..., 0], p[..., 1]) - self.inner) / (self.radius - self.inner)
            elif self.kind == "cone":
                v = z / self.height
            elif self.kind == "hyperboloid":
                v = (z - self.p1[2]) / (self.p2[2] - self.p1[2])
            else:
                v = (z - self.zmin) / (self.zmax - self.zmin)
            return self._phi(p) / self.phimax, v

    def _clipped(self, p):
        return (p[..., 2] < self.zmin) | (p[..., 2] > self.zmax) | (self._phi(p) > self.phimax)

    def _gradient(self, p):
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        zero = np.zeros_like(x)
        if self.kind == "sphere":
            return p
        if self.kind == "disk":
            return np.stack([zero, zero, zero + 1], -1)
        if self.kind == "cylinder":
            return np.stack([x, y, zero], -1)
        if self.kind == "cone":
            k = (self.radius / self.height) ** 2
            return np.stack([x, y, -k * (z - self.height)], -1)
        if self.kind == "paraboloid":
            k = self.zmax / self.radius ** 2
            return np.stack([2 * k * x, 2 * k * y, zero - 1], -1)
        return np.stack([self.a * x, self.a * y, -self.c * z], -1)

    def intersect(self, o, d, mint, maxt):
        """-> t (inf where missed), world normal, root (0 = plane or near root, 1 = far root)"""
        oo, od = xpoint(self.w2o, o), xvec(self.w2o, d)
        ox, oy, oz, dx, dy, dz = oo[..., 0], oo[..., 1], oo[..., 2], od[..., 0], od[..., 1], od[..., 2]
        mint, maxt = np.broadcast_to(mint, ox.shape), np.broadcast_to(maxt, ox.shape)
        with np.errstate(all="ignore"):
            if self.kind == "disk":
                t = (self.height - oz) / dz
                ok = (np.abs(dz) >= 1e-7) & (t >= mint) & (t <= maxt)
                p = oo + np.where(ok, t, 0.0)[..., None] * od
                r2 = p[..., 0] ** 2 + p[..., 1] ** 2
                ok &= (r2 <= self.radius ** 2) & (r2 >= self.inner ** 2) & (self._phi(p) <= self.phimax)
                root = np.zeros(ox.shape, np.int64)
            else:
                if self.kind == "sphere":
                    A, B, C = dx * dx + dy * dy + dz * dz, 2 * (dx * ox + dy * oy + dz * oz), ox * ox + oy * oy + oz * oz - self.radius ** 2
                elif self.kind == "cylinder":
                    A, B, C = dx * dx + dy * dy, 2 * (dx * ox + dy * oy), ox * ox + oy * oy - self.radius ** 2
                elif self.kind == "cone":
                    k, h = (self.radius / self.height) ** 2, self.height
                    A, B, C = dx * dx + dy * dy - k * dz * dz, 2 * (dx * ox + dy * oy - k * dz * (oz - h)), ox * ox + oy * oy - k * (oz - h) ** 2
                elif self.kind == "paraboloid":
                    k = self.zmax / self.radius ** 2
                    A, B, C = k * (dx * dx + dy * dy), 2 * k * (dx * ox + dy * oy) - dz, k * (ox * ox + oy * oy) - oz
                else:
                    a, c = self.a, self.c
                    A, B, C = a * dx * dx + a * dy * dy - c * dz * dz, 2 * (a * dx * ox + a * dy * oy - c * dz * oz), a * ox * ox + a * oy * oy - c * oz * oz - 1
                disc = B * B - 4 * A * C                                          # Quadratic (core/pbrt.h:645-659)
                ok = disc >= 0
                q = -.5 * np.where(B < 0, B - np.sqrt(np.abs(disc)), B + np.sqrt(np.abs(disc)))
                ta, tb = q / A, C / q
                t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
                ok &= np.isfinite(t0) & np.isfinite(t1) & ~((t0 > maxt) | (t1 < mint))
                first_is_far = t0 < mint
                t = np.where(first_is_far, t1, t0)
                ok &= t <= maxt
                clip = self._clipped(oo + np.where(ok, t, 0.0)[..., None] * od)
                second = ok & clip & ~first_is_far & (t1 <= maxt)
                second &= ~self._clipped(oo + np.where(second, t1, 0.0)[..., None] * od)
                ok = (ok & ~clip) | second
                t = np.where(second, t1, t)
                root = (first_is_far | second).astype(np.int64)
                p = oo + np.where(ok, t, 0.0)[..., None] * od
            if self.kind == "hyperboloid":
                # the implicit form (a, c) has its waist at z = 0 whatever p1 and p2 are, so it does not contain the line p1 p2 in general;
                # the reference's normal is Cross(dpdu, dpdv) of the ruled parametrisation at the hit's phi (hyperboloid.cpp:135-147)
                phi = self._phi(p)
                zero = np.zeros_like(phi)
                e = self.p2 - self.p1
                dpdu = np.stack([-p[..., 1], p[..., 0], zero], -1)
                dpdv = np.stack([e[0] * np.cos(phi) - e[1] * np.sin(phi), e[0] * np.sin(phi) + e[1] * np.cos(phi), zero + e[2]], -1)
                n = np.cross(xvec(self.o2w, dpdu), xvec(self.o2w, dpdv))
            else:
                n = xnormal(self.o2w, _norm(self._gradient(np.where(ok[..., None], p, 1.0))))
            if self.twin != "normal_not_renormalised":
                n = _norm(n)
        return np.where(ok, t, np.inf), n, root


# ------------------------------------------------------------------------------------------------ lights
class Light:
    """kind "point" (lights/point.cpp:49-61), "spot" (lights/spot.cpp:52-78, :96-117), "distant" (lights/distant.cpp:54-68), under
    the light's CTM `l2w`.  sample(p) -> (Li, wi, segment end or None, zone): a point or spot light is tested over the segment p -> pos
    clipped to [RAY_EPSILON, 1 - RAY_EPSILON] (core/light.h:79), a distant one over [RAY_EPSILON, inf) of p + t wi (core/light.h:82)."""

    def __init__(self, kind, color, l2w=None, frm=(0, 0, 0), to=(0, 0, 1), coneangle=30.0, conedelta=5.0, twin=None):
        self.kind, self.color = kind, f32(color)
        l2w = np.eye(4) if l2w is None else l2w
        frm, to = f32(frm), f32(to)
        if kind == "distant":
            self.dir = _norm(xvec(l2w, frm - to))
            return
        self.pos = xpoint(l2w, frm)
        if kind == "spot":
            # WorldToLight of a vector is dirToZ A^-1 w (A the linear part of the CTM); dirToZ is orthonormal, so the cosine to the
            # axis is dir . A^-1 w / |A^-1 w|
            self.axis = _norm(to - frm)
            self.w2l = np.linalg.inv(l2w[:3, :3]) if twin != "spot_axis_untransformed" else np.eye(3)
            ca, cd = float(f32(coneangle)), float(f32(conedelta))
            self.cos_total, self.cos_start = np.cos(np.radians(ca)), np.cos(np.radians(float(np.float32(ca) - np.float32(cd))))

    def sample(self, p, exponent=4):
        if self.kind == "distant":
            wi = np.broadcast_to(self.dir, p.shape)
            return np.broadcast_to(self.color, p.shape), wi, None, np.zeros(p.shape[:-1], np.int64)
        to_l = self.pos - p
        d2 = _dot(to_l, to_l)
        wi = to_l / np.sqrt(d2)[..., None]
        li = self.color / d2[..., None]
        zone = np.zeros(p.shape[:-1], np.int64)
        if self.kind == "spot":
            wl = _norm((-wi) @ self.w2l.T)
            c = _dot(wl, self.axis)
            delta = (c - self.cos_total) / (self.cos_start - self.cos_total)
            fall = np.where(c < self.cos_total, 0.0, np.where(c > self.cos_start, 1.0, np.clip(delta, 0, 1) ** exponent))
            li = li * fall[..., None]
            zone = np.where(c < self.cos_total, 0, np.where(c > self.cos_start, 2, 1))
        return li, wi, self.pos, zone


# ------------------------------------------------------------------------------------------------ BSDFs
def fr_dielectric(cosi, eta_i, eta_t):
    """FresnelDielectric::Evaluate (core/reflection.cpp:77-95).  plastic, uber and translucent construct it as (1.5, 1), so for the
    half-vector cosine > 0 light "enters" from index 1.5 into 1 and total reflection (1) is reported beyond sin = 2 / 3."""
    cosi = np.clip(cosi, -1, 1)
    ei = np.where(cosi > 0, eta_i, eta_t)
    et = np.where(cosi > 0, eta_t, eta_i)
    sint = ei / et * np.sqrt(np.maximum(0, 1 - cosi * cosi))
    cost = np.sqrt(np.maximum(0, 1 - np.minimum(sint, 1) ** 2))
    ci = np.abs(cosi)
    with np.errstate(all="ignore"):
        rpar = (et * ci - ei * cost) / (et * ci + ei * cost)
        rper = (ei * ci - et * cost) / (ei * ci + et * cost)
    return np.where(sint >= 1, 1.0, (rpar * rpar + rper * rper) / 2)


def fr_conductor(cosi, eta, k=0.0):
    """FrCond (core/reflection.cpp:40-51); eta per channel"""
    c = np.abs(cosi)[..., None]
    tmp = (eta * eta + k * k) * c * c
    rpar = (tmp - 2 * eta * c + 1) / (tmp + 2 * eta * c + 1)
    tf = eta * eta + k * k
    rper = (tf - 2 * eta * c + c * c) / (tf + 2 * eta * c + c * c)
    return (rpar + rper) / 2


def approx_eta(r):
    """FresnelApproxEta (core/reflection.cpp:52-56): the reflectance is clamped to .999 first"""
    s = np.sqrt(np.clip(r, 0, .999))
    return (1 + s) / (1 - s)


def blinn_exponent(roughness):
    """Blinn(1 / roughness) with the cap (core/reflection.h:313)"""
    with np.errstate(divide="ignore"):
        e = 1.0 / float(f32(roughness))
    return 1000.0 if (e > 1000 or np.isnan(e)) else e


def lambert(r, wo, wi, n):
    return np.broadcast_to(r / PI, wo.shape)


def oren_nayar(r, sigma_deg, wo, wi, n, b_term=True):
    """OrenNayar (core/reflection.h:264-271, core/reflection.cpp:132-156); sigma in degrees, already clamped by the material"""
    s2 = np.radians(sigma_deg) ** 2
    A, B = 1 - s2 / (2 * (s2 + .33)), (.45 * s2 / (s2 + .09) if b_term else 0.0)
    ci, co = _dot(wi, n), _dot(wo, n)
    si, so = np.sqrt(np.maximum(0, 1 - ci * ci)), np.sqrt(np.maximum(0, 1 - co * co))
    ti, to = wi - ci[..., None] * n, wo - co[..., None] * n
    with np.errstate(all="ignore"):
        dcos = np.where((si > 1e-4) & (so > 1e-4), _dot(ti, to) / (si * so), 0.0)
        maxcos = np.maximum(0, dcos)
        first = np.abs(ci) > np.abs(co)
        sinalpha = np.where(first, so, si)
        tanbeta = np.where(first, si / np.abs(ci), so / np.abs(co))
    return r / PI * (A + B * maxcos * sinalpha * tanbeta)[..., None]


def microfacet(r, exponent, fresnel, wo, wi, n, geometric=True, norm_add=2):
    """Microfacet::f with the Blinn distribution (core/reflection.cpp:163-175, core/reflection.h:293-301, :315-320);
    fresnel(cos) -> [..., 1 or 3]"""
    co, ci = np.abs(_dot(wo, n)), np.abs(_dot(wi, n))
    wh = _norm(wi + wo)
    ch = _dot(wi, wh)
    nh = np.abs(_dot(wh, n))
    with np.errstate(all="ignore"):
        D = (exponent + norm_add) / (2 * PI) * nh ** exponent
        woh = np.abs(_dot(wo, wh))
        G = np.minimum(1, np.minimum(2 * nh * co / woh, 2 * nh * ci / woh)) if geometric else 1.0
        f = r * (D * G / (4 * ci * co))[..., None] * fresnel(ch)
    return np.where(((ci == 0) | (co == 0))[..., None], 0.0, f)


class Material:
    """f(wo, wi) summed over the lobes the reference's material adds (materials/matte.cpp, plastic.cpp, uber.cpp, shinymetal.cpp,
    translucent.cpp), with BSDF::f's rule (core/reflection.cpp:480-494): the GEOMETRIC normal decides whether the reflection or the
    transmission lobes count.  A transmission lobe is BRDFToBTDF: the BRDF at wi mirrored into wo's hemisphere (reflection.cpp:63-66).
    Specular lobes (mirror, uber's, shinymetal's) do not answer f().  `twin` names a deliberately wrong variant (tests only)."""

    def __init__(self, kind, twin=None, **kw):
        self.kind, self.twin = kind, twin
        c = lambda k, d: np.clip(f32(kw.get(k, d)) * np.ones(3), 0, 1)          # Spectrum::Clamp()
        self.refl, self.trans = [], []
        dielectric = (lambda ch: fr_dielectric(ch, 1.5, 1.0)[..., None]) if twin != "fresnel_one" else (lambda ch: np.ones(ch.shape + (1,)))
        geo = twin != "no_geometric_term"
        nadd = 1 if twin == "blinn_normalised_by_e_plus_1" else 2
        if kind == "matte":
            kd, sig = c("Kd", 1), min(max(float(f32(kw.get("sigma", 0))), 0.0), 90.0)
            if twin == "sigma_unclamped":
                sig = float(f32(kw.get("sigma", 0)))
            self.refl.append((lambda wo, wi, n: lambert(kd, wo, wi, n)) if sig == 0 else (lambda wo, wi, n: oren_nayar(kd, sig, wo, wi, n, twin != "oren_nayar_without_b")))
        elif kind in ("plastic", "uber"):
            op = c("opacity", 1) if kind == "uber" else np.ones(3)
            if twin == "opacity_ignored":
                op = np.ones(3)
            kd, ks, e = op * c("Kd", 1), op * c("Ks", 1), blinn_exponent(kw.get("roughness", .1))
            if twin == "exponent_uncapped":
                e = 1.0 / float(f32(kw.get("roughness", .1)))
            if kd.any() or kind == "plastic":
                self.refl.append(lambda wo, wi, n: lambert(kd, wo, wi, n))
            if ks.any() or kind == "plastic":
                self.refl.append(lambda wo, wi, n: microfacet(ks, e, dielectric, wo, wi, n, geo, nadd))
        elif kind == "shinymetal":
            ks, e = c("Ks", 1), blinn_exponent(kw.get("roughness", .1))
            eta = approx_eta(ks) if twin != "eta_unclamped" else (1 + np.sqrt(np.minimum(ks, 1 - 1e-12))) / (1 - np.sqrt(np.minimum(ks, 1 - 1e-12)))
            fres = (lambda ch: fr_conductor(ch, eta)) if twin != "fresnel_one" else (lambda ch: np.ones(ch.shape + (1,)))
            self.refl.append(lambda wo, wi, n: microfacet(np.ones(3), e, fres, wo, wi, n, geo, nadd))
        elif kind == "translucent":
            kd, ks, r, t = c("Kd", 1), c("Ks", 1), c("reflect", .5), c("transmit", .5)
            if twin == "reflect_transmit_swapped":
                r, t = t, r
            e = blinn_exponent(kw.get("roughness", .1))
            if r.any() or t.any():
                if kd.any():
                    if r.any():
                        self.refl.append(lambda wo, wi, n: lambert(r * kd, wo, wi, n))
                    if t.any():
                        self.trans.append(lambda wo, wi, n: lambert(t * kd, wo, wi, n))
                if ks.any():
                    if r.any():
                        self.refl.append(lambda wo, wi, n: microfacet(r * ks, e, dielectric, wo, wi, n, geo, nadd))
                    if t.any():
                        self.trans.append(lambda wo, wi, n: microfacet(t * ks, e, dielectric, wo, wi, n, geo, nadd))
        elif kind == "mirror":
            self.kr = c("Kr", 1)
        elif kind == "glass":
            self.kr, self.kt, self.ior = c("Kr", 1), c("Kt", 1), float(f32(kw.get("index", 1.5)))
        else:
            raise ValueError(kind)

    def f(self, wo, wi, n):
        same = _dot(wi, n) * _dot(wo, n) > 0
        out = np.zeros(wo.shape)
        fr = sum((l(wo, wi, n) for l in self.refl), np.zeros(wo.shape))
        if self.trans:
            mirrored = wi - 2 * _dot(wi, n)[..., None] * n                       # otherHemisphere (core/reflection.h:151-153)
            ft = sum((l(wo, mirrored, n) for l in self.trans), np.zeros(wo.shape))
        else:
            ft = np.zeros(wo.shape)
        if self.twin == "normal_ignored":
            return fr
        out = np.where(same[..., None], fr, ft)
        return out


# ------------------------------------------------------------------------------------------------ medium
class Medium:
    """Volume "homogeneous" (volumes/homogeneous.cpp:63-67): tau over the part of a ray's [mint, maxt] inside the box p0..p1 (in volume
    space, core/volume.cpp's IntersectP through BBox::IntersectP) is its world length times sigma_a + sigma_s"""

    def __init__(self, p0, p1, sigma_a, sigma_s, v2w=None):
        self.p0, self.p1 = np.minimum(f32(p0), f32(p1)), np.maximum(f32(p0), f32(p1))
        self.sigma_t = f32(sigma_a) * np.ones(3) + f32(sigma_s) * np.ones(3)
        self.w2v = np.linalg.inv(np.eye(4) if v2w is None else v2w)

    def transmittance(self, o, d, mint, maxt):
        oo, od = xpoint(self.w2v, o), xvec(self.w2v, d)
        t0, t1 = np.broadcast_to(mint, oo.shape[:-1]).astype(np.float64), np.broadcast_to(maxt, oo.shape[:-1]).astype(np.float64)
        with np.errstate(all="ignore"):
            for a in range(3):
                inv = 1.0 / od[..., a]
                tn, tf = (self.p0[a] - oo[..., a]) * inv, (self.p1[a] - oo[..., a]) * inv
                tn, tf = np.minimum(tn, tf), np.maximum(tn, tf)
                t0, t1 = np.maximum(t0, np.where(np.isnan(tn), -np.inf, tn)), np.minimum(t1, np.where(np.isnan(tf), np.inf, tf))
        length = np.where(t1 > t0, (t1 - t0) * np.linalg.norm(d, axis=-1), 0.0)
        return np.exp(-length[..., None] * self.sigma_t)


# ------------------------------------------------------------------------------------------------ the integrator
class Scene:
    """surfaces: [(shape, Material)], lights: [Light], medium or None, maxdepth of SurfaceIntegrator "whitted".
    twin: a deliberately wrong variant of the whole form (tests only): "near_root_always", "shadow_unclipped", "falloff_cubed",
    "no_inverse_square", "no_cosine", "first_light_only", "mirror_unlit"."""

    def __init__(self, camera, surfaces, lights, medium=None, maxdepth=0, twin=None):
        self.camera, self.surfaces, self.lights, self.medium, self.maxdepth, self.twin = camera, surfaces, lights, medium, maxdepth, twin

    def closest(self, o, d, mint, maxt):
        """-> t, n, surface index (-1: none), root"""
        best = np.full(o.shape[:-1], np.inf)
        bn = np.zeros(o.shape)
        bi = np.full(o.shape[:-1], -1, np.int64)
        br = np.zeros(o.shape[:-1], np.int64)
        for i, (shape, _) in enumerate(self.surfaces):
            t, n, root = shape.intersect(o, d, mint, maxt)
            if self.twin == "near_root_always" and isinstance(shape, Quadric) and shape.kind != "disk":
                t = np.where(root == 1, np.inf, t)
            nearer = t < best
            best, bi, br = np.where(nearer, t, best), np.where(nearer, i, bi), np.where(nearer, root, br)
            bn = np.where(nearer[..., None], n, bn)
        return best, bn, bi, br

    def li(self, o, d, mint, maxt, depth=0):
        """Scene::Li (core/scene.cpp:120-126) with WhittedIntegrator::Li (integrators/whitted.cpp:44-140) and, with a medium, the
        "emission" volume integrator's transmittance (Le black).  -> L [.., 3], alpha, signature: an integer that names the discrete
        outcome of the sample (surface, root, per light: occluded / side of the normal / outside the spot's cone, and the same along
        the mirror path); two samples with equal signatures have no discontinuity between them."""
        shape = o.shape[:-1]
        t, n, idx, root = self.closest(o, d, mint, maxt)
        hit = idx >= 0
        L = np.zeros(o.shape)
        sig = (idx + 1) * 2 + root
        ts = np.where(hit, t, 0.0)
        p = o + ts[..., None] * d
        wo = -d
        for li_no, light in enumerate(self.lights):
            if self.twin == "first_light_only" and li_no > 0:
                break
            lcol, wi, end, zone = light.sample(p, exponent=3 if self.twin == "falloff_cubed" else 4)
            if self.twin == "no_inverse_square" and end is not None:
                lcol = np.broadcast_to(light.color, p.shape) * (lcol.sum(-1) > 0)[..., None]
            if end is not None:
                so, sd = p, end - p
                lo, hi = (0.0, 1.0) if self.twin == "shadow_unclipped" else (RAY_EPSILON, 1 - RAY_EPSILON)
            else:
                so, sd, lo, hi = p, wi, RAY_EPSILON, np.inf
            st, _, _, _ = self.closest(so, sd, lo, hi)
            occluded = np.isfinite(st) & hit
            side = (_dot(wi, n) > 0).astype(np.int64) * 2 + (_dot(wo, n) > 0).astype(np.int64)
            sig = (sig * 2 + occluded) * 4 + np.where(hit, side, 0)
            sig = sig * 2 + np.where(hit, zone == 0, 0)
            tr = 1.0
            if self.medium is not None:
                tr = self.medium.transmittance(so, sd, lo, hi)
            for m_no, (_, mat) in enumerate(self.surfaces):
                sel = hit & (idx == m_no) & ~occluded
                if mat.kind in ("mirror", "glass") or not sel.any():
                    continue
                with np.errstate(all="ignore"):
                    cos = 1.0 if self.twin == "no_cosine" else np.abs(_dot(wi, n))[..., None]
                    term = mat.f(wo, wi, n) * lcol * cos * tr
                L = np.where(sel[..., None], L + np.nan_to_num(term), L)
        if depth < self.maxdepth:
            for m_no, (_, mat) in enumerate(self.surfaces):
                sel = hit & (idx == m_no)
                if mat.kind not in ("mirror", "glass") or not sel.any():
                    continue
                cos_o = _dot(wo, n)
                # SpecularReflection::Sample_f (core/reflection.cpp:96-103): wi is wo mirrored about n, f = F Kr / |cos|, times |cos|;
                # the mirror's Fresnel is the no-op, glass's is FresnelDielectric(1, index) at cos(wo) (materials/glass.cpp)
                wi = -wo + 2 * cos_o[..., None] * n
                fr = np.ones(shape) if mat.kind == "mirror" else fr_dielectric(cos_o, 1.0, mat.ior)
                if self.twin == "glass_no_fresnel" and mat.kind == "glass":
                    fr = np.zeros(shape)
                ok = sel & (np.abs(_dot(wi, n)) > 0) & (fr > 0)
                if ok.any():
                    l2, _, s2 = self.li(p, wi, RAY_EPSILON, np.inf, depth + 1)
                    if self.twin == "mirror_unlit":
                        l2 = l2 * 0
                    L = np.where(ok[..., None], L + mat.kr * fr[..., None] * l2, L)
                    sig = np.where(ok, sig * 100003 + s2, sig)
                if mat.kind == "glass":
                    # SpecularTransmission::Sample_f (core/reflection.cpp:104-127): the side is the sign of cos(wo) against the SHADING normal,
                    # which for a triangle follows its winding; f |cos| = (et / ei)^2 (1 - F) Kt; nothing beyond total reflection
                    entering = cos_o > 0
                    ei, et = np.where(entering, 1.0, mat.ior), np.where(entering, mat.ior, 1.0)
                    eta = ei / et
                    sint2 = eta * eta * np.maximum(0, 1 - cos_o * cos_o)
                    cost = np.sqrt(np.maximum(0, 1 - sint2)) * np.where(entering, -1.0, 1.0)
                    wt = eta[..., None] * -(wo - cos_o[..., None] * n) + cost[..., None] * n
                    ok = sel & (sint2 < 1) & (np.abs(cost) > 0)
                    if ok.any():
                        l2, _, s2 = self.li(p, np.where(ok[..., None], wt, d), RAY_EPSILON, np.inf, depth + 1)
                        w = ((et * et) / (ei * ei) * (1 - fr))[..., None] * mat.kt
                        L = np.where(ok[..., None], L + w * l2, L)
                        sig = np.where(ok, sig * 1000003 + s2 + 1, sig)
                    sig = sig * 2 + (sel & (sint2 >= 1))
        if self.medium is not None:
            L = L * self.medium.transmittance(o, d, mint, np.where(hit, t, maxt))
        return np.where(hit[..., None], L, 0.0), hit.astype(np.float64), sig

    def samples(self, ix, iy):
        """radiance, alpha and signature of the camera samples at image positions (ix, iy)"""
        o, d, mint, maxt = self.camera.rays(ix, iy)
        return self.li(o, d, mint, maxt)


BAND_OFFSET = 0.02      # pixels


def band(scene, ix, iy):
    """The exclusion band, in float64 geometric terms only: a sample is left out when the scene's discrete outcome (Scene.li's signature:
    which surface and root the camera ray meets, and per light whether the shadow segment is blocked, on which side of the normal wi and
    wo lie (the terminator, the silhouette's far side) and whether the point is outside the spot's cone) differs at any of eight image
    positions BAND_OFFSET pixels away.  At a 60 degree field of view over 64 pixels that is 3e-4 rad of the camera ray, a few hundred
    times the float32 rounding of a ray direction; no error of any renderer enters."""
    ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
    _, _, s0 = scene.samples(ix, iy)
    out = np.zeros(ix.shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if dx or dy:
                _, _, s = scene.samples(ix + dx * BAND_OFFSET, iy + dy * BAND_OFFSET)
                out |= s != s0
    return out


def ray_band(scene, o, d, mint, maxt, angle=3e-4):
    """The band for given rays (the reference's own camera rays of a probe fixture): the closest hit's surface and root differ when the
    direction is turned by `angle` radians (what BAND_OFFSET pixels are at 60 degrees over 64 pixels) about the origin, in eight directions."""
    def sig(dd):
        t, _, idx, root = scene.closest(o, dd, mint, maxt)
        return (idx + 1) * 2 + root
    s0 = sig(d)
    a = _norm(np.cross(d, np.where(np.abs(d[..., :1]) < .6, [1.0, 0, 0], [0, 1.0, 0])))
    b = np.cross(_norm(d), a)
    out = np.zeros(s0.shape, bool)
    for ca in (-1, 0, 1):
        for cb in (-1, 0, 1):
            if ca or cb:
                out |= sig(d + angle * np.linalg.norm(d, axis=-1, keepdims=True) * (ca * a + cb * b)) != s0
    return out


def sample_error(got, L, included):
    """e = max_c |got - L| / (max_c |L| + 0.01 Lcase), Lcase the largest channel of L over the included samples"""
    lcase = float(np.abs(L[included]).max()) if included.any() else 0.0
    num, den = np.abs(np.asarray(got, np.float64) - L).max(-1), np.abs(L).max(-1) + 0.01 * lcase
    with np.errstate(all="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))
