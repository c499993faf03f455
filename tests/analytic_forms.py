"""Float64 closed forms of what one Whitted camera sample computes in a scene of a few analytic surfaces lit by delta lights: cameras,
ray / quad and ray / quadric intersection, point / spot / distant lights, the BSDFs of matte, plastic, uber, shinymetal and translucent
as the reference assembles them, the mirror step, the transmittance of a homogeneous medium and what the volume integrators "emission" and "single" estimate
by marching a homogeneous, exponential or volumegrid region (Medium: the exact integral and an allowance for the march's random offsets); and of what the hit itself carries: a
triangle mesh's barycentrics, (u, v), geometric and shading normal (Mesh), the quadrics' (u, v), the texture classes and 2-D mappings evaluated
at the hit (Texture, Mapping), materials resolved from them per sample (Textured) and the debug integrator's channels.  Plain numpy, vectorised over samples,
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


def _cross(a, b):
    """np.cross over the last axis, written out (broadcasting; several times faster on large blocks)"""
    ax, ay, az, bx, by, bz = a[..., 0], a[..., 1], a[..., 2], b[..., 0], b[..., 1], b[..., 2]
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], -1)


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
                if self.twin == "sphere_v_linear_in_z":
                    v = (z - self.zmin) / (self.zmax - self.zmin)
            elif self.kind == "disk":
                v = 1 - (np.hypot(p[..., 0], p[..., 1]) - self.inner) / (self.radius - self.inner)
            elif self.kind == "cone":
                v = z / (self.radius if self.twin == "cone_v_by_zmax_of_another_kind" else self.height)
            elif self.kind == "hyperboloid":
                v = (z - self.p1[2]) / (self.p2[2] - self.p1[2])
            else:
                v = (z - self.zmin) / (self.zmax - self.zmin)
            return self._phi(p) / (2 * PI if self.twin == "phimax_ignored_in_u" else self.phimax), v

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


class Mesh:
    """A `trianglemesh` with optional per-vertex uv, N, S under an object-to-world matrix (shapes/trianglemesh.cpp).  The vertices go to world
    space first (:167-168).  A hit has barycentrics (b0, b1, b2) and (u, v) = sum b_i uv_i (:270-272); without "uv" EVERY triangle has
    (0,0) (1,0) (1,1) (GetUVs, :315-328), so the inner diagonal of a two-triangle quad is a discontinuity of (u, v).  The geometric normal is
    Normalize(Cross(dpdu, dpdv)) (core/geometry DifferentialGeometry), the triangle's plane normal up to a sign that the (u, v) mapping decides.
    GetShadingGeometry (:71-133): with N, ns = Normalize(ObjectToWorld(sum b_i N_i)), a Normal, so under the inverse transpose; without N,
    ns is the geometric normal; ss = Normalize(ObjectToWorld(sum b_i S_i)) or Normalize(dpdu); ts = Normalize(Cross(ss, ns)), ss = Cross(ts, ns),
    and the shading normal is Normalize(Cross(ss, ts)) = ns whenever ss is not parallel to ns: S turns the frame, not the normal.  The
    barycentrics GetShadingGeometry solves from (u, v) are the hit's own while the triangle's uvs are not collinear.  ReverseOrientation and
    a mirroring transform flip signs only; every consumer here takes the line of the normal (the debug integrator's fabsf, BSDFs without glass).
    `twin`: a deliberately wrong variant (tests only)."""

    def __init__(self, P, indices, o2w=None, uv=None, N=None, S=None, twin=None):
        self.o2w = np.eye(4) if o2w is None else o2w
        self.twin = twin
        self.p = xpoint(self.o2w, f32(P).reshape(-1, 3))
        self.idx = np.asarray(indices, np.int64).reshape(-1, 3)
        self.uv = None if uv is None else f32(uv).reshape(-1, 2)
        self.N = None if N is None else f32(N).reshape(-1, 3)
        self.S = None if S is None else f32(S).reshape(-1, 3)
        self._memo = None
        self.sub_matters = self.uv is None or self.N is not None       # the triangle hit is a discrete outcome of the sample (band)
        if twin == "default_uvs_always":
            self.uv = None

    def _tri_uv(self, k):
        if self.uv is None:
            return np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])
        return self.uv[self.idx[k]]

    def full(self, o, d, mint, maxt):
        """-> dict(t (inf where missed), n, ns, u, v, tri)"""
        if self._memo is not None and self._memo[0] is o and self._memo[1] is d and self._memo[2] is mint and self._memo[3] is maxt:
            return self._memo[4]              # Scene.closest and Scene.details ask for the same rays
        key = (o, d, mint, maxt)
        shape = o.shape[:-1]
        o, d = np.broadcast_to(o, shape + (3,)).reshape(-1, 3), np.broadcast_to(d, shape + (3,)).reshape(-1, 3)
        mint, maxt = np.broadcast_to(mint, shape).reshape(-1, 1), np.broadcast_to(maxt, shape).reshape(-1, 1)
        p1 = self.p[self.idx[:, 0]]
        e1, e2 = self.p[self.idx[:, 1]] - p1, self.p[self.idx[:, 2]] - p1
        n_all = len(o)
        # only the rays whose line passes the vertices' bounding sphere (grown by a thousandth) can meet a triangle
        centre = (self.p.min(0) + self.p.max(0)) / 2
        near = np.linalg.norm(_cross(centre - o, _norm(d)), axis=-1) <= 1.001 * np.linalg.norm(self.p - centre, axis=1).max()
        o, d, mint, maxt = o[near], d[near], mint[near], maxt[near]
        best, tri, bb = np.full(len(o), np.inf), np.full(len(o), -1, np.int64), np.zeros((len(o), 3))
        for lo in range(0, len(o), 4096):                 # every ray against every triangle (:213-246), a block of rays at a time
            oo, dd = o[lo:lo + 4096, None, :], d[lo:lo + 4096, None, :]
            s1 = _cross(dd, e2)
            div = _dot(s1, e1)
            with np.errstate(all="ignore"):
                od = oo - p1
                b1 = _dot(od, s1) / div
                s2 = _cross(od, e1)
                b2 = _dot(dd, s2) / div
                t = _dot(s2, e2) / div
            ok = (div != 0) & (b1 >= 0) & (b1 <= 1) & (b2 >= 0) & (b1 + b2 <= 1) & (t >= mint[lo:lo + 4096]) & (t <= maxt[lo:lo + 4096])
            t = np.where(ok, t, np.inf)
            k = np.argmin(t, axis=1)
            rows = np.arange(len(k))
            hit = np.isfinite(t[rows, k])
            best[lo:lo + 4096] = t[rows, k]
            tri[lo:lo + 4096] = np.where(hit, k, -1)
            bb[lo:lo + 4096] = np.where(hit[:, None], np.stack([1 - b1[rows, k] - b2[rows, k], b1[rows, k], b2[rows, k]], -1), 0.0)

        def scatter(a, fill):
            out = np.full((n_all,) + a.shape[1:], fill, a.dtype)
            out[near] = a
            return out
        best, tri, bb = scatter(best, np.inf).reshape(shape), scatter(tri, -1).reshape(shape), scatter(bb, 0.0).reshape(shape + (3,))
        n, ns, u, v = np.zeros(shape + (3,)), np.zeros(shape + (3,)), np.zeros(shape), np.zeros(shape)
        for k in np.unique(tri[tri >= 0]):
            sel = tri == k
            i = self.idx[k]
            uv = self._tri_uv(k)
            du1, du2, dv1, dv2 = uv[0, 0] - uv[2, 0], uv[1, 0] - uv[2, 0], uv[0, 1] - uv[2, 1], uv[1, 1] - uv[2, 1]
            dp1, dp2 = self.p[i[0]] - self.p[i[2]], self.p[i[1]] - self.p[i[2]]
            det = du1 * dv2 - dv1 * du2
            assert det != 0, "a triangle with collinear uvs: the forms do not restate CoordinateSystem's fall-back"
            dpdu, dpdv = (dv2 * dp1 - dv1 * dp2) / det, (-du2 * dp1 + du1 * dp2) / det
            ng = _norm(np.cross(dpdu, dpdv))
            b = bb[sel]
            n[sel] = ng
            u[sel], v[sel] = b @ uv[:, 0], b @ uv[:, 1]
            if self.N is not None and self.twin != "geometric_for_shading_normal":
                nn = b @ self.N[i]
                nn = xvec(self.o2w, nn) if self.twin == "normal_transformed_as_vector" else xnormal(self.o2w, nn)
                ns[sel] = nn if self.twin == "normal_not_renormalised" else _norm(nn)
            else:
                ns[sel] = ng
        if self.twin == "u_v_swapped":
            u, v = v, u
        if self.twin == "shading_for_geometric_normal":
            n = ns
        self._memo = key + (dict(t=best, n=n, ns=ns, u=u, v=v, tri=tri),)
        return self._memo[4]

    def intersect(self, o, d, mint, maxt):
        h = self.full(o, d, mint, maxt)
        return h["t"], h["n"], np.zeros(h["t"].shape, np.int64)


# ------------------------------------------------------------------------------------------------ textures
class Mapping:
    """TextureMapping2D (core/texture.cpp:63-149): "uv": s = uscale u + udelta, t = vscale v + vdelta; "planar": s = udelta + p . v1,
    t = vdelta + p . v2 (world p); "spherical": with w = Normalize(WorldToTexture(p)), s = acos(w.z) / pi, t = phi / 2 pi, phi = atan2(w.y, w.x)
    in [0, 2 pi); "cylindrical": s = (pi + atan2(w.y, w.x)) / 2 pi, t = w.z.  WorldToTexture is the inverse of the CTM at the Texture statement.
    map() -> s, t, wrap: the coordinate that jumps by 1 across the mapping's seam (phi = 0; atan2 = +-pi), or None."""

    def __init__(self, kind="uv", t2w=None, twin=None, **kw):
        self.kind, self.twin = kind, twin
        g = lambda k, dflt: float(f32(kw.get(k, dflt)))
        self.su, self.sv, self.du, self.dv = g("uscale", 1), g("vscale", 1), g("udelta", 0), g("vdelta", 0)
        self.v1, self.v2 = f32(kw.get("v1", (1, 0, 0))), f32(kw.get("v2", (0, 1, 0)))
        if twin == "deltas_dropped" and kind == "planar":
            self.du = self.dv = 0.0
        self.w2t = np.linalg.inv(np.eye(4) if (t2w is None or twin == "texture_ctm_ignored") else t2w)

    def map(self, p, u, v):
        if self.kind == "uv":
            return self.su * u + self.du, self.sv * v + self.dv, None
        if self.kind == "planar":
            return self.du + _dot(p, self.v1), self.dv + _dot(p, self.v2), None
        w = _norm(xpoint(self.w2t, p))
        if self.kind == "spherical":
            phi = np.arctan2(w[..., 1], w[..., 0])
            t = np.where(phi < 0, phi + 2 * PI, phi) / (2 * PI)
            return np.arccos(np.clip(w[..., 2], -1, 1)) / PI, t, t
        if self.kind == "cylindrical":
            s = (PI + np.arctan2(w[..., 1], w[..., 0])) / (2 * PI)
            return s, w[..., 2], s
        raise ValueError(self.kind)


class Texture:
    """The texture classes (textures/constant.cpp, scale.cpp, mix.cpp, bilerp.cpp, uv.cpp, checkerboard.cpp with aamode "none", dimension 2).
    A float texture travels as (f, f, f).  kind "constant": value; "scale": tex1 * tex2; "mix": (1 - amount) tex1 + amount tex2; "bilerp":
    (1-s)(1-t) v00 + (1-s) t v01 + s (1-t) v10 + s t v11; "uv": (s - floor s, t - floor t, 0); "checkerboard": tex1 where
    floor s + floor t is even, else tex2.  Children (tex1, tex2, amount) are Textures.  `twin`: a deliberately wrong variant (tests only)."""

    def __init__(self, kind, mapping=None, twin=None, **kw):
        self.kind, self.mapping, self.twin, self.kw = kind, mapping, twin, kw
        if kind == "bilerp":
            self.corners = [f32(kw[k]) * np.ones(3) for k in ("v00", "v01", "v10", "v11")]
            if twin == "corners_transposed":
                self.corners[1], self.corners[2] = self.corners[2], self.corners[1]
        if kind == "constant":
            self.value = f32(kw["value"]) * np.ones(3)

    def eval(self, p, u, v, trace):
        """-> value [..., 3]; appends to trace["cells"] the integer cell of every checkerboard / uv node evaluated and to trace["wraps"] the
        seam coordinate of every spherical / cylindrical mapping evaluated (the discrete outcomes the band needs)"""
        k = self.kind
        if k == "constant":
            return np.broadcast_to(self.value, p.shape)
        if k in ("scale", "mix"):
            a, b = self.kw["tex1"].eval(p, u, v, trace), self.kw["tex2"].eval(p, u, v, trace)
            if k == "scale":
                return a + b if self.twin == "scale_adds" else a * b
            amt = self.kw["amount"].eval(p, u, v, trace)
            if self.twin == "amount_complemented":
                amt = 1 - amt
            if self.twin == "tex1_tex2_swapped":
                a, b = b, a
            return (1 - amt) * a + amt * b
        s, t, wrap = self.mapping.map(p, u, v)
        if wrap is not None:
            trace["wraps"].append(wrap)
        if k == "bilerp":
            s, t = s[..., None], t[..., None]
            c = self.corners
            return (1 - s) * (1 - t) * c[0] + (1 - s) * t * c[1] + s * (1 - t) * c[2] + s * t * c[3]
        fl = np.trunc if self.twin == "cells_truncated_toward_zero" else np.floor
        cs, ct = fl(s).astype(np.int64), fl(t).astype(np.int64)
        trace["cells"].append(cs * 4099 + ct)
        if k == "uv":
            if self.twin == "fraction_not_taken":
                cs, ct = 0, 0
            return np.stack([s - cs, t - ct, np.zeros_like(s)], -1)
        if k == "checkerboard":
            a, b = self.kw["tex1"].eval(p, u, v, trace), self.kw["tex2"].eval(p, u, v, trace)
            return np.where((((cs + ct) % 2) == 0)[..., None], a, b)
        raise ValueError(k)


class Textured:
    """A material whose parameters may be Textures: resolve() evaluates them at the hit (p, u, v) and hands the per-sample arrays to Material
    (a float parameter takes the first channel)."""
    FLOATS = ("sigma", "roughness", "index")

    def __init__(self, kind, twin=None, **kw):
        self.kind, self.twin, self.kw = kind, twin, kw

    def resolve(self, p, u, v, trace):
        vals = {}
        for k, x in self.kw.items():
            if isinstance(x, Texture):
                x = x.eval(p, u, v, trace)
                x = x[..., 0] if k in self.FLOATS else x
            vals[k] = x
        return Material(self.kind, twin=self.twin, **vals)


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
    if isinstance(roughness, np.ndarray) and roughness.ndim:       # per sample, from a texture
        with np.errstate(divide="ignore", invalid="ignore"):
            e = 1.0 / roughness
        return np.where((e > 1000) | np.isnan(e), 1000.0, e)
    with np.errstate(divide="ignore"):
        e = 1.0 / float(f32(roughness))
    return 1000.0 if (e > 1000 or np.isnan(e)) else e


def _param(x):
    """a material parameter: a literal of the scene file (float32) or, from a texture, a float64 array over the samples"""
    return x if isinstance(x, np.ndarray) and x.dtype == np.float64 and x.ndim else f32(x)


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
        # Spectrum::Clamp(): at 0 below, unbounded above (core/color.h:161)
        c = (lambda k, d: _param(kw.get(k, d)) * np.ones(3)) if twin == "kd_unclamped" else (lambda k, d: np.maximum(_param(kw.get(k, d)) * np.ones(3), 0))
        per_sample = any(isinstance(x, np.ndarray) and x.ndim for x in kw.values())          # a parameter evaluated from a texture
        self.refl, self.trans = [], []
        dielectric = (lambda ch: fr_dielectric(ch, 1.5, 1.0)[..., None]) if twin != "fresnel_one" else (lambda ch: np.ones(ch.shape + (1,)))
        geo = twin != "no_geometric_term"
        nadd = 1 if twin == "blinn_normalised_by_e_plus_1" else 2
        if kind == "matte":
            kd = self.kd = c("Kd", 1)
            if per_sample:
                # Oren-Nayar at sigma = 0 has A = 1, B = 0: the Lambert branch (materials/matte.cpp:58-61) is the same function there
                sg = _param(kw.get("sigma", 0)) * np.ones(kd.shape[:-1])
                sig = sg if twin == "sigma_unclamped" else np.clip(sg, 0.0, 90.0)
                self.refl.append(lambda wo, wi, n: oren_nayar(kd, sig, wo, wi, n, twin != "oren_nayar_without_b"))
                return
            sig = min(max(float(f32(kw.get("sigma", 0))), 0.0), 90.0)
            if twin == "sigma_unclamped":
                sig = float(f32(kw.get("sigma", 0)))
            self.refl.append((lambda wo, wi, n: lambert(kd, wo, wi, n)) if sig == 0 else (lambda wo, wi, n: oren_nayar(kd, sig, wo, wi, n, twin != "oren_nayar_without_b")))
        elif kind in ("plastic", "uber"):
            op = c("opacity", 1) if kind == "uber" else np.ones(3)
            if twin == "opacity_ignored":
                op = np.ones(3)
            kd, ks, e = op * c("Kd", 1), op * c("Ks", 1), blinn_exponent(kw.get("roughness", .1))
            if twin == "exponent_uncapped":
                e = 1.0 / _param(kw.get("roughness", .1))
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
    space, core/volume.cpp's IntersectP through BBox::IntersectP) is its world length times sigma_a + sigma_s.

    With Le, single scattering or a density (kinds "exponential", "volumegrid") the region is one that the volume integrator MARCHES with
    random offsets.  The float64 side then states the exact integrals (depth(), lv()) and, beside them, an allowance that bounds what any
    offset can do (interval(), lv()); it never replays a draw.  Lengths s along a ray are world lengths along its unit direction."""

    def __init__(self, p0, p1, sigma_a, sigma_s, v2w=None, kind="homogeneous", Le=(0, 0, 0), g=0.0, a=1.0, b=1.0, updir=(0, 1, 0),
                 nx=1, ny=1, nz=1, values=None, integrator="emission", stepsize=1.0, twin=None):
        """kind "exponential" (volumes/exponential.cpp) and "volumegrid" (volumes/volumegrid.cpp) are DensityRegions (core/volume.h:62-90):
        sigma_a, sigma_s and Le are scaled by Density(WorldToVolume(p)).  v2w: the CTM at the Volume statement.  integrator, stepsize: the
        VolumeIntegrator ("emission", integrators/emission.cpp; "single", integrators/single.cpp).  twin: a deliberately wrong variant (tests only)."""
        self.p0, self.p1 = np.minimum(f32(p0), f32(p1)), np.maximum(f32(p0), f32(p1))
        self.sigma_s = f32(sigma_s) * np.ones(3)
        self.sigma_t = f32(sigma_a) * np.ones(3) + f32(sigma_s) * np.ones(3)
        self.w2v = np.linalg.inv(np.eye(4) if (v2w is None or twin == "volume_ctm_ignored") else v2w)
        self.kind, self.twin, self.integrator, self.step = kind, twin, integrator, float(f32(stepsize))
        self.le, self.g = f32(Le) * np.ones(3), float(f32(g)) * (-1.0 if twin == "phase_g_sign_flipped" else 1.0)
        self.a, self.b = float(f32(a)), float(f32(b))
        self.up = f32(updir) if twin == "updir_unnormalised" else _norm(f32(updir))            # exponential.cpp:33
        self.n = np.array([int(nx), int(ny), int(nz)])
        self.values = None if values is None else f32(values).ravel()
        # a region that the float64 side integrates along the ray and that carries an allowance (Scene.allowance); the homogeneous box under
        # "emission" with Le black is the closed form below and has none
        self.marches = kind != "homogeneous" or integrator == "single" or bool(self.le.any())

    # ---- the region along a ray ----------------------------------------------------------------------------------------------------
    def clip(self, o, d, lo, hi):
        """-> the unit direction and the part [s0, s1] of o + s dn, s a WORLD length, inside the extent (DensityRegion::Tau normalises the
        direction and scales mint and maxt, core/volume.cpp:145-150; IntersectP takes the ray to volume space, where s is still the parameter),
        and whether there is such a part.  Where there is none s0 = s1 = 0."""
        length = np.linalg.norm(d, axis=-1)
        dn = d / length[..., None]
        oo, od = xpoint(self.w2v, o), xvec(self.w2v, dn)
        t0, t1 = np.broadcast_to(lo, length.shape) * length, np.broadcast_to(hi, length.shape) * length
        with np.errstate(all="ignore"):
            for a in range(3):
                inv = 1.0 / od[..., a]
                tn, tf = (self.p0[a] - oo[..., a]) * inv, (self.p1[a] - oo[..., a]) * inv
                tn, tf = np.minimum(tn, tf), np.maximum(tn, tf)
                t0, t1 = np.maximum(t0, np.where(np.isnan(tn), -np.inf, tn)), np.minimum(t1, np.where(np.isnan(tf), np.inf, tf))
            ok = np.isfinite(t0) & np.isfinite(t1) & (t1 > t0)
        return dn, np.where(ok, t0, 0.0), np.where(ok, t1, 0.0), ok

    def density(self, p):
        """Density(WorldToVolume(p)) at points of a clipped segment (so the extent's Inside test, which only rounding could fail there, is left out)"""
        q = xpoint(self.w2v, p)
        if self.kind == "homogeneous":
            return np.ones(q.shape[:-1])
        if self.kind == "exponential":                                                         # exponential.cpp:40-44
            rel = q if self.twin == "height_from_origin" else q - self.p0
            return self.a * np.exp(-self.b * _dot(rel, self.up))
        # volumegrid.cpp:64-84: voxel centres at (i + .5) / n, Floor2Int, indices clamped, density[z nx ny + y nx + x], lerps along x, then y, then z
        nx, ny, nz = self.n
        vox = (q - self.p0) / (self.p1 - self.p0) * self.n - (0.0 if self.twin == "voxel_centres_at_corners" else 0.5)
        v = np.floor(vox)
        dx, dy, dz = (vox - v)[..., 0], (vox - v)[..., 1], (vox - v)[..., 2]
        v = v.astype(np.int64)

        def D(ax, ay, az):
            x, y, z = np.clip(v[..., 0] + ax, 0, nx - 1), np.clip(v[..., 1] + ay, 0, ny - 1), np.clip(v[..., 2] + az, 0, nz - 1)
            return self.values[(x * ny * nz + y * nz + z) if self.twin == "grid_axes_transposed" else (z * nx * ny + y * nx + x)]
        lerp = lambda t, a, b: (1 - t) * a + t * b
        d00, d10 = lerp(dx, D(0, 0, 0), D(1, 0, 0)), lerp(dx, D(0, 1, 0), D(1, 1, 0))
        d01, d11 = lerp(dx, D(0, 0, 1), D(1, 0, 1)), lerp(dx, D(0, 1, 1), D(1, 1, 1))
        return lerp(dz, lerp(dy, d00, d10), lerp(dy, d01, d11))

    def density_bounds(self):
        """(max f, a bound of the total variation of f along ANY straight segment inside the extent), f = Density: crude and global, for the thin
        regions where they enter at second order.  An exponential is monotone along a line: TV <= max - min over the box.  A line crosses at most
        nx + ny + nz + 1 cells of the grid, and inside a cell the trilinear value stays between its corners'."""
        if self.kind == "homogeneous":
            return 1.0, 0.0
        if self.kind == "exponential":
            c = np.array([[x, y, z] for x in (self.p0[0], self.p1[0]) for y in (self.p0[1], self.p1[1]) for z in (self.p0[2], self.p1[2])])
            f = self.a * np.exp(-self.b * _dot(c if self.twin == "height_from_origin" else c - self.p0, self.up))
            return float(f.max()), float(f.max() - f.min())
        return float(self.values.max()), float((self.n.sum() + 1) * (self.values.max() - self.values.min()))

    PIECES = 32

    def nodes(self, o, dn, s0, s1, q, pieces=True):
        """Quadrature along the clipped segment: it is cut into pieces on which the integrand is smooth (a volumegrid: at every plane through
        voxel centres, between which the trilinear density is a cubic of s; otherwise PIECES equal parts), and each piece gets the q Gauss-Legendre
        nodes.  -> s [.., K] in ascending order, the piece ends included (with weight 0: they serve the total variation), and the weights."""
        if self.kind == "volumegrid" and pieces:
            oo, od = xpoint(self.w2v, o), xvec(self.w2v, dn)
            cuts = [s0[..., None], s1[..., None]]
            off = 0.0 if self.twin == "voxel_centres_at_corners" else 0.5
            for a in range(3):
                c = self.p0[a] + (np.arange(self.n[a]) + off) / self.n[a] * (self.p1[a] - self.p0[a])
                with np.errstate(all="ignore"):
                    s = (c - oo[..., a, None]) / od[..., a, None]
                cuts.append(np.clip(np.where(np.isfinite(s), s, 0.0), s0[..., None], s1[..., None]))
            B = np.sort(np.concatenate(cuts, -1), -1)
        elif pieces:
            B = s0[..., None] + (s1 - s0)[..., None] * np.linspace(0.0, 1.0, self.PIECES + 1)
        else:
            B = np.stack([s0, s1], -1)
        x, w = np.polynomial.legendre.leggauss(q)
        lo, hi = B[..., :-1], B[..., 1:]
        mid, half = (lo + hi) / 2, (hi - lo) / 2
        s = np.concatenate([lo[..., None], mid[..., None] + half[..., None] * x], -1).reshape(lo.shape[:-1] + (-1,))
        ww = np.concatenate([np.zeros(lo.shape + (1,)), half[..., None] * w], -1).reshape(s.shape)
        return np.concatenate([s, B[..., -1:]], -1), np.concatenate([ww, np.zeros(s.shape[:-1] + (1,))], -1)

    def depth(self, o, d, lo, hi, q=3, pieces=True):
        """of f = Density along the part of the ray inside the extent: the exact integral (a cubic per piece under 3 nodes; an exponential to
        1e-12 on PIECES parts), its total variation over the nodes and piece ends, its maximum.  Times sigma_t this is tau."""
        dn, s0, s1, ok = self.clip(o, d, lo, hi)
        s, w = self.nodes(o, dn, s0, s1, q, pieces)
        f = self.density(o[..., None, :] + s[..., None] * dn[..., None, :]) * ok[..., None]
        return (w * f).sum(-1), np.abs(np.diff(f, axis=-1)).sum(-1), f.max(-1)

    def interval(self, o, d, lo, hi, h):
        """Transmittance over [lo, hi] of the ray as Tau computes it with step h and ANY offset u in [0, 1) (core/volume.cpp:139-157): samples of
        f every h from s0 + u h while s < s1.  Cell k holds sample k and the last cell overhangs s1 by at most h, so the sum differs from the
        integral by at most h (TV(f; [s0, s1]) + max f).  -> exp(-tau), tau, that bound of tau (per channel).  A homogeneous region's Tau is
        its length times sigma_t whatever u (volumes/homogeneous.cpp:63-67)."""
        tau, tv, fmax = self.depth(o, d, lo, hi)
        dd = 0.0 * tau if self.kind == "homogeneous" else h * (tv + fmax)
        return np.exp(-tau[..., None] * self.sigma_t), tau[..., None] * self.sigma_t, dd[..., None] * self.sigma_t

    # ---- VolumeIntegrator::Li ------------------------------------------------------------------------------------------------------------
    def phase(self, cos):
        """PhaseHG(w, wp, g) (core/volume.cpp:44-49) at cos = Dot(w, wp).  The integrators call p(p, -ray.d, -wi) (single.cpp:107), so cos is
        Dot(ray.d, wi): g > 0 favours light that keeps its direction on the way to the camera."""
        g = self.g
        return (1 - g * g) / (4 * PI * (1 + g * g - 2 * g * cos) ** 1.5)

    def lv(self, o, d, lo, hi, light):
        """The exact value of what EmissionIntegrator::Li / SingleScattering::Li estimate along the camera ray (emission.cpp:61-95, single.cpp:56-116),
        the integral over the part [s0, s1] inside the extent of
            g(s) = Tr(s) (Lve(s) + sigma_s(s) PhaseHG(Dot(ray.d, wi)) L_light(s) T_shadow(s)),
        and the allowance: the march puts ONE sample into each of N = ceil((s1 - s0) / stepsize) cells that tile [s0, s1] exactly, at the same
        offset in each, so its sum differs from the integral by at most step TV(g).  In a density region the march's Tr is a product of per-step Taus
        at .5 stepsize and T_shadow a Tau at 4 stepsize: with every tau within dc (ds) of the integral, each term is within a factor
        exp(+-(dc + ds)) of g.  -> Lv, D, the lower end of Tr at s1 (the roulette's quantity)."""
        shape = o.shape[:-1]
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        lo, hi = np.broadcast_to(lo, shape).reshape(-1), np.broadcast_to(hi, shape).reshape(-1)
        Lv, Dv, trlow = np.zeros((len(o), 3)), np.zeros((len(o), 3)), np.ones((len(o), 3))
        single = self.integrator == "single" and light is not None and bool(self.sigma_s.any())
        fmax, tvmax = self.density_bounds()
        for b0 in range(0, len(o), 2048):                      # a block of rays at a time (the nodes of a block: a few hundred thousand points)
            sl = slice(b0, b0 + 2048)
            dn, s0, s1, ok = self.clip(o[sl], d[sl], lo[sl], hi[sl])
            s, w = self.nodes(o[sl], dn, s0, s1, 4)
            p = o[sl, None, :] + s[..., None] * dn[:, None, :]
            dens = self.density(p)
            if self.kind == "homogeneous":
                cum = s - s0[:, None]
            else:             # the depth up to each node by the trapezoid rule over the nodes: the regions marched here are thin (tau of order .01)
                cum = np.concatenate([np.zeros((len(s), 1)), np.cumsum((dens[:, 1:] + dens[:, :-1]) / 2 * np.diff(s, axis=-1), -1)], -1)
            tr = np.exp(-cum[..., None] * self.sigma_t)
            g = (1.0 if self.twin == "emission_unattenuated" else tr) * dens[..., None] * self.le
            if single:
                li, wi, pos, _ = light.sample(p)
                tau_s = self.depth(p, pos - p, RAY_EPSILON, 1 - RAY_EPSILON, q=6 if self.kind == "volumegrid" else 3, pieces=self.kind == "exponential")[0]
                tsh = 1.0 if self.twin == "shadow_transmittance_dropped" else np.exp(-tau_s[..., None] * self.sigma_t)
                ss = self.sigma_s * (1.0 if self.twin == "sigma_s_not_scaled_by_density" else dens[..., None])
                g = g + tr * ss * self.phase(_dot(dn[:, None, :], wi))[..., None] * li * tsh
            g = g * ok[:, None, None]
            n = np.maximum(np.ceil((s1 - s0) / self.step), 1.0)
            step = ((s1 - s0) / n)[:, None]
            integral, tv = (w[..., None] * g).sum(-2), np.abs(np.diff(g, axis=-2)).sum(-2)
            # float32: where the segment ends ON the extent (not at the ray's own mint or at the surface hit), a first sample at u near 0 or a last
            # one at u near 1 lies within rounding of that face, and Inside() of the rounded point may answer no: Density, sigma_s and Lve are 0 there
            # and the cell's term is lost.  One end at most for a given u.
            length = np.linalg.norm(d[sl], axis=-1)
            on_face0, on_face1 = (s0 > lo[sl] * length)[:, None], (s1 < hi[sl] * length)[:, None]
            dev = step * (tv + np.maximum(g[:, 0] * on_face0, g[:, -1] * on_face1))
            dc = 0.0
            if self.kind != "homogeneous":
                # every step's Tau at .5 stepsize: (h / 2) (TV over the step + max f) each; the overhangs add up over the n steps and the start
                dc = 0.5 * self.step * (tvmax + (n[:, None] + 1) * fmax) * self.sigma_t
                ds = (4 * self.step * (tvmax + fmax) * self.sigma_t) if single else 0.0
                dev = dev + np.expm1(dc + ds) * (integral + dev)
            Lv[sl], Dv[sl] = integral, dev
            trlow[sl] = np.exp(-(cum[:, -1, None] * self.sigma_t + dc))
        return Lv.reshape(shape + (3,)), Dv.reshape(shape + (3,)), trlow.reshape(shape + (3,))

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
    A surface's material may be a Textured: it is resolved at every hit, on every recursion level.
    twin: a deliberately wrong variant of the whole form (tests only): "near_root_always", "shadow_unclipped", "falloff_cubed",
    "no_inverse_square", "no_cosine", "first_light_only", "mirror_unlit", "wall_material_at_the_floor"."""

    def __init__(self, camera, surfaces, lights, medium=None, maxdepth=0, twin=None, debug=None):
        """debug: the channel triple of SurfaceIntegrator "debug" (u v nx ny nz snx sny snz one zero hit), or None for "whitted" """
        self.camera, self.surfaces, self.lights, self.medium, self.maxdepth, self.twin = camera, surfaces, lights, medium, maxdepth, twin
        self.debug = debug
        self.trace = dict(cells=[], wraps=[])
        self.mats = {}
        self.sig_only = False          # band(): only the signature is read, so a march's integral is left out
        self.D = None                  # the allowance of the last li() (zero without a marched medium)

    def details(self, o, d, mint, maxt, idx):
        """(u, v), the shading normal and the sub-outcome (the triangle, where it decides a value) of the closest hits: a mesh's from
        Mesh.full, a quadric's own parametrisation with the shading normal its geometric one, a Quad's left at 0 (its cases read neither)"""
        shape = o.shape[:-1]
        u, v, ns, sub = np.zeros(shape), np.zeros(shape), np.zeros(shape + (3,)), np.zeros(shape, np.int64)
        for i, (shp, _) in enumerate(self.surfaces):
            sel = idx == i
            if not sel.any():
                continue
            if isinstance(shp, Mesh):
                h = shp.full(o, d, mint, maxt)
                u, v, ns = np.where(sel, h["u"], u), np.where(sel, h["v"], v), np.where(sel[..., None], h["ns"], ns)
                if shp.sub_matters:
                    sub = np.where(sel, h["tri"] + 1, sub)
            else:
                t, n, _ = shp.intersect(o, d, mint, maxt)
                ns = np.where(sel[..., None], n, ns)
                if isinstance(shp, Quadric):
                    qu, qv = shp.uv(o + np.where(sel, t, 0.0)[..., None] * d)
                    u, v = np.where(sel, qu, u), np.where(sel, qv, v)
        return u, v, ns, sub

    def debug_li(self, o, d, mint, maxt):
        """DebugIntegrator::Li (integrators/debug.cpp:61-133): per channel u, v, |ng|, |ns| of the camera ray's hit (0 on a miss), the
        constants, the hit mask; alpha is 1 for every sample (:69), misses included"""
        t, n, idx, root = self.closest(o, d, mint, maxt)
        hit = idx >= 0
        u, v, ns, sub = self.details(o, d, mint, maxt, idx)
        one = np.ones(hit.shape)
        val = dict(u=u, v=v, nx=np.abs(n[..., 0]), ny=np.abs(n[..., 1]), nz=np.abs(n[..., 2]), snx=np.abs(ns[..., 0]), sny=np.abs(ns[..., 1]),
                   snz=np.abs(ns[..., 2]), one=one, zero=0 * one, hit=one)
        L = np.stack([val[c] if c == "one" else np.where(hit, val[c], 0.0) for c in self.debug], -1)
        return L, one, ((idx + 1) * 2 + root) * 100003 + sub

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
        surfaces = self.surfaces
        if any(isinstance(m, Textured) for _, m in surfaces):
            # the materials resolved at this hit; every integer cell a texture took is part of the sample's discrete outcome
            u, v, _, sub = self.details(o, d, mint, maxt, idx)
            surfaces = []
            for m_no, (shp, m) in enumerate(self.surfaces):
                if isinstance(m, Textured):
                    tr = dict(cells=[], wraps=[])
                    m = m.resolve(p, u, v, tr)
                    sel = hit & (idx == m_no)
                    for c in tr["cells"]:
                        sig = sig * 8191 + np.where(sel, c, 0)
                    self.trace["wraps"] += [np.where(sel, w, 0.0) for w in tr["wraps"]]
                surfaces.append((shp, m))
            sig = sig * 1031 + sub
        self.mats[depth] = [m for _, m in surfaces]
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
            if self.medium is not None and self.medium.marches:
                # VisibilityTester::Transmittance has no Sample: Tau at 4 x stepsize from a draw (emission.cpp:54-57, single.cpp:49-52)
                tr, tau_s, dd_s = self.medium.interval(so, sd, lo, hi, 4 * self.medium.step)
            elif self.medium is not None:
                tr = self.medium.transmittance(so, sd, lo, hi)
            for m_no, (_, mat) in enumerate(surfaces):
                sel = hit & (idx == m_no) & ~occluded
                if mat.kind in ("mirror", "glass") or not sel.any():
                    continue
                with np.errstate(all="ignore"):
                    cos = 1.0 if self.twin == "no_cosine" else np.abs(_dot(wi, n))[..., None]
                    term = mat.f(wo, wi, n) * lcol * cos * tr
                L = np.where(sel[..., None], L + np.nan_to_num(term), L)
        if depth < self.maxdepth:
            for m_no, (_, mat) in enumerate(surfaces):
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
                    kr = mat.kr
                    if self.twin == "wall_material_at_the_floor":     # the record of the reflected ray's hit read where the mirror's own is due
                        kr = next(m.kd for m in self.mats[depth + 1] if m.kind == "matte")
                    L = np.where(ok[..., None], L + kr * fr[..., None] * l2, L)
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
        self.D = np.zeros(o.shape)
        if self.medium is not None and self.medium.marches:
            # Scene::Li (core/scene.cpp:120-126): T Lo + Lv, alpha the surface integrator's alone: a camera ray that hits nothing carries Lv at alpha 0
            self.march_conditions(depth)
            end = np.where(hit, t, maxt)
            tc, tau_c, dd_c = self.medium.interval(o, d, mint, end, self.medium.step)
            S = np.where(hit[..., None], L * tc, 0.0)
            # the intervals T in [exp(-(tau + d)), exp(-max(tau - d, 0))] of the camera and the shadow segment, through the product
            up, low = np.exp(np.minimum(dd_c, tau_c) + np.minimum(dd_s, tau_s)), np.exp(-(dd_c + dd_s))
            self.D = S * np.maximum(up - 1, 1 - low)
            if self.sig_only:
                return S, hit.astype(np.float64), sig
            Lv, Dv, trlow = self.medium.lv(o, d, mint, end, self.lights[0])
            # no roulette draw: the march's lowest possible Tr.y() stays at or above 0.01 wherever the march adds anything (emission.cpp:84-88)
            y = trlow @ np.array([0.212671, 0.715160, 0.072169])
            assert (y[(Lv > 0).any(-1)] >= 0.01).all(), "a march of this scene could reach the Russian roulette"
            self.D = self.D + Dv
            return S + Lv, hit.astype(np.float64), sig
        if self.medium is not None:
            L = L * self.medium.transmittance(o, d, mint, np.where(hit, t, maxt))
        return np.where(hit[..., None], L, 0.0), hit.astype(np.float64), sig

    def march_conditions(self, depth):
        """What keeps every draw but the offsets out of a march (conditions on the float64 scene, not measurements): Scene::Li is not entered from a
        recursion; one delta light (lightNum is 0, pdf is 1, u1 and u2 unused) that lies outside the region (1 / d^2 stays bounded along every ray);
        every surface in y <= 0, the region and the light in y >= 0, so that no shadow segment from a point of the region is occluded."""
        m = self.medium
        assert depth == 0 and self.maxdepth == 0 and len(self.lights) == 1 and self.lights[0].kind in ("point", "spot")
        q = xpoint(m.w2v, self.lights[0].pos)
        assert not ((q >= m.p0) & (q <= m.p1)).all(), "the light lies inside the region"
        corners = np.array([[x, y, z] for x in (m.p0[0], m.p1[0]) for y in (m.p0[1], m.p1[1]) for z in (m.p0[2], m.p1[2])])
        assert xpoint(np.linalg.inv(m.w2v), corners)[:, 1].min() >= 0 and self.lights[0].pos[1] > 0
        assert all(isinstance(shp, Quad) and shp.p[:, 1].max() <= 0 for shp, _ in self.surfaces)

    def allowance(self, ix, iy):
        """-> L, D, alpha, signature: the radiance as samples() gives it and beside it the per-sample, per-channel allowance D >= 0, which
        bounds what ANY choice of the draws that enter a march (the scatter offset, every Tau's offset) can move the renderer's value away from L;
        derived from the float64 scene alone (Medium.interval, Medium.lv).  Zero for a scene without a marched medium."""
        L, alpha, sig = self.samples(ix, iy)
        return L, self.D, alpha, sig

    def samples(self, ix, iy):
        """radiance, alpha and signature of the camera samples at image positions (ix, iy)"""
        o, d, mint, maxt = self.camera.rays(ix, iy)
        self.trace = dict(cells=[], wraps=[])       # wraps: the seam coordinates met by this call (read by band())
        if self.debug:
            return self.debug_li(o, d, mint, maxt)
        return self.li(o, d, mint, maxt)


BAND_OFFSET = 0.02      # pixels


def band(scene, ix, iy):
    """The exclusion band, in float64 geometric terms only: a sample is left out when the scene's discrete outcome (Scene.li's signature:
    which surface and root the camera ray meets, and per light whether the shadow segment is blocked, on which side of the normal wi and
    wo lie (the terminator, the silhouette's far side) and whether the point is outside the spot's cone; the integer cell of every
    checkerboard and uv texture evaluated; the triangle hit where a mesh has no uvs or has N) differs, or the seam coordinate of a spherical
    or cylindrical mapping jumps (Scene.trace["wraps"]: phi = 0, atan2 = +-pi), at any of eight image
    positions BAND_OFFSET pixels away.  At a 60 degree field of view over 64 pixels that is 3e-4 rad of the camera ray, a few hundred
    times the float32 rounding of a ray direction; no error of any renderer enters."""
    ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
    scene.sig_only = True
    _, _, s0 = scene.samples(ix, iy)
    w0 = scene.trace["wraps"]
    out = np.zeros(ix.shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if dx or dy:
                _, _, s = scene.samples(ix + dx * BAND_OFFSET, iy + dy * BAND_OFFSET)
                out |= s != s0
                for a, b in zip(scene.trace["wraps"], w0):       # across a mapping's seam the coordinate jumps by 1
                    out |= np.abs(a - b) > 0.5
    scene.sig_only = False
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


def sample_scale(L, included):
    """max_c |L| + 0.01 Lcase, Lcase the largest channel of L over the included samples"""
    lcase = float(np.abs(L[included]).max()) if included.any() else 0.0
    return np.abs(L).max(-1) + 0.01 * lcase


def sample_error(got, L, included, D=None):
    """e = max_c |got - L| / (max_c |L| + 0.01 Lcase), Lcase the largest channel of L over the included samples; with an allowance D
    (Scene.allowance) the excess e' = max_c max(0, |got - L| - D) over the same scale"""
    num, den = np.abs(np.asarray(got, np.float64) - L), sample_scale(L, included)
    num = (num if D is None else np.maximum(0.0, num - D)).max(-1)
    with np.errstate(all="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))
