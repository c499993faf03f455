"""Float64 forms of the four BSDF queries an integrator makes of a hit -- BSDF::f, BSDF::Pdf, BSDF::Sample_f and BSDF::NumComponents
(core/reflection.cpp:402-494, core/reflection.h:382-388) -- over the lobes the seven materials add, and of Intersection::Le (core/primitive.cpp:142-145).

The lobes' f are analytic_forms' (lambert, oren_nayar, microfacet, the Fresnel terms: proven on the reference's films by tests/test_analytic_host.py);
the pdfs, the sampling maps, the lobe choice and the specular lobes are written here from core/reflection.cpp.  Everything is evaluated in the BSDF's
local frame (BSDF ctor, reflection.cpp:471-479: nn = dgShading.nn, sn = Normalize(dgShading.dpdu), tn = Cross(nn, sn)); the frame and the geometric
normal are INPUTS -- a fixture holds the float32 values the reference had at the hit --, so these forms state the BSDF and nothing of the geometry.

`twin` names a deliberately wrong variant (tests only):
  fresnel_one               f, s_f: the microfacet and specular Fresnel terms taken as 1
  btdf_pdf_at_wi            pdf: BRDFToBTDF::Pdf taken at wi instead of -wi (reflection.cpp:231-234)
  specular_not_counted      pdf: specular lobes left out of Pdf's matchingComps (:464-469)
  blinn_pdf_without_zero    s_pdf, s_type: Blinn without the Dot(wo, H) <= 0 zero (:260, :270; in Pdf itself the zero is out of reach: Dot(wo, wo + wi) = 1 + Dot(wo, wi) >= 0)
  uber_order_dgtr           s_wi, s_type: uber's lobes taken in the order D, G, T, R (uber.cpp:62-85 adds T, D, G, R)
  sample_pdf_not_averaged   s_pdf: Sample_f's pdf not divided by matchingComps (:442)
  flags_any_bit             n_components: a lobe matches when it shares ANY bit with the flags (reflection.h:96-98 asks for all of its bits)
  le_both_sides             le: Lemit on both sides of the emitter (lights/area.h: only where Dot(n, w) > 0)"""
import numpy as np

import analytic_forms as F

REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY, SPECULAR, ALL = 1, 2, 4, 8, 16, 31
FLAG_CYCLE = (ALL, ALL & ~SPECULAR, REFLECTION | SPECULAR, TRANSMISSION | SPECULAR, REFLECTION | DIFFUSE | GLOSSY, TRANSMISSION | DIFFUSE | GLOSSY)
Z = np.array([0.0, 0.0, 1.0])
PI = np.pi

# the exclusion rule's fixed distances (never an error of anything): a direction this close (cosine) to the geometric or the shading horizon,
# u3 * matchingComps this close to an integer that separates two lobes, sin^2 of the refracted angle this close to 1
HORIZON = 1e-3
LOBE_EDGE = 1e-5
TIR_EDGE = 1e-3


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class Lobe:
    """one BxDF: its BxDFType bits, f(wo, wi), pdf(wo, wi) and sample(wo, u1, u2) -> (wi, pdf, f or None), all in the local frame"""

    def __init__(self, type_, f, pdf, sample):
        self.type, self.f, self.pdf, self.sample = type_, f, pdf, sample


def cosine_pdf(wo, wi):
    """BxDF::Pdf (reflection.cpp:227-230)"""
    return np.where(wo[..., 2] * wi[..., 2] > 0, np.abs(wi[..., 2]) / PI, 0.0)


def cosine_sample(wo, u1, u2):
    """BxDF::Sample_f (reflection.cpp:219-226) with CosineSampleHemisphere (core/mc.h:38-44) over ConcentricSampleDisk"""
    dx, dy = F.concentric_sample_disk(u1, u2)
    z = np.sqrt(np.maximum(0.0, 1 - dx * dx - dy * dy))
    wi = np.stack([dx, dy, np.where(wo[..., 2] < 0, -z, z)], -1)
    return wi, cosine_pdf(wo, wi)


def blinn_pdf(e, wo, wi, zero=True):
    """Blinn::Pdf (reflection.cpp:263-272)"""
    with np.errstate(all="ignore"):
        H = _unit(wo + wi)
        woh = _dot(wo, H)
        p = (e + 1) * np.abs(H[..., 2]) ** e / (2 * PI * 4 * woh)
    return np.where(woh <= 0, 0.0, p) if zero else p


def blinn_sample(e, wo, u1, u2, zero=True):
    """Blinn::Sample_f (reflection.cpp:246-262); Microfacet::Sample_f (:235-240) hands its pdf on whatever the hemisphere of wi"""
    cost = u1 ** (1.0 / (e + 1))
    sint = np.sqrt(np.maximum(0.0, 1 - cost * cost))
    phi = u2 * 2 * PI
    H = np.stack([sint * np.cos(phi), sint * np.sin(phi), cost], -1)
    H = np.where((wo[..., 2] * H[..., 2] > 0)[..., None], H, -H)
    woh = _dot(wo, H)
    wi = -wo + 2 * woh[..., None] * H
    with np.errstate(all="ignore"):
        p = (e + 1) * cost ** e / (2 * PI * 4 * woh)
    return wi, (np.where(woh <= 0, 0.0, p) if zero else p)


def flip_z(w):
    return w * np.array([1.0, 1.0, -1.0])


def brdf(type_, f, pdf, sample):
    return Lobe(type_, f, pdf, lambda wo, u1, u2: sample(wo, u1, u2) + (None,))


def btdf(type_, inner, twin):
    """BRDFToBTDF (reflection.h:140-175, reflection.cpp:63-72, :231-234): f at wi mirrored, the sample mirrored, the pdf at -wi"""
    pdf = inner.pdf if twin == "btdf_pdf_at_wi" else (lambda wo, wi: inner.pdf(wo, -wi))

    def sample(wo, u1, u2):
        wi, p, _ = inner.sample(wo, u1, u2)
        return flip_z(wi), p, None
    return Lobe(type_, lambda wo, wi: inner.f(wo, flip_z(wi)), pdf, sample)


def specular_reflection(r, fresnel):
    """SpecularReflection (reflection.cpp:96-103); fresnel(cos) -> [..., 1 or 3]"""
    def sample(wo, u1, u2):
        wi = wo * np.array([-1.0, -1.0, 1.0])
        with np.errstate(all="ignore"):
            f = fresnel(wo[..., 2]) * r / np.abs(wi[..., 2:3])
        return wi, np.ones(wo.shape[:-1]), f
    zero = lambda wo, wi: np.zeros(wo.shape)
    return Lobe(REFLECTION | SPECULAR, zero, lambda wo, wi: np.zeros(wo.shape[:-1]), sample)


def specular_transmission(t, etai, etat, twin=None):
    """SpecularTransmission (reflection.cpp:104-127).  sample() leaves the distance of sin^2 of the refracted angle to 1 in `.edge`"""
    lobe = Lobe(TRANSMISSION | SPECULAR, lambda wo, wi: np.zeros(wo.shape), lambda wo, wi: np.zeros(wo.shape[:-1]), None)

    def sample(wo, u1, u2):
        entering = wo[..., 2] > 0
        ei, et = np.where(entering, etai, etat), np.where(entering, etat, etai)
        sini2 = np.maximum(0.0, 1 - wo[..., 2] ** 2)
        eta = ei / et
        sint2 = eta * eta * sini2
        lobe.edge = np.abs(sint2 - 1)
        cost = np.sqrt(np.maximum(0.0, 1 - sint2))
        cost = np.where(entering, -cost, cost)
        wi = np.stack([eta * -wo[..., 0], eta * -wo[..., 1], cost], -1)
        Fr = np.ones(wo.shape[:-1]) if twin == "fresnel_one" else F.fr_dielectric(wo[..., 2], etai, etat)
        with np.errstate(all="ignore"):
            f = ((et * et) / (ei * ei) * (1 - Fr))[..., None] * t / np.abs(wi[..., 2:3])
        ok = sint2 < 1
        return np.where(ok[..., None], wi, 0.0), np.where(ok, 1.0, 0.0), np.where(ok[..., None], f, 0.0)
    lobe.sample = sample
    return lobe


def resolve(kw, p, u, v, trace=None):
    """a material's parameters at hits (p, u, v): a Texture is evaluated there (a float parameter takes the first channel), a literal stays"""
    trace = dict(cells=[], wraps=[]) if trace is None else trace
    out = {}
    for k, x in kw.items():
        if isinstance(x, F.Texture):
            x = x.eval(p, u, v, trace)
            x = x[..., 0] if k in F.Textured.FLOATS else x
        out[k] = x
    return out


def material_lobes(kind, kw, n, twin=None):
    """the BxDFs Material::GetBSDF adds, in its order, for n hits of one material whose parameters are literals or [n]-arrays.  A lobe that depends on
    a parameter being non-black must be present at all n hits or at none."""
    def c(k, d):
        return np.broadcast_to(np.maximum(F._param(kw.get(k, d)) * np.ones(3), 0.0), (n, 3))

    def present(x):
        a = x.any(-1)
        assert a.all() or not a.any(), "a lobe present at some hits of a material and absent at others"
        return bool(a.all())
    one = lambda ch: np.ones(ch.shape + (1,))
    dielectric = one if twin == "fresnel_one" else (lambda ch: F.fr_dielectric(ch, 1.5, 1.0)[..., None])
    zero_at = twin != "blinn_pdf_without_zero"

    def lambert(r):
        return brdf(REFLECTION | DIFFUSE, lambda wo, wi: F.lambert(r, wo, wi, Z), cosine_pdf, cosine_sample)

    def micro(r, e, fres):
        return brdf(REFLECTION | GLOSSY, lambda wo, wi: F.microfacet(r, e, fres, wo, wi, Z),
                    lambda wo, wi: np.where(wo[..., 2] * wi[..., 2] > 0, blinn_pdf(e, wo, wi, zero_at), 0.0), lambda wo, u1, u2: blinn_sample(e, wo, u1, u2, zero_at))
    rough = lambda: F.blinn_exponent(F._param(kw.get("roughness", .1)))
    if kind == "matte":
        kd, sig = c("Kd", 1), np.clip(F._param(kw.get("sigma", 0)) * np.ones(n), 0.0, 90.0)
        if not sig.any():                                         # materials/matte.cpp:58-61
            return [lambert(kd)]
        return [brdf(REFLECTION | DIFFUSE, lambda wo, wi: F.oren_nayar(kd, sig, wo, wi, Z), cosine_pdf, cosine_sample)]
    if kind == "plastic":                                         # materials/plastic.cpp:57-67
        return [lambert(c("Kd", 1)), micro(c("Ks", 1), rough(), dielectric)]
    if kind == "uber":                                            # materials/uber.cpp:61-85
        op = c("opacity", 1)
        lobes = {}
        if present(1 - op):
            lobes["T"] = specular_transmission(1 - op, 1.0, 1.0, twin)
        if present(op * c("Kd", 1)):
            lobes["D"] = lambert(op * c("Kd", 1))
        if present(op * c("Ks", 1)):
            lobes["G"] = micro(op * c("Ks", 1), rough(), dielectric)
        if present(op * c("Kr", 0)):
            lobes["R"] = specular_reflection(op * c("Kr", 0), dielectric)
        return [lobes[k] for k in ("DGTR" if twin == "uber_order_dgtr" else "TDGR") if k in lobes]
    if kind == "shinymetal":                                      # materials/shinymetal.cpp:54-63
        cond = lambda r: one if twin == "fresnel_one" else (lambda ch: F.fr_conductor(ch, F.approx_eta(r)))
        return [micro(np.ones(3), rough(), cond(c("Ks", 1))), specular_reflection(np.ones(3), cond(c("Kr", 1)))]
    if kind == "translucent":                                     # materials/translucent.cpp:60-82
        kd, ks, r, t = c("Kd", 1), c("Ks", 1), c("reflect", .5), c("transmit", .5)
        lobes = []
        if not present(r) and not present(t):
            return lobes
        if present(kd):
            if present(r):
                lobes.append(lambert(r * kd))
            if present(t):
                lobes.append(btdf(TRANSMISSION | DIFFUSE, lambert(t * kd), twin))
        if present(ks):
            if present(r):
                lobes.append(micro(r * ks, rough(), dielectric))
            if present(t):
                lobes.append(btdf(TRANSMISSION | GLOSSY, micro(t * ks, rough(), dielectric), twin))
        return lobes
    if kind == "mirror":                                          # materials/mirror.cpp:51-53 (FresnelNoOp)
        return [specular_reflection(c("Kr", 1), one)]
    if kind == "glass":                                           # materials/glass.cpp:53-61
        ior = F._param(kw.get("index", 1.5)) * np.ones(n)
        lobes = []
        if present(c("Kr", 1)):
            lobes.append(specular_reflection(c("Kr", 1), one if twin == "fresnel_one" else (lambda ch: F.fr_dielectric(ch, 1.0, ior)[..., None])))
        if present(c("Kt", 1)):
            lobes.append(specular_transmission(c("Kt", 1), 1.0, ior, twin))
        return lobes
    raise ValueError(kind)


class Bsdf:
    """The BSDF of n hits of one material.  nn, dpdu: bsdf->dgShading's normal and dpdu; ng: dg.nn, the geometric normal (all [n, 3], world)."""

    def __init__(self, kind, kw, nn, dpdu, ng, twin=None):
        self.n, self.twin = len(nn), twin
        self.nn, self.ng = np.asarray(nn, np.float64), np.asarray(ng, np.float64)
        self.sn = _unit(np.asarray(dpdu, np.float64))
        self.tn = np.cross(self.nn, self.sn)
        self.lobes = material_lobes(kind, kw, self.n, twin)

    def local(self, w):
        return np.stack([_dot(w, self.sn), _dot(w, self.tn), _dot(w, self.nn)], -1)

    def world(self, w):
        return self.sn * w[..., 0:1] + self.tn * w[..., 1:2] + self.nn * w[..., 2:3]

    def matches(self, lobe, flags):
        if self.twin == "flags_any_bit":
            return (lobe.type & flags) != 0
        return (lobe.type & flags) == lobe.type                   # BxDF::MatchesFlags reflection.h:96-98

    def n_components(self, flags):
        return sum((self.matches(l, flags).astype(np.int64) for l in self.lobes), np.zeros(self.n, np.int64))

    def f(self, wo, wi, flags):
        """BSDF::f reflection.cpp:480-494, world directions"""
        same = _dot(wi, self.ng) * _dot(wo, self.ng) > 0
        flags = np.where(same, flags & ~TRANSMISSION, flags & ~REFLECTION)
        lo, li = self.local(wo), self.local(wi)
        out = np.zeros((self.n, 3))
        for l in self.lobes:
            if not l.type & SPECULAR:
                out += np.where(self.matches(l, flags)[..., None], l.f(lo, li), 0.0)
        return out

    def pdf(self, wo, wi, flags):
        """BSDF::Pdf reflection.cpp:458-470"""
        lo, li = self.local(wo), self.local(wi)
        total, count = np.zeros(self.n), np.zeros(self.n)
        for l in self.lobes:
            m = self.matches(l, flags)
            total += np.where(m, l.pdf(lo, li), 0.0)
            if not (self.twin == "specular_not_counted" and l.type & SPECULAR):
                count += m
        with np.errstate(all="ignore"):
            return np.where(count > 0, total / count, 0.0)

    def sample(self, wo, u, flags):
        """BSDF::Sample_f reflection.cpp:402-457 -> dict(s_wi, s_f, s_pdf, s_type, near, drawn): a failed sample (pdf == 0) is all zeros; `near`:
        u3 * matchingComps within LOBE_EDGE of an integer between two lobes, or the refraction within TIR_EDGE of total internal reflection; `drawn`:
        the direction the chosen lobe drew, kept for a failed sample too (on the horizon its pdf is 0 in one arithmetic and tiny in another)"""
        n = self.n
        lo = self.local(wo)
        matching = self.n_components(flags)
        x = u[..., 2] * matching
        which = np.minimum(np.floor(x).astype(np.int64), matching - 1)
        k = np.rint(x)
        near = (np.abs(x - k) < LOBE_EDGE) & (k >= 1) & (k <= matching - 1)
        s_wi, s_f, s_pdf, s_type = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int64)
        drawn = np.zeros((n, 3))                                   # the chosen lobe's direction, whether or not its pdf let the sample stand
        rank = np.zeros(n, np.int64)                               # how many matching lobes come before this one
        for l in self.lobes:
            m = self.matches(l, flags)
            sel = m & (rank == which) & (matching > 0)
            rank = rank + m
            if not sel.any():
                continue
            wi, pdf, fs = l.sample(lo, u[..., 0], u[..., 1])
            ok = sel & (pdf != 0)                                  # the chosen lobe's own pdf decides (:428-431)
            if l.type & SPECULAR:
                f = fs
                if l.type & TRANSMISSION:
                    near |= sel & (l.edge < TIR_EDGE)
            else:
                for o in self.lobes:
                    if o is not l:
                        pdf = pdf + np.where(self.matches(o, flags), o.pdf(lo, wi), 0.0)
                f = self.f(wo, self.world(wi), flags)
            if self.twin != "sample_pdf_not_averaged":
                pdf = pdf / np.maximum(matching, 1)
            s_wi = np.where(ok[..., None], self.world(wi), s_wi)
            drawn = np.where(sel[..., None], np.nan_to_num(self.world(wi)), drawn)
            s_f = np.where(ok[..., None], f, s_f)
            s_pdf = np.where(ok, pdf, s_pdf)
            s_type = np.where(ok, l.type, s_type)
        return dict(s_wi=s_wi, s_f=s_f, s_pdf=s_pdf, s_type=s_type, near=near, drawn=drawn)


def le(L, ng, wo, twin=None):
    """AreaLight::L (lights/area.h): Lemit where Dot(n, w) > 0"""
    if twin == "le_both_sides":
        return np.broadcast_to(np.asarray(L, np.float64), ng.shape).copy()
    return np.where((_dot(ng, wo) > 0)[..., None], np.asarray(L, np.float64), 0.0)


def horizon(w, *normals):
    """a direction within HORIZON (cosine) of the plane of one of the normals"""
    out = np.zeros(w.shape[:-1], bool)
    for nrm in normals:
        out |= np.abs(_dot(_unit(w), _unit(nrm))) < HORIZON
    return out


def query_error(got, want, included, unit_scale=False):
    """e = max_c |got - want| / (max_c |want| + 0.01 S) per query, S the median of max_c |want| over the included queries where it is not zero
    (1 for a direction).  A query whose scale is zero has e = 0 when got is zero too, else infinity."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    mx = np.abs(want).max(-1)
    nz = included & (mx > 0)
    S = 1.0 if unit_scale else (float(np.median(mx[nz])) if nz.any() else 0.0)
    num, den = np.abs(got - want).max(-1), mx + 0.01 * S
    with np.errstate(all="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))
