"""Float64 forms of what DeviceScene.medium (rt_medium_device) answers, on analytic_forms.Medium for the transform, the extent and the density.

Unlike Medium.depth / Medium.lv, which state exact integrals beside an allowance, these REPLAY the reference's loops with the supplied offsets and
the keyed draws, as tests/test_analytic_host.py: tau_loop does: DensityRegion::Tau (core/volume.cpp:137-153) sample by sample and
EmissionIntegrator::Li (integrators/emission.cpp:60-95) step by step, roulette included.  What float32 can decide differently from float64 is left
out by rule, never by looking at an answer:
  - a point within BAND of a face of the extent (Inside, Density's extent test),
  - a ray whose clipped interval is shorter than BAND, or that misses the extent by less (IntersectP),
  - a Tau whose sample count turns within BAND of t1, or whose first sample lies within BAND of a face,
  - an emission march whose step count turns within BAND_N of an integer, whose roulette test lies within BAND_Y of its threshold, or one of
    whose steps' Tau is left out.
"""
import numpy as np

import analytic_forms as F
import light_forms as LF

BAND = 2e-5           # lengths, world or volume units (the extents are of order 1; float32 positions there are good to 1e-6)
BAND_N = 1e-4         # of (t1 - t0) / stepsize, a count
BAND_Y = 1e-3         # relative, of Tr.y() against 1e-3
Y_WEIGHTS = np.array([0.212671, 0.715160, 0.072169])       # Spectrum::y(), core/color.h

POINT_OUTPUTS = ("sigma_a", "sigma_s", "sigma_t", "lve", "phase")
RAY_OUTPUTS = ("t01", "tau", "tr", "tr_null", "lv")
OUTPUTS = POINT_OUTPUTS + RAY_OUTPUTS                      # the float outputs; hit, draws_tr and draws_lv are compared for equality


def sigma_a(med):
    return med.sigma_t - med.sigma_s


def inside(med, p):
    """extent.Inside(WorldToVolume(p)) and whether p is within BAND of a face's plane"""
    q = F.xpoint(med.w2v, p)
    near = (np.abs(q - med.p0) < BAND).any(-1) | (np.abs(q - med.p1) < BAND).any(-1)
    return ((q >= med.p0) & (q <= med.p1)).all(-1), near


def density(med, p):
    """Density(WorldToVolume(p)) with the extent's test (0 outside); 1 inside a homogeneous region"""
    ins, near = inside(med, p)
    with np.errstate(all="ignore"):
        f = med.density(p)
    return np.where(ins, f, 0.0), near


def points(med, p, w, wp):
    f, near = density(med, p)
    ins = inside(med, p)[0]
    cos = (w * wp).sum(-1)
    ph = med.phase(cos) * (ins if med.kind == "homogeneous" else 1.0)        # a density region's p() has no inside test (volume.h:84-86)
    return dict(sigma_a=f[:, None] * sigma_a(med), sigma_s=f[:, None] * med.sigma_s, sigma_t=f[:, None] * med.sigma_t, lve=f[:, None] * med.le, phase=ph,
                band_point=near)


def clip_raw(med, o, d, lo, hi):
    """BBox::IntersectP on the volume-space ray, in the ray's own parameter: t0, t1 as the slabs leave them (t0 > t1: a miss)"""
    oo, od = F.xpoint(med.w2v, o), F.xvec(med.w2v, d)
    t0, t1 = np.array(np.broadcast_to(lo, o.shape[:-1]), np.float64), np.array(np.broadcast_to(hi, o.shape[:-1]), np.float64)
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = 1.0 / od[..., a]
            tn, tf = (med.p0[a] - oo[..., a]) * inv, (med.p1[a] - oo[..., a]) * inv
            tn, tf = np.minimum(tn, tf), np.maximum(tn, tf)
            t0, t1 = np.maximum(t0, np.where(np.isnan(tn), -np.inf, tn)), np.minimum(t1, np.where(np.isnan(tf), np.inf, tf))
    return t0, t1


def tau_replay(med, o, d, lo, hi, h, u):
    """VolumeRegion::Tau(Ray(o, d, lo, hi), h, u) -> (tau [n, 3], band [n], samples taken [n])"""
    length = np.linalg.norm(d, axis=-1)
    dn = d / length[:, None]
    t0, t1 = clip_raw(med, o, dn, lo * length, hi * length)
    ok = t1 >= t0
    band = np.abs(t1 - t0) < BAND
    t0, t1 = np.where(ok, t0, 0.0), np.where(ok, t1, 0.0)
    if med.kind == "homogeneous":                                              # homogeneous.cpp:63-67: Distance(ray(t0), ray(t1)) * (sigma_a + sigma_s)
        return (t1 - t0)[:, None] * med.sigma_t, band, np.zeros(len(o), np.int64)
    x = (t1 - t0) / h - u
    K = np.where(ok, np.maximum(np.ceil(x), 0.0), 0.0).astype(np.int64)
    band = band | (ok & (np.abs(x - np.rint(x)) * h < BAND))
    start_near = inside(med, o + dn * t0[:, None])[1]
    band = band | (ok & start_near & (u * h < BAND))
    ks = np.arange(max(int(K.max()), 1))
    s = t0[:, None] + (u[:, None] + ks) * h
    f, _ = density(med, o[:, None, :] + s[..., None] * dn[:, None, :])
    f = f * (ks < K[:, None])
    return (f.sum(-1) * h)[:, None] * med.sigma_t, band, K


def lv_replay(med, o, d, lo, hi, step, u_scatter, key, ctr, seed):
    """EmissionIntegrator::Li with a sample -> (Lv [n, 3], band [n], draws [n], steps that took the roulette's draw [n])"""
    n = len(o)
    t0, t1 = clip_raw(med, o, d, lo, hi)
    ok = (t1 >= t0) & ((t1 - t0) != 0.0)
    band = np.abs(t1 - t0) * np.linalg.norm(d, axis=-1) < BAND
    t0, t1 = np.where(ok, t0, 0.0), np.where(ok, t1, 1.0)
    x = (t1 - t0) / step
    N = np.where(ok, np.ceil(x), 0.0).astype(np.int64)
    band = band | (ok & (np.abs(x - np.rint(x)) < BAND_N))
    dt = (t1 - t0) / np.maximum(N, 1)
    Tr, Lv = np.ones((n, 3)), np.zeros((n, 3))
    used, roulette = np.zeros(n, np.int64), np.zeros(n, np.int64)
    alive = ok.copy()
    p = o + d * t0[:, None]
    for i in range(int(N.max()) if n else 0):
        act = alive & (i < N)
        if not act.any():
            break
        t = t0 + (u_scatter + i) * dt
        prev, p = p, o + d * t[:, None]
        u = LF.keyed_draw(key, ctr + used, seed).astype(np.float64)
        used = used + act
        seg = np.where(act[:, None], p - prev, [1.0, 0.0, 0.0])
        tau, b, _ = tau_replay(med, prev, seg, np.zeros(n), np.ones(n), .5 * step, u)
        Tr = np.where(act[:, None], Tr * np.exp(-tau), Tr)
        band = band | (act & b)
        y = (Tr * Y_WEIGHTS).sum(-1)
        low = act & (y < 1e-3)
        band = band | (act & (np.abs(y - 1e-3) < BAND_Y * 1e-3))
        u2 = LF.keyed_draw(key, ctr + used, seed)
        used, roulette = used + low, roulette + low
        die = low & (u2 > np.float32(.5))
        alive = alive & ~die
        Tr = np.where((low & ~die)[:, None], Tr / .5, Tr)
        cont = act & ~die
        f, near = density(med, p)
        band = band | (cont & near)
        Lv = Lv + np.where(cont[:, None], Tr * f[:, None] * med.le, 0.0)
    return Lv * dt[:, None], band, used, roulette


def evaluate(med, q, step, seed):
    """the forms on the query records q (p, w, wp, rays [n, 8], u, u_scatter, rng [n, 2]) -> dict of every output, `excluded`, and what coverage reads"""
    g = lambda k: q[k].astype(np.float64)
    out = points(med, g("p"), g("w"), g("wp"))
    rays = g("rays")
    o, d, lo, hi = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    key, ctr = q["rng"][:, 0].astype(np.uint64), q["rng"][:, 1].astype(np.uint64)
    t0, t1 = clip_raw(med, o, d, lo, hi)
    hit = t1 >= t0
    with np.errstate(all="ignore"):
        band_hit = np.abs(t1 - t0) * np.linalg.norm(d, axis=-1) < BAND
    out["hit"] = hit.astype(np.int32)
    out["t01"] = np.where(hit[:, None], np.stack([t0, t1], -1), 0.0)
    out["tau"], b_tau, out["tau_samples"] = tau_replay(med, o, d, lo, hi, step, g("u"))
    out["tr"] = np.exp(-out["tau"])
    tau4, b_null, _ = tau_replay(med, o, d, lo, hi, 4 * step, LF.keyed_draw(key, ctr, seed).astype(np.float64))
    out["tr_null"] = np.exp(-tau4)
    out["draws_tr"] = np.ones(len(o), np.int32)
    out["lv"], b_lv, used, out["roulette"] = lv_replay(med, o, d, lo, hi, step, g("u_scatter"), key, ctr.astype(np.int64), seed)
    out["draws_lv"] = used.astype(np.int32)
    out["excluded"] = out.pop("band_point") | band_hit | b_tau | b_null | b_lv
    return out
