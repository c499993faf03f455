"""The medium-query cases of tests/golden/medium/: the regions, the seeded queries, the scene text, the record layout of the reference-side plugin
(tests/golden/medium_probe.cpp) and the float64 forms (tests/medium_forms.py) on a fixture.  Shared by tests/golden/make_medium_golden.py,
tests/test_medium_host.py and tests/test_gpu_medium.py."""
import re

import numpy as np

import analytic_cases as A
import analytic_forms as F
import bsdf_forms as B
import medium_forms as MF

SEED = 5                        # the frame's seed ("integer seed" of the keyed sampler): the keyed stream depends on it
N_QUERIES = 1024
OUTPUTS = MF.OUTPUTS
COLUMNS = {"sigma_a": slice(0, 3), "sigma_s": slice(3, 6), "sigma_t": slice(6, 9), "lve": slice(9, 12), "phase": 12, "hit": 13, "t01": slice(14, 16),
           "tau": slice(16, 19), "tr": slice(19, 22), "tr_null": slice(22, 25), "draws_tr": 25, "lv": slice(26, 29), "draws_lv": 29}
DISCRETE = ("hit", "draws_tr", "draws_lv")

BOX = dict(p0=(-1, -.5, -1.5), p1=(1.5, 1, 1))
HOM_CTM = [("Translate", .4, -.3, .6), ("Rotate", 30, 1, 2, .5), ("Scale", 1.3, .7, 1.1)]
GRID = dict(kind="volumegrid", nx=5, ny=4, nz=3, values=A.grid_values(5, 4, 3, 23))
# the steps: the extents' world diagonals are below 4.6, so a Tau at `stepsize` takes at most 19 samples, an emission march (ray directions of
# length .6 to 2, Taus at .5 stepsize over world length stepsize x |d|) at most 39 steps and 39 + 37 Tau samples
CASES = {
    "homogeneous_ctm": dict(stepsize=.25, twin="volume_ctm_ignored",
                            medium=dict(kind="homogeneous", sigma_a=(.3, .4, .5), sigma_s=(.2, .1, .15), Le=(.4, .3, .2), g=.3, ctm=HOM_CTM, **BOX)),
    "exponential_ctm": dict(stepsize=.25, twin="height_from_origin",
                            medium=dict(kind="exponential", a=1.2, b=.8, updir=A.UPDIR, sigma_a=(.3, .4, .5), sigma_s=(.2, .1, .15), Le=(.3, .2, .4), g=-.2,
                                        ctm=A.VOL_CTM, **BOX)),
    "grid": dict(stepsize=.25, twin="voxel_centres_at_corners", also=("grid_axes_transposed",),
                 medium=dict(GRID, sigma_a=(.3, .4, .5), sigma_s=(.2, .1, .15), g=.5, **BOX)),
    "grid_roulette": dict(stepsize=.25, twin="grid_axes_transposed", also=("voxel_centres_at_corners",),
                          medium=dict(GRID, sigma_a=(3, 4, 5), sigma_s=(.5, .4, .3), Le=(.5, .4, .3), g=0, **BOX)),
}


def medium_form(name, twin=None):
    c = CASES[name]
    med = c["medium"]
    more = {k: med[k] for k in ("Le", "g", "a", "b", "updir", "nx", "ny", "nz", "values") if k in med}
    return F.Medium(med["p0"], med["p1"], med["sigma_a"], med["sigma_s"], v2w=A._ctm(med.get("ctm", [])), kind=med["kind"], integrator="emission",
                    stepsize=c["stepsize"], twin=twin, **more)


def scene_text(name, queries="queries.bin", dump="medium.bin"):
    """the scene file: the frame (4 x 4, one unjittered sample per pixel) means nothing to the "mediumprobe" integrator, which answers the query file"""
    c = CASES[name]
    return ('LookAt 0 0 -9 0 0 0 0 1 0\nCamera "perspective" "float fov" [40]\n'
            'Film "image" "integer xresolution" [4] "integer yresolution" [4] "string filename" ["out.exr"]\n'
            'Sampler "keyed" "string inner" ["stratified"] "integer seed" [%d] "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\n'
            'PixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n'
            'SurfaceIntegrator "mediumprobe" "string queries" ["%s"] "string dump" ["%s"] "float stepsize" [%s]\n'
            'VolumeIntegrator "emission" "float stepsize" [%s]\nWorldBegin\n' % (SEED, queries, dump, A._fmt(c["stepsize"]), A._fmt(c["stepsize"]))
            + A._volume_text(c["medium"]) +
            'AttributeBegin\nMaterial "matte"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [50 50 50 51 50 50 50 51 50]\nAttributeEnd\nWorldEnd\n')


def product_text(text):
    """a fixture's scene text as the product parses it: the probe integrator is the reference's plugin, any surface integrator serves; the
    product's own sampler takes the keyed wrapper's seed"""
    text = re.sub(r'SurfaceIntegrator "mediumprobe"[^\n]*', 'SurfaceIntegrator "directlighting"', str(text))
    return text


def queries(name):
    """seeded query records: points inside, outside and on both sides of each face; rays that cross, graze, start inside or miss, with unnormalised
    directions, maxt = inf, maxt inside the region, and mint > maxt"""
    med = medium_form(name)
    rs = np.random.RandomState(sum(map(ord, name)))
    n = N_QUERIES
    v2w = np.linalg.inv(med.w2v)
    ext, mid = med.p1 - med.p0, (med.p0 + med.p1) / 2
    box = lambda k, s: mid + (rs.uniform(size=(k, 3)) - .5) * ext * s
    q = box(n, 1.5)                                                     # volume space: inside and around the extent
    f = np.arange(n) % 4 == 0                                           # a quarter on both sides of a face, .003 to .08 away
    ax, side = rs.randint(0, 3, n), rs.randint(0, 2, n)
    off = rs.uniform(.003, .08, n) * rs.choice([-1.0, 1.0], n)
    inner = box(n, .9)
    inner[np.arange(n), ax] = np.where(side == 1, med.p1[ax], med.p0[ax]) + off
    q[f] = inner[f]
    p = F.xpoint(v2w, q)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    w, wp = unit(rs.normal(size=(n, 3))), unit(rs.normal(size=(n, 3)))
    start_in = rs.uniform(size=n) < .35
    o = np.where(start_in[:, None], box(n, .95), mid + unit(rs.normal(size=(n, 3))) * ext * rs.uniform(1.0, 1.8, (n, 1)))
    target = box(n, 1.5)                                                # some rays miss or graze the extent
    o, target = F.xpoint(v2w, o), F.xpoint(v2w, target)
    d = unit(target - o) * rs.uniform(.6, 2.0, (n, 1))
    mint = np.where(rs.uniform(size=n) < .7, 0.0, rs.uniform(0, .5, n))
    maxt = np.where(rs.uniform(size=n) < .5, np.inf, rs.uniform(.5, 6.0, n))
    empty = np.arange(n) % 37 == 5
    mint, maxt = np.where(empty, 2.0, mint), np.where(empty, 1.0, maxt)   # mint > maxt: an ordinary empty ray
    rays = np.concatenate([o, d, mint[:, None], maxt[:, None]], -1).astype(np.float32)
    rng = np.stack([rs.randint(0, 1 << 31, n), rs.randint(0, 40, n)], -1).astype(np.uint32)
    rng[::7, 0] |= np.uint32(0x80000000)
    return dict(p=p.astype(np.float32), w=w.astype(np.float32), wp=wp.astype(np.float32), rays=rays, u=rs.uniform(size=n).astype(np.float32),
                u_scatter=rs.uniform(.02, .98, n).astype(np.float32), rng=rng)


def query_records(q):
    """the probe's input: 24 words per query (tests/golden/medium_probe.cpp)"""
    rec = np.zeros((len(q["p"]), 24), np.float32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:17], rec[:, 17], rec[:, 18] = q["p"], q["w"], q["wp"], q["rays"], q["u"], q["u_scatter"]
    rec.view(np.uint32)[:, 19:21] = q["rng"]
    return rec


def answer(ans, k):
    a = ans[:, COLUMNS[k]]
    return a.astype(np.int32) if k in DISCRETE else a


def evaluate(name, q, seed=SEED, twin=None):
    return MF.evaluate(medium_form(name, twin), q, float(np.float32(CASES[name]["stepsize"])), seed)


def errors(got, w, inc):
    """per float output the largest error of `got` (a dict, or the reference's answer records) against the forms over the included queries, in the
    measure of bsdf_forms.query_error"""
    get = (lambda k: answer(got, k)) if isinstance(got, np.ndarray) else (lambda k: got[k])
    return {k: float(B.query_error(get(k), w[k], inc)[inc].max()) for k in OUTPUTS}


def ref_err(name, q, ans, seed=SEED, twin=None):
    """-> ({output: the reference's largest error against the forms over the included queries}, left-out share, the forms' dict)"""
    w = evaluate(name, q, seed, twin)
    inc = ~w["excluded"]
    return errors(ans, w, inc), float(w["excluded"].mean()), w


def coverage(name, q, w):
    """what the included queries reach: the generator refuses a case whose region no included query enters -> list of what is missing"""
    inc = ~w["excluded"]
    missing = []
    if (w["sigma_t"][inc].any(-1)).mean() < .2 or (~w["sigma_t"][inc].any(-1)).mean() < .2:
        missing.append("points inside and outside")
    if w["hit"][inc].mean() < .3 or (1 - w["hit"][inc]).mean() < .1:
        missing.append("rays that hit and rays that miss")
    if (w["tau"][inc].any(-1)).mean() < .3:
        missing.append("a Tau that is not zero")
    if CASES[name]["medium"].get("Le") and (w["lv"][inc].any(-1)).mean() < .3:
        missing.append("an Lv that is not zero")
    if name == "grid_roulette" and (w["roulette"][inc] > 0).sum() < 30:
        missing.append("marches that reach the roulette")
    return missing
