"""Generate the seeded cross-feature fixtures in tests/golden/mixes/ by running the UNMODIFIED reference (oracle/_ref/pbrt_ref_keyed under the keyed
sampler, and the countaccel wrapper for ray counts), the way tests/golden/make_bidir_golden.py does for the bidirectional integrator.  Runs only
where the reference sources exist; mix_scene(seed) is importable without them (tests/test_mixes_host.py and tests/test_gpu_mixes.py call it).

    python tests/golden/make_mix_golden.py

mix_scene(seed) draws one scene from np.random.default_rng(seed): one value per axis (geometry, materials, lights, medium, integrator, sampler,
accelerator, camera, filter, crop window, film size), never a combination rt_render refuses by design.  Triangles only.

Seeds are tried in order from 0.  Whether a seed becomes a fixture is decided by the reference's films alone (accept()):
  * no stderr lines, a finite film, at least 30 % of the pixels non-black;
  * for every drawn new-feature axis the reference's film with that feature taken out -- the infinite light removed, the medium's density replaced by
    the homogeneous region of the same constants, shinymetal / translucent replaced by matte, bidirectional replaced by path -- differs from the
    fixture film on at least 5 % of the pixels (per-pixel L2 > 1e-3).
Every seed tried is listed in tests/golden/mixes/MANIFEST.json, rejected ones with their reason.  The generator stops at the first count >= 48 of
accepted fixtures whose coverage table (coverage_gaps(), asserted again by tests/test_mixes_host.py) has no gap; 64 accepted fixtures with a gap is
an error, to be answered by the draw's weights.

Each mix_<seed>.npz holds the scene text, the reference's float film (rgb, alpha), its ray counts / StatsPrint table, `features` (what was drawn,
JSON), `shares` (the ablation shares, JSON) and `bar`: "strict" (Whitted or DirectLighting without an infinite light: every pixel within 1e-5, equal
ray counts) or "loose" (path, bidirectional or an infinite light: the 99.5 % bar).  Fixtures are DATA; no reference source text is stored."""
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

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mixes")
MIN_SHARE = 0.05
MIN_LIT = 0.30
MAX_BYTES = 64 * 1024
WANT, HARD_STOP = 48, 64

INTEGRATORS = ("whitted", "directlighting", "path", "bidirectional")
LIGHTS = ("area", "point", "spot", "distant", "infinite")
MEDIA = ("homogeneous", "exponential", "volumegrid")
NEW_MATERIALS = ("shinymetal", "translucent")
FILTERS = ("box", "gaussian", "mitchell", "sinc", "triangle")

QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [%s]\n'
FLOOR = QUAD % "756 0 -200 -200 0 -200 -200 0 760 756 0 760"
PANEL_A = QUAD % "60 10 420 300 10 520 300 360 520 60 360 420"
PANEL_B = QUAD % "320 10 330 520 10 430 520 300 430 320 300 330"
SHEET = QUAD % "120 40 260 440 40 260 440 330 260 120 330 260"
INF_RE = re.compile(r'^LightSource "infinite".*\n', re.M)
INTEGRATOR_RE = re.compile(r'^SurfaceIntegrator "bidirectional"[^\n]*\n', re.M)


def pick(rng, seq, weights=None):
    """One element of seq (rng.random() only: the stream does not depend on how numpy draws from a list)."""
    u = float(rng.random())
    if weights is None:
        return seq[min(int(u * len(seq)), len(seq) - 1)]
    acc, tot = 0.0, float(sum(weights))
    for s, w in zip(seq, weights):
        acc += w / tot
        if u < acc:
            return s
    return seq[-1]


def uni(rng, lo, hi, digits=3):
    return round(lo + (hi - lo) * float(rng.random()), digits)


def col(rng, lo, hi, digits=2):
    return "%s %s %s" % (uni(rng, lo, hi, digits), uni(rng, lo, hi, digits), uni(rng, lo, hi, digits))


def roughness(rng):
    return pick(rng, (0.02, uni(rng, 0.05, 0.4), 0.6))


def material(rng, kind):
    if kind == "matte":
        return '"matte" "color Kd" [%s] "float sigma" [%d]' % (col(rng, .2, .8), pick(rng, (0, 30)))
    if kind == "plastic":
        return '"plastic" "color Kd" [%s] "color Ks" [%s] "float roughness" [%s]' % (col(rng, .1, .7), col(rng, .2, .6), roughness(rng))
    if kind == "uber":
        return '"uber" "color Kd" [%s] "color Ks" [%s] "color Kr" [.2 .2 .2] "float roughness" [%s] "color opacity" [%s]' % (
            col(rng, .1, .7), col(rng, .1, .4), roughness(rng), col(rng, .4, .9))
    if kind == "mirror":
        return '"mirror" "color Kr" [%s]' % col(rng, .7, .95)
    if kind == "glass":
        return '"glass" "float index" [%s]' % uni(rng, 1.2, 1.7, 2)
    if kind == "shinymetal":
        return '"shinymetal" "color Ks" [%s] "color Kr" [%s] "float roughness" [%s]' % (col(rng, .3, .9), col(rng, .3, .8), roughness(rng))
    assert kind == "translucent"
    subset = pick(rng, ("full", "reflect_black", "transmit_black", "Ks_black", "Kd_black"))
    kd, ks, refl, tran = col(rng, .3, .7), col(rng, .2, .5), col(rng, .3, .6), col(rng, .4, .8)
    if subset == "reflect_black": refl = "0 0 0"
    if subset == "transmit_black": tran = "0 0 0"
    if subset == "Ks_black": ks = "0 0 0"
    if subset == "Kd_black": kd = "0 0 0"
    return '"translucent" "color Kd" [%s] "color Ks" [%s] "color reflect" [%s] "color transmit" [%s] "float roughness" [%s]' % (kd, ks, refl, tran, roughness(rng))


def obj(mat, shape, xform=""):
    return 'AttributeBegin\n%sMaterial %s\n%s\nAttributeEnd\n' % (xform, mat, shape.rstrip("\n"))


def tetra_soup(rng, n_tris, n_parts):
    """A soup of n_tris small triangles as n_tris / 4 scattered tetrahedra with integer coordinates, dealt round-robin into n_parts meshes (one per
    material).  Four triangles share four vertices and every number has at most three digits: the text of 3000 triangles compresses to about 25 KB
    where 3000 independent float triangles (scenes.lcg_soup) take 160 KB, far above a fixture's 64 KiB."""
    k = n_tris // 4
    half = 30 if n_tris <= 300 else 12
    centres = rng.integers([60, 40, 80], [500, 440, 520], size=(k, 3))
    verts = centres[:, None, :] + rng.integers(-half, half + 1, size=(k, 4, 3))
    out = []
    for p in range(n_parts):
        v = verts[p::n_parts]
        idx = " ".join("%d %d %d %d %d %d %d %d %d %d %d %d" % (a, a + 1, a + 2, a, a + 1, a + 3, a, a + 2, a + 3, a + 1, a + 2, a + 3) for a in range(0, 4 * len(v), 4))
        out.append('Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n' % (idx, " ".join(str(int(x)) for x in v.ravel())))
    return out


def volume_text(rng, kind, emission):
    sig = '"color sigma_a" [%s] "color sigma_s" [%s] "float g" [%s]' % (col(rng, .001, .003, 4), col(rng, .002, .004, 4), uni(rng, -.3, .5, 2))
    if emission:
        sig += ' "color Le" [%s]' % col(rng, .001, .004, 4)
    if kind == "homogeneous":
        return 'Volume "homogeneous" "point p0" [0 0 0] "point p1" [556 549 559] %s\n' % sig, {}
    xform = "Translate 278 0 280\nRotate %d 0 1 0\nRotate %d 1 0 0\nScale %s %s %s\n" % (
        rng.integers(-40, 41), rng.integers(-15, 16), uni(rng, .8, 1.3, 2), uni(rng, .8, 1.2, 2), uni(rng, .8, 1.3, 2))
    box = '"point p0" [-260 5 -260] "point p1" [260 500 260]'
    if kind == "exponential":
        up = "%s 1 %s" % (uni(rng, -.4, .4, 2), uni(rng, -.4, .4, 2))
        a, b = uni(rng, 1.0, 2.5, 2), uni(rng, .002, .008, 4)
        return ('AttributeBegin\n%sVolume "exponential" %s %s "float a" [%s] "float b" [%s] "vector updir" [%s]\nAttributeEnd\n' % (xform, box, sig, a, b, up),
                dict(a=a, b=b))
    n = [int(rng.integers(2, 13)) for _ in range(3)]
    vals = np.round(rng.random(n[0] * n[1] * n[2]) * 2.0, 2)
    return ('AttributeBegin\n%sVolume "volumegrid" "integer nx" [%d] "integer ny" [%d] "integer nz" [%d] %s %s "float density" [%s]\nAttributeEnd\n' % (
        xform, n[0], n[1], n[2], box, sig, " ".join("%.9g" % v for v in vals)), dict(grid=n))


def mix_scene(seed):
    """(scene text, features) of one seeded draw.  The text is what the reference is given (keyed sampler, counting accelerator); ParsedScene
    unwraps both."""
    rng = np.random.default_rng(seed)
    f = {"seed": int(seed)}
    # ---- integrator first: it decides which media and strategies may be drawn
    integ = pick(rng, INTEGRATORS, (.30, .32, .19, .19))
    f["integrator"] = integ
    f["medium"] = "none" if integ == "bidirectional" or rng.random() < 0.36 else pick(rng, MEDIA)
    lights = [l for l in LIGHTS if rng.random() < (.45, .35, .35, .3, .27)[LIGHTS.index(l)]]
    if not lights:
        lights = [pick(rng, LIGHTS)]
    f["lights"] = lights
    opts = dict(integrator=integ, keyed=True, count=True, seed=int(rng.integers(0, 1000)))
    if integ == "path":
        opts["maxdepth"] = int(rng.integers(1, 9))
    f["strategy"] = None
    if integ == "directlighting":
        allowed = ["all", "one"]
        if "infinite" not in lights and not (f["medium"] != "none" and "area" in lights):
            allowed.append("weighted")
        f["strategy"] = pick(rng, allowed)
        opts["integrator_params"] = '"string strategy" ["%s"]' % f["strategy"]
    # ---- sampler, at most 4 samples per pixel (lowdiscrepancy 8 on the small frames only: the same number of camera samples)
    xres, yres = int(rng.integers(10, 20)) * 2 + 1, int(rng.integers(10, 20)) * 2 + 1
    sampler = pick(rng, ("stratified", "stratified_jitter", "lowdiscrepancy", "random"))
    f["sampler"] = sampler
    nx, ny = pick(rng, ((1, 1), (2, 1), (1, 2), (2, 2)))
    if sampler == "lowdiscrepancy":
        ps = pick(rng, (2, 4, 8))
        if ps == 8 and max(xres, yres) > 28:
            xres, yres = min(xres, 27), min(yres, 27)
        opts.update(sampler="lowdiscrepancy", pixelsamples=ps)
        f["spp"] = ps
    else:
        opts.update(sampler="random" if sampler == "random" else "stratified", xsamples=nx, ysamples=ny, jitter=sampler == "stratified_jitter")
        f["spp"] = nx * ny
    opts.update(xres=xres, yres=yres)
    f["film"] = [xres, yres]
    f["accelerator"] = opts["accelerator"] = pick(rng, ("kdtree", "grid"))
    f["filter"] = opts["pixel_filter"] = pick(rng, FILTERS)
    f["crop"] = None
    if rng.random() < 0.25:
        x0, y0 = uni(rng, 0, .3, 2), uni(rng, 0, .3, 2)
        f["crop"] = [x0, round(x0 + uni(rng, .5, .7, 2), 2), y0, round(y0 + uni(rng, .5, .7, 2), 2)]
        opts["crop"] = f["crop"]
    camera = pick(rng, ("perspective", "perspective_lens", "orthographic", "environment"), (.4, .2, .2, .2))
    f["camera"] = camera
    if camera == "perspective_lens":
        opts.update(lensradius=uni(rng, 4, 16, 1), focaldistance=uni(rng, 900, 1300, 0))
    f["volume_integrator"] = None
    if f["medium"] != "none":
        f["volume_integrator"] = pick(rng, ("emission", "single"))
        opts["volume_integrator"] = '"%s" "float stepsize" [%d]' % (f["volume_integrator"], rng.integers(15, 181))
    # ---- the world
    base = pick(rng, ("cornell", "open"))
    f["base"] = base
    kinds = ["matte", "plastic", "uber", "mirror", "glass", "shinymetal", "translucent"]
    weights = [1, 1, 1, .7, .7, 2.2, 2.2]
    chosen = []
    for _ in range(int(rng.integers(2, 5))):
        k = pick(rng, kinds, weights)
        weights[kinds.index(k)] = 0
        chosen.append(k)
    mats = [material(rng, k) for k in chosen]
    parts = []
    if "infinite" in lights:
        parts.append('LightSource "infinite" "color L" [%s] "integer nsamples" [%d]\n' % (col(rng, .3, 1.0), rng.integers(1, 4)))
    if "point" in lights:
        parts.append('LightSource "point" "point from" [%d %d %d] "color I" [%s]\n' % (rng.integers(100, 450), rng.integers(300, 520), rng.integers(50, 300),
                                                                                 col(rng, 80000, 300000, 0)))
    if "spot" in lights:
        parts.append('LightSource "spot" "point from" [%d 540 %d] "point to" [%d 0 %d] "color I" [%s] "float coneangle" [%d] "float conedeltaangle" [%d]\n' % (
            rng.integers(150, 420), rng.integers(80, 300), rng.integers(150, 400), rng.integers(200, 450), col(rng, 300000, 600000, 0),
            rng.integers(20, 46), rng.integers(5, 16)))
    if "distant" in lights:
        parts.append('LightSource "distant" "point from" [%d 600 %d] "point to" [278 0 300] "color L" [%s]\n' % (
            rng.integers(-200, 700), rng.integers(-400, 200), col(rng, 1.0, 2.5)))
    objects = [PANEL_A, PANEL_B]
    xforms = ["", ""]
    f["sheet"] = bool(rng.random() < 0.4)
    if f["sheet"]:
        objects.append(SHEET); xforms.append("")
    f["mesh"] = bool(rng.random() < 0.4)
    if f["mesh"]:
        objects.append(scenes.smooth_mesh_text(radius=float(rng.integers(90, 170)), nu=12, nv=8, squash=(1.0, uni(rng, .7, 1.0, 2), 1.0)))
        xforms.append("Translate %d %d %d\n" % (rng.integers(180, 380), rng.integers(130, 220), rng.integers(150, 300)))
    first = int(rng.integers(0, len(mats)))
    used = set()
    for i, (shape, xf) in enumerate(zip(objects, xforms)):
        used.add((first + i) % len(mats))
        parts.append(obj(mats[(first + i) % len(mats)], shape, xf))
    f["soup"] = int(pick(rng, (0, 300, 3000)))
    if f["soup"]:
        parts.extend(obj(m, shape) for m, shape in zip(mats, tetra_soup(rng, f["soup"], len(mats))))
        used = set(range(len(mats)))
    f["materials"] = [k for i, k in enumerate(chosen) if i in used]        # (a drawn material that no object received is not in the scene)
    vol, vinfo = ("", {}) if f["medium"] == "none" else volume_text(rng, f["medium"], f["volume_integrator"] == "emission" or rng.random() < 0.3)
    f.update(vinfo)
    area = "area" in lights
    ns = int(rng.integers(1, 5))
    if base == "cornell":
        world = scenes.cornell_world(area_light=area, light_L=(17, 12, 4), light_nsamples=ns, extra="".join(parts) + vol)
    else:
        emitter = ""
        if area:
            emitter = ('AttributeBegin\nAreaLightSource "area" "color L" [17 12 4] "integer nsamples" [%d]\nMaterial "matte" "color Kd" [0 0 0]\n' % ns +
                       QUAD % scenes._fmt(scenes.CORNELL_LIGHT) + 'AttributeEnd\n')
        world = "WorldBegin\n" + "".join(parts) + obj('"matte" "color Kd" [.6 .6 .55]', FLOOR) + emitter + vol + "WorldEnd\n"
    text = scenes.options_block(**opts) + world
    if camera == "orthographic":
        win = "-300 300 -290 290" if base == "cornell" else "-420 420 -420 420"
        text, n = re.subn(r'Camera "perspective"[^\n]*\n', 'Camera "orthographic" "float screenwindow" [%s]\n' % win, text)
        assert n == 1
    elif camera == "environment":
        text = text.replace("LookAt 278 273 -800  278 273 0  0 1 0", "LookAt 278 273 200  278 273 600  0 1 0")
        text, n = re.subn(r'Camera "perspective"[^\n]*\n', 'Camera "environment"\n', text)
        assert n == 1
    return text, f


def bar_of(features):
    """The project's rule (tests/test_gpu_materials.py, tests/test_gpu_infinite.py) on triangle-only scenes."""
    return "strict" if features["integrator"] in ("whitted", "directlighting") and "infinite" not in features["lights"] else "loose"


# ---- the scene with one feature taken out
def without_infinite(text):
    out, n = INF_RE.subn("", text)
    assert n == 1, n
    return out


def as_homogeneous(text):
    """The density region replaced by the homogeneous region of the same constants (extent, transform, sigma_a, sigma_s, Le, g)."""
    def repl(m):
        line = m.group(0)
        keep = re.findall(r'"(?:point p0|point p1|color sigma_a|color sigma_s|color Le|float g)" \[[^\]]*\]', line)
        return 'Volume "homogeneous" ' + " ".join(keep) + "\n"
    out, n = re.subn(r'^Volume "(?:exponential|volumegrid)"[^\n]*\n', repl, text, flags=re.M)
    assert n == 1, n
    return out


def as_matte(text):
    out, n = re.subn(r'Material "(shinymetal|translucent)"', 'Material "matte"', text)
    assert n >= 1
    return out


def as_path(text):
    out, n = INTEGRATOR_RE.subn('SurfaceIntegrator "path" \n', text)
    assert n == 1, n
    return out


def ablations(text, f):
    out = {}
    if "infinite" in f["lights"]:
        out["infinite"] = without_infinite(text)
    if f["medium"] in ("exponential", "volumegrid"):
        out["density"] = as_homogeneous(text)
    if any(m in NEW_MATERIALS for m in f["materials"]):
        out["materials"] = as_matte(text)
    if f["integrator"] == "bidirectional":
        out["bidirectional"] = as_path(text)
    return out


def has_no_light(text):
    return "LightSource" not in text         # (matches AreaLightSource too)


def accept(REF, text, f):
    """(reason or None, rgb, alpha, stats, shares): the reference alone decides."""
    rgb, alpha, st = REF.run_reference(text, keyed=True)
    if st["stderr_lines"] != 0:
        return "the reference wrote %d stderr lines" % st["stderr_lines"], rgb, alpha, st, {}
    if not (np.isfinite(rgb).all() and np.isfinite(alpha).all()):
        return "non-finite film", rgb, alpha, st, {}
    lit = float((rgb.max(axis=-1) > 0).mean())
    if lit < MIN_LIT:
        return "only %.3f of the pixels are non-black" % lit, rgb, alpha, st, {}
    shares = {}
    for axis, other in ablations(text, f).items():
        if has_no_light(other) and ('SurfaceIntegrator "path"' in other or 'SurfaceIntegrator "bidirectional"' in other):
            # the reference's path and bidirectional integrators index lights[-1] in a scene without lights: it cannot render this one.  Without a light
            # or an emitter every radiance is zero: the film is black.
            orgb = np.zeros_like(rgb)
        else:
            orgb, _, ost = REF.run_reference(other, keyed=True)
        shares[axis] = float((np.sqrt(((rgb - orgb) ** 2).sum(-1)) > 1e-3).mean())
        if shares[axis] < MIN_SHARE:
            return "without %s only %.3f of the pixels differ" % (axis, shares[axis]), rgb, alpha, st, shares
    return None, rgb, alpha, st, shares


def coverage_gaps(feats):
    """The coverage table over the accepted fixtures' features: the list of cells that are not met (empty = the table holds)."""
    gaps = []
    def count(pred):
        return sum(1 for f in feats if pred(f))
    def need(what, pred, n=1):
        c = count(pred)
        if c < n:
            gaps.append("%s: %d < %d" % (what, c, n))
    dens = lambda f: f["medium"] in ("exponential", "volumegrid")
    newmat = lambda f: any(m in NEW_MATERIALS for m in f["materials"])
    inf = lambda f: "infinite" in f["lights"]
    bidir = lambda f: f["integrator"] == "bidirectional"
    for m in NEW_MATERIALS:
        for i in INTEGRATORS:
            need("%s under %s" % (m, i), lambda f: m in f["materials"] and f["integrator"] == i)
    for k in MEDIA:
        for i in INTEGRATORS[:3]:
            need("%s medium under %s" % (k, i), lambda f: f["medium"] == k and f["integrator"] == i)
        for v in ("emission", "single"):
            need("%s medium with %s" % (k, v), lambda f: f["medium"] == k and f["volume_integrator"] == v)
    for i in INTEGRATORS:
        need("infinite under %s" % i, lambda f: inf(f) and f["integrator"] == i)
    for s in ("all", "one"):
        need("infinite with strategy %s" % s, lambda f: inf(f) and f["strategy"] == s)
    need("infinite with a medium", lambda f: inf(f) and f["medium"] != "none", 2)
    for l in LIGHTS:
        need("bidirectional with %s light" % l, lambda f: bidir(f) and l in f["lights"])
    for s in ("stratified", "stratified_jitter", "lowdiscrepancy", "random"):
        need("bidirectional with %s sampler" % s, lambda f: bidir(f) and f["sampler"] == s)
    for a in ("kdtree", "grid"):
        need("bidirectional with %s" % a, lambda f: bidir(f) and f["accelerator"] == a)
    need("bidirectional with a non-perspective camera", lambda f: bidir(f) and f["camera"] in ("orthographic", "environment"))
    need("density medium x new material", lambda f: dens(f) and newmat(f), 3)
    need("density medium x infinite", lambda f: dens(f) and inf(f), 3)
    need("new material x infinite", lambda f: newmat(f) and inf(f), 3)
    need("strict fixtures", lambda f: bar_of(f) == "strict", 20)
    return gaps


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def main():
    REF = g.load_ref_runner()
    os.makedirs(OUT, exist_ok=True)
    for name in os.listdir(OUT):
        os.remove(os.path.join(OUT, name))
    manifest, feats = [], []
    seed = 0
    while True:
        text, f = mix_scene(seed)
        reason, rgb, alpha, st, shares = accept(REF, text, f)
        entry = dict(seed=seed, accepted=reason is None, reason=reason, bar=bar_of(f), features=f, shares=shares)
        if reason is None:
            path = os.path.join(OUT, "mix_%03d.npz" % seed)
            st = {k: v for k, v in st.items() if not k.endswith("_s")}          # (wall-clock times: the same run gives the same bytes without them)
            save_npz(path, scene=np.array(text), rgb=rgb, alpha=alpha, stats=np.array(json.dumps(st, sort_keys=True)),
                     features=np.array(json.dumps(f, sort_keys=True)), shares=np.array(json.dumps(shares, sort_keys=True)), bar=np.array(bar_of(f)))
            size = os.path.getsize(path)
            if size >= MAX_BYTES:
                os.remove(path)
                entry.update(accepted=False, reason="a fixture of %d bytes" % size)
            else:
                feats.append(f)
        manifest.append(entry)
        print(seed, "accepted" if entry["accepted"] else "REJECTED: " + entry["reason"], bar_of(f), f["integrator"], f["medium"], f["lights"], f["materials"], shares)
        seed += 1
        gaps = coverage_gaps(feats)
        if len(feats) >= WANT and not gaps:
            break
        assert len(feats) < HARD_STOP, "64 accepted fixtures and the coverage table is not met: %s" % gaps
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as fh:
        json.dump(dict(accepted=len(feats), tried=seed, seeds=manifest), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("accepted", len(feats), "of", seed, "seeds tried")


if __name__ == "__main__":
    main()
