"""The per-sample analytic cases: one table, read by tests/golden/make_analytic_golden.py (which renders the unmodified reference and
stores tests/golden/analytic/<case>.npz), tests/test_analytic_host.py and tests/test_gpu_analytic.py.  Each case is a scene of one or two
analytic surfaces under delta lights and SurfaceIntegrator "whitted", so that one camera sample is one evaluation of
f(wo, wi) Li |cos| (times transmittances); scene_text() writes it as a scene file, form() builds the float64 side (tests/analytic_forms.py).
Every case names the term it is there for and one wrong twin of its form that the fixture must reject."""
import numpy as np

import analytic_forms as F

RES = 64
COLORS = {"Kd", "Ks", "Kr", "Kt", "reflect", "transmit", "opacity", "I", "L", "sigma_a", "sigma_s", "Le"}
POINTS = {"from", "to", "p0", "p1", "p2"}
FAMILIES = ("lights", "lobes", "quadrics", "specular", "medium")

PLANE_CAM = dict(lookat=(0, 2, -6, 0, .6, 0, 0, 1, 0))
QUADRIC_CAM = dict(lookat=(0, 0, -4, 0, 0, 0, 0, 1, 0))
PLANE = ("quad", (-1000, 0, -1000, 1000, 0, -1000, 1000, 0, 1000, -1000, 0, 1000))
MATTE = ("matte", dict(Kd=(.7, .6, .5)))
POINT = dict(kind="point", I=(30, 25, 20), **{"from": (1, 3, 1)})
BEHIND = dict(kind="point", I=(30, 25, 20), **{"from": (1, -3, 1)})
SPOT = dict(kind="spot", I=(40, 35, 30), coneangle=38, conedeltaangle=20, **{"from": (0, 4, -1), "to": (.3, 0, 0)})
DISTANT = dict(kind="distant", L=(3, 2.5, 2), **{"from": (1, 2, -1), "to": (0, 0, 0)})
Q_LIGHTS = [dict(kind="distant", L=(1.6, 1.4, 1.2), **{"from": (-1, 1.5, -2), "to": (0, 0, 0)}),
            dict(kind="point", I=(9, 10, 12), **{"from": (2.5, 1, -3.5)})]
TILT = [("Rotate", -65, 1, 0, 0), ("Rotate", 150, 0, 0, 1)]


def plane_case(term, twin, lights, material=MATTE, family="lobes", **kw):
    return dict(family=family, term=term, twin=twin, camera=PLANE_CAM, lights=lights, surfaces=[dict(shape=PLANE, material=material)], **kw)


def quadric_case(term, twin, kind, params, ctm=TILT, **kw):
    surf = dict(shape=(kind, params), ctm=ctm, material=("matte", dict(Kd=(.7, .7, .6))), reverse=kw.pop("reverse", False))
    return dict(family="quadrics", term=term, twin=twin, camera=QUADRIC_CAM, lights=Q_LIGHTS, surfaces=[surf], **kw)


CASES = {
    # ---- lights on a matte plane that runs to the horizon
    "light_point": plane_case("point light: I / d^2", "no_inverse_square", [POINT], family="lights"),
    "light_spot": plane_case("spot light: the falloff ((cos - cosTotal) / (cosStart - cosTotal))^4", "falloff_cubed", [SPOT], family="lights",
                             min_falloff_share=.03),
    "light_distant": plane_case("distant light: constant L along Normalize(from - to)", "no_cosine", [DISTANT], family="lights"),
    "light_point_and_spot": plane_case("the loop over the lights", "first_light_only", [POINT, SPOT], family="lights"),
    "light_spot_ctm": plane_case("a spot light under Translate / Rotate / Scale: position and WorldToLight of the falloff", "spot_axis_untransformed",
                                 [dict(SPOT, ctm=[("Translate", .5, 0, 1), ("Rotate", 25, 0, 1, 0), ("Scale", 1.5, 1, .7)])], family="lights",
                                 min_falloff_share=.03),
    "light_grazing": plane_case("a light 0.1 above the plane: grazing wi", "no_cosine",
                                [dict(kind="point", I=(.05, .04, .03), **{"from": (0, .1, -1)})], family="lights"),
    # ---- lobes on the same plane under a point light
    "matte_sigma0": plane_case("Lambert", "no_cosine", [dict(kind="point", I=(14, 18, 24), **{"from": (-1.5, 2.5, 0)})], ("matte", dict(Kd=(.3, .5, .8)))),
    "matte_sigma20": plane_case("Oren-Nayar", "oren_nayar_without_b", [POINT], ("matte", dict(Kd=(.7, .6, .5), sigma=20))),
    "matte_sigma120": plane_case("Oren-Nayar: sigma clamped to 90", "sigma_unclamped", [POINT], ("matte", dict(Kd=(.7, .6, .5), sigma=120))),
    "plastic_rough_.2": plane_case("plastic: Lambert + Blinn microfacet, the torrance-sparrow geometric term", "no_geometric_term", [POINT],
                                   ("plastic", dict(Kd=(.4, .3, .2), Ks=(.5, .5, .4), roughness=.2))),
    "plastic_rough_.02": plane_case("plastic: the Blinn distribution's normalisation (e + 2) / (2 pi)", "blinn_normalised_by_e_plus_1", [POINT],
                                    ("plastic", dict(Kd=(.4, .3, .2), Ks=(.25, .2, .15), roughness=.02))),
    "plastic_rough_.0005": plane_case("plastic: the Blinn exponent capped at 1000", "exponent_uncapped",
                                      [dict(kind="point", I=(3400, 3000, 2400), **{"from": (2, 30, 50)})],      # far away: the highlight covers more of the frame
                                      ("plastic", dict(Kd=(.05, .04, .03), Ks=(.02, .015, .01), roughness=.0005))),
    "uber_opacity_.6": plane_case("uber: opacity-scaled lobes", "opacity_ignored", [POINT],
                                  ("uber", dict(Kd=(.5, .4, .3), Ks=(.4, .4, .3), opacity=(.6, .6, .6), roughness=.15))),
    "shinymetal": plane_case("shinymetal: FresnelApproxEta (clamp at .999) + FresnelConductor, k = 0", "eta_unclamped", [POINT],
                             ("shinymetal", dict(Ks=(.9995, .6, .3), roughness=.05))),
    "translucent_front": plane_case("translucent lit from the camera's side: the reflection lobes", "reflect_transmit_swapped", [POINT],
                                    ("translucent", dict(Kd=(.6, .5, .4), Ks=(.4, .4, .3), reflect=(.3, .3, .3), transmit=(.7, .7, .7), roughness=.1))),
    "translucent_behind": plane_case("translucent lit from behind: BRDFToBTDF of Lambert and Blinn microfacet", "reflect_transmit_swapped", [BEHIND],
                                     ("translucent", dict(Kd=(.6, .5, .4), Ks=(.4, .4, .3), reflect=(.3, .3, .3), transmit=(.7, .7, .7), roughness=.1))),
    "translucent_reflect_black": plane_case("translucent with reflect black: transmission lobes only", "normal_ignored", [BEHIND],
                                            ("translucent", dict(Kd=(.6, .5, .4), Ks=(.4, .4, .3), reflect=(0, 0, 0), transmit=(.7, .7, .7), roughness=.1))),
    "translucent_transmit_black": plane_case("translucent with transmit black: reflection lobes only", "reflect_transmit_swapped", [POINT],
                                             ("translucent", dict(Kd=(.6, .5, .4), Ks=(.4, .4, .3), reflect=(.6, .6, .6), transmit=(0, 0, 0), roughness=.1))),
    "translucent_kd_black": plane_case("translucent with Kd black: glossy transmission alone", "fresnel_one", [BEHIND],
                                       ("translucent", dict(Kd=(0, 0, 0), Ks=(.6, .5, .4), reflect=(.4, .4, .4), transmit=(.6, .6, .6), roughness=.2))),
    # ---- quadrics, matte, lit by a distant and a point light; each partial, so that the camera sees the inside through the cut
    "quadric_sphere": quadric_case("sphere: zmin / zmax / phimax, far root after a clipped near root", "near_root_always", "sphere",
                                   dict(radius=1.5, zmin=-1.1, zmax=.9, phimax=250)),
    "quadric_cylinder": quadric_case("cylinder under a non-uniform scale", "normal_not_renormalised", "cylinder", dict(radius=1, zmin=-1.2, zmax=1.2, phimax=250),
                                     ctm=TILT + [("Scale", 1.4, .8, 1)]),
    # (the apex, where the normal is undefined and its neighbourhood ill-conditioned, lies above the frame; the camera looks through the
    # mirror nappe beyond the apex, clipped by z > height, so every hit here is a far root)
    "quadric_cone": quadric_case("cone: the nappe beyond the apex clipped, the far root taken", "near_root_always", "cone", dict(radius=1.8, height=3.2, phimax=250),
                                 ctm=[("Translate", 0, -.6, 0)] + TILT + [("Translate", 0, 0, 2)]),
    "quadric_paraboloid": quadric_case("paraboloid under a non-uniform scale", "near_root_always", "paraboloid", dict(radius=1.3, zmin=.3, zmax=2.2, phimax=250),
                                       ctm=[("Translate", 0, -.8, 0)] + TILT + [("Scale", 1.2, .8, 1)]),
    "quadric_hyperboloid": quadric_case("hyperboloid", "near_root_always", "hyperboloid", dict(p1=(1.3, 0, -1.2), p2=(.5, .8, 1.2), phimax=250)),
    "quadric_disk_inner": quadric_case("disk with innerradius and phimax", "inner_radius_ignored", "disk", dict(height=.2, radius=1.7, innerradius=1.1, phimax=290),
                                       ctm=[("Rotate", -50, 1, 0, 0), ("Rotate", 30, 0, 0, 1)]),
    "quadric_sphere_reversed": quadric_case("ReverseOrientation", "near_root_always", "sphere", dict(radius=1.5, zmin=-1.1, zmax=.9, phimax=250), reverse=True,
                                            ctm=[("Rotate", -70, 1, 0, 0), ("Rotate", 170, 0, 0, 1)]),
    "quadric_cylinder_grid": quadric_case("the grid accelerator", "near_root_always", "cylinder", dict(radius=1.1, zmin=-1, zmax=1.3, phimax=240), accel="grid"),
    # ---- specular recursion
    "mirror_floor": dict(family="specular", term="mirror: Kr, Fresnel no-op, the reflected ray", twin="mirror_unlit", camera=PLANE_CAM, maxdepth=1,
                         lights=[dict(kind="point", I=(40, 35, 30), **{"from": (0, 3, 0)})],
                         surfaces=[dict(shape=PLANE, material=("mirror", dict(Kr=(.9, .8, .7)))),
                                   dict(shape=("quad", (-4, 0, 3, 4, 0, 3, 4, 5, 3, -4, 5, 3)), material=MATTE)]),
    # the slab is two outward-wound quads (top wound to face up, bottom to face down) and no sides: a ray that enters near the rim and passes the
    # bottom quad's edge goes on to the floor unrefracted; the form follows the geometry ray by ray, so such samples are in it.  The slab
    # reaches behind the camera: seen through an open NEAR side, light that is totally reflected twice inside the slab comes out black on 5 % of
    # the samples in the reference (and on the device alike), which the form does not explain; no camera ray of this case can take that path
    "glass_slab": dict(family="specular", term="glass: reflection and transmission with Fresnel, (et / ei)^2, the side from the winding", twin="glass_no_fresnel",
                       camera=PLANE_CAM, maxdepth=3, lights=[dict(kind="point", I=(3, 2.6, 2.2), **{"from": (.3, .5, -.5)})],
                       surfaces=[dict(shape=("quad", (-2, 1.2, -8, -2, 1.2, 1.5, 2, 1.2, 1.5, 2, 1.2, -8)), material=("glass", dict(Kr=(1, 1, 1), Kt=(.9, .95, 1), index=1.5))),
                                 dict(shape=("quad", (-2, 1, -8, 2, 1, -8, 2, 1, 1.5, -2, 1, 1.5)), material=("glass", dict(Kr=(1, 1, 1), Kt=(.9, .95, 1), index=1.5))),
                                 dict(shape=PLANE, material=MATTE)]),
    # ---- medium
    "medium_homogeneous": plane_case("homogeneous medium: transmittance of the camera segment and of the shadow segment, both clipped to the box",
                                     "shadow_unclipped", [POINT], family="medium", volume_integrator="emission",
                                     medium=dict(p0=(-3, 0, -2.5), p1=(3, 3.5, 4), sigma_a=(.05, .08, .12), sigma_s=(.1, .06, .03))),
}


# ---- the three camera probes: an orthographic camera with a screen window, an environment camera and a thin-lens perspective camera (under
# the unjittered 1 x 1 sampler its lens sample is (.5, .5), the lens centre, so the ray is closed form), 32 x 32, each looking at one of every
# quadric (partial, rotated, two under a non-uniform scale); the reference's probe integrator records every camera ray and its closest hit
def _probe_surfaces():
    m = ("matte", dict(Kd=(.5, .5, .5)))
    place = lambda x, y, z, *more: [("Translate", x, y, z), ("Rotate", -65, 1, 0, 0), ("Rotate", 150, 0, 0, 1)] + list(more)
    return [dict(shape=("sphere", dict(radius=1.5, zmin=-1.1, zmax=.9, phimax=250)), ctm=place(4, 0, 0), material=m),
            dict(shape=("disk", dict(height=.2, radius=1.7, innerradius=.8, phimax=290)), ctm=place(-4, .5, 0), material=m),
            dict(shape=("cylinder", dict(radius=1, zmin=-1.2, zmax=1.2, phimax=250)), ctm=place(0, 0, 4, ("Scale", 1.4, .8, 1)), material=m),
            dict(shape=("cone", dict(radius=1.4, height=2.4, phimax=250)), ctm=place(0, -3.5, -1), material=m),
            dict(shape=("paraboloid", dict(radius=1.3, zmin=.3, zmax=2.2, phimax=250)), ctm=place(0, 3.5, 1, ("Scale", 1.2, .8, 1)), material=m),
            dict(shape=("hyperboloid", dict(p1=(1.3, 0, -1.2), p2=(.5, .8, 1.2), phimax=250)), ctm=place(-3, -3, 3), material=m)]


PROBES = {
    "probe_ortho_quadrics": dict(camera=dict(kind="orthographic", lookat=(3, 4, -20, 0, 0, 0, 0, 1, 0), screenwindow=(-7, 7, -6, 5), res=(32, 32)),
                                 lights=[], surfaces=_probe_surfaces(), twin=None),
    "probe_env_quadrics": dict(camera=dict(kind="environment", lookat=(.3, .2, -.4, 0, .5, 1, 0, 1, 0), res=(32, 32)),
                               lights=[], surfaces=_probe_surfaces(), twin=None),
    "probe_lens_quadrics": dict(camera=dict(kind="perspective", fov=55, lookat=(2, 3, -12, 0, 0, 0, 0, 1, 0), lensradius=.4, focaldistance=11, res=(32, 32)),
                                lights=[], surfaces=_probe_surfaces(), twin=None),
}


def _fmt(v):
    return " ".join("%.9g" % float(np.float32(x)) for x in np.atleast_1d(v))


def _params(d, skip=("kind", "ctm")):
    out = []
    for k, v in d.items():
        if k in skip:
            continue
        typ = "color" if k in COLORS else "point" if k in POINTS else "float"
        out.append('"%s %s" [%s]' % (typ, k, _fmt(v)))
    return " ".join(out)


def _ctm_text(ctm):
    return "".join("%s %s\n" % (op[0], _fmt(op[1:])) for op in ctm)


def _ctm(ctm):
    ops = {"Translate": F.translate, "Rotate": F.rotate, "Scale": F.scale}
    return F.compose(*[ops[op[0]](*op[1:]) for op in ctm])


def scene_text(name, jitter=False, seed=7, probe_dump=None):
    """the scene file of a case: unjittered, one sample per pixel at the pixel centre, under a box filter of width .5 (a film pixel is
    then its one sample); jitter=True: stratified 2 x 2 jittered samples from the keyed seed (the product's own sampler parameter).
    A probe scene (PROBES) names the oracle-side "probe" integrator, which dumps one record per camera ray to `probe_dump`."""
    c = CASES[name] if name in CASES else PROBES[name]
    cam = c["camera"]
    xres, yres = cam.get("res", (RES, RES))
    out = ["LookAt %s\n" % _fmt(cam["lookat"])]
    kind = cam.get("kind", "perspective")
    extra = (' "float fov" [%s]' % _fmt(cam.get("fov", 60))) if kind == "perspective" else ""
    if "screenwindow" in cam:
        extra += ' "float screenwindow" [%s]' % _fmt(cam["screenwindow"])
    if "lensradius" in cam:
        extra += ' "float lensradius" [%s] "float focaldistance" [%s]' % (_fmt(cam["lensradius"]), _fmt(cam["focaldistance"]))
    out.append('Camera "%s"%s\n' % (kind, extra))
    out.append('Film "image" "integer xresolution" [%d] "integer yresolution" [%d] "string filename" ["out.exr"]\n' % (xres, yres))
    if jitter:
        out.append('Sampler "stratified" "integer seed" [%d] "integer xsamples" [2] "integer ysamples" [2] "bool jitter" ["true"]\n' % seed)
    else:
        out.append('Sampler "stratified" "integer xsamples" [1] "integer ysamples" [1] "bool jitter" ["false"]\n')
    out.append('PixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n')
    if name in PROBES:
        out.append('SurfaceIntegrator "probe" "string dump" ["%s"] "point target" [0 50 0]\n' % (probe_dump or "probe_rays.bin"))
    else:
        out.append('SurfaceIntegrator "whitted" "integer maxdepth" [%d]\n' % c.get("maxdepth", 0))
    if c.get("volume_integrator"):
        out.append('VolumeIntegrator "%s"\n' % c["volume_integrator"])
    out.append('Accelerator "%s"\nWorldBegin\n' % c.get("accel", "kdtree"))
    for l in c["lights"]:
        out.append("AttributeBegin\n%sLightSource \"%s\" %s\nAttributeEnd\n" % (_ctm_text(l.get("ctm", [])), l["kind"], _params(l)))
    for s in c["surfaces"]:
        kind, sp = s["shape"]
        out.append("AttributeBegin\n" + _ctm_text(s.get("ctm", [])) + ("ReverseOrientation\n" if s.get("reverse") else ""))
        out.append('Material "%s" %s\n' % (s["material"][0], _params(s["material"][1])))
        if kind == "quad":
            out.append('Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [%s]\n' % _fmt(sp))
        else:
            out.append('Shape "%s" %s\n' % (kind, _params(sp)))
        out.append("AttributeEnd\n")
    if c.get("medium"):
        out.append('Volume "homogeneous" %s\n' % _params(c["medium"]))
    out.append("WorldEnd\n")
    return "".join(out)


def camera_form(cam):
    xres, yres = cam.get("res", (RES, RES))
    return F.Camera(cam.get("kind", "perspective"), xres, yres, F.look_at(cam["lookat"][0:3], cam["lookat"][3:6], cam["lookat"][6:9]), fov=cam.get("fov", 60),
                    screen=cam.get("screenwindow"), lensradius=cam.get("lensradius", 0.0), focaldistance=cam.get("focaldistance", 1e30))


MATERIAL_TWINS = {"fresnel_one", "blinn_normalised_by_e_plus_1", "no_geometric_term", "sigma_unclamped", "oren_nayar_without_b", "opacity_ignored", "exponent_uncapped", "eta_unclamped",
                  "reflect_transmit_swapped", "normal_ignored"}
SHAPE_TWINS = {"normal_not_renormalised", "inner_radius_ignored"}
LIGHT_TWINS = {"spot_axis_untransformed"}


def form(name, wrong=False):
    """the float64 side of a case (analytic_forms.Scene); wrong=True: its wrong twin"""
    c = CASES[name] if name in CASES else PROBES[name]
    twin = c["twin"] if wrong else None
    camera = camera_form(c["camera"])
    lights = []
    for l in c["lights"]:
        col = l["L"] if l["kind"] == "distant" else l["I"]
        lights.append(F.Light(l["kind"], col, _ctm(l.get("ctm", [])), l.get("from", (0, 0, 0)), l.get("to", (0, 0, 1)), l.get("coneangle", 30), l.get("conedeltaangle", 5),
                              twin=twin if twin in LIGHT_TWINS else None))
    surfaces = []
    for s in c["surfaces"]:
        kind, sp = s["shape"]
        m = _ctm(s.get("ctm", []))
        shape = F.Quad(sp, m) if kind == "quad" else F.Quadric(kind, m, twin=twin if twin in SHAPE_TWINS else None, **sp)
        surfaces.append((shape, F.Material(s["material"][0], twin=twin if twin in MATERIAL_TWINS else None, **s["material"][1])))
    med = c.get("medium")
    medium = F.Medium(med["p0"], med["p1"], med["sigma_a"], med["sigma_s"]) if med else None
    return F.Scene(camera, surfaces, lights, medium, c.get("maxdepth", 0), twin=twin if twin not in MATERIAL_TWINS | SHAPE_TWINS | LIGHT_TWINS else None)


def pixel_centres(xres=RES, yres=RES):
    """image positions of the unjittered samples in the sampler's (scanline) order: the sample extent of a 64 x 64 film under a filter of
    width .5 is 65 x 65 (the last row and column lie off the film)"""
    iy, ix = np.mgrid[0:yres + 1, 0:xres + 1]
    return ix + .5, iy + .5


# ------------------------------------------------------------------------------------------------ the measure, the band, the bars
BAND_CAP = 0.03             # at most 3 % of a case's samples may be in the band: a condition, not a measurement
BAR_FACTOR = 4.0            # the device's powf / sinf / cosf / acosf / atan2f / division differ from glibc's in the last bits
MIN_TWIN_SHARE = 0.05       # the wrong twin must differ on this share of the included samples by 10 x the bar


def measure(name, rgb, alpha):
    """a film of the unjittered scene (one sample per pixel at its centre) against the float64 form: band, ref_err and what the generator prints"""
    ix, iy = pixel_centres()
    ix, iy = ix[:RES, :RES], iy[:RES, :RES]
    sc = form(name)
    L, hit, _ = sc.samples(ix, iy)
    band = F.band(sc, ix, iy)
    inc = ~band
    e = F.sample_error(rgb, L, inc)
    o, d, mint, maxt = sc.camera.rays(ix, iy)
    t, n, idx, root = sc.closest(o, d, mint, maxt)
    falloff = 0.0
    spots = [l for l in sc.lights if l.kind == "spot"]
    if spots and hit.any():
        p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
        falloff = float((spots[0].sample(p)[3] == 1)[hit > 0].mean())
    return dict(band=band, band_share=float(band.mean()), ref_err=float(e[inc].max()), hit_share=float(hit.mean()), lcase=float(np.abs(L[inc]).max()),
                alpha_equal=bool(np.array_equal(alpha[inc], hit[inc].astype(np.float32))), far_root_share=float(((root == 1) & (hit > 0)).mean()),
                falloff_share=falloff, L=L, e=e)


def bar(name, ref_errs):
    """4 x max(ref_err of the case, median ref_err over the case's family): the reference's own deviation from float64 is the scale"""
    fam = [v for n, v in ref_errs.items() if CASES[n]["family"] == CASES[name]["family"]]
    return BAR_FACTOR * max(ref_errs[name], float(np.median(fam)))


def twin_share(name, rgb, band, bar_value):
    """the share of the included samples on which the reference's film lies beyond 10 x the bar from the case's wrong twin"""
    ix, iy = pixel_centres()
    L, _, _ = form(name, wrong=True).samples(ix[:RES, :RES], iy[:RES, :RES])
    inc = ~band
    return float((F.sample_error(rgb, L, inc)[inc] > 10 * bar_value).mean())


def measure_probe(name, rec):
    """the reference's probe records (20 floats per camera ray: o d mint maxt | hit t p n u v | ..) of a probe scene against the float64
    camera and intersectors: the camera's deviation (what the device's rt_camera_rays is held to, times BAR_FACTOR), and outside the band
    of analytic_forms.ray_band the hit's t, point, normal (up to its sign) and (u, v)"""
    sc = form(name)
    xres, yres = PROBES[name]["camera"]["res"]
    ix, iy = pixel_centres(xres, yres)
    o, d, mint, maxt = sc.camera.rays(ix.ravel(), iy.ravel())
    ro, rd = rec[:, 0:3].astype(np.float64), rec[:, 3:6].astype(np.float64)
    out = dict(dev_o=float(np.abs(ro - o).max() / np.abs(o).max()), dev_d=float(np.abs(rd - d).max()),
               mint_equal=bool(np.array_equal(rec[:, 6], mint.astype(np.float32))), maxt_equal=bool(np.allclose(rec[:, 7], maxt, rtol=2.0 ** -22, atol=0)))       # (yon - hither) / d.z: a float32 division of a rounded d.z
    # the hits of the reference's own rays
    t, n, idx, root = sc.closest(ro, rd, rec[:, 6].astype(np.float64), rec[:, 7].astype(np.float64))
    band = F.ray_band(sc, ro, rd, rec[:, 6].astype(np.float64), rec[:, 7].astype(np.float64))
    inc = ~band
    hit = idx >= 0
    both = inc & hit & (rec[:, 8] > 0)
    p = ro + np.where(hit, t, 0.0)[:, None] * rd
    u, v = np.zeros(len(rec)), np.zeros(len(rec))
    for i, (shape, _) in enumerate(sc.surfaces):
        sel = both & (idx == i)
        if sel.any():
            u[sel], v[sel] = shape.uv(p[sel])
    rn = rec[:, 13:16].astype(np.float64)
    out.update(band=band, band_share=float(band.mean()), hit_equal=bool(np.array_equal(hit[inc], rec[inc, 8] > 0)), hit_share=float(hit.mean()),
               kinds_hit=sorted({sc.surfaces[i][0].kind for i in np.unique(idx[both])}), far_root_share=float((root[both] == 1).mean()),
               dev_t=float((np.abs(rec[both, 9] - t[both]) / t[both]).max()),
               dev_p=float((np.abs(rec[both, 10:13] - p[both]).max(-1) / t[both]).max()),
               dev_n=float(np.minimum(np.abs(rn - n).max(-1), np.abs(rn + n).max(-1))[both].max()),
               dev_uv=float(max(np.abs(rec[both, 16] - u[both]).max(), np.abs(rec[both, 17] - v[both]).max())))
    return out
