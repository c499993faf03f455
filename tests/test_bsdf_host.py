"""The fixtures of tests/golden/bsdf/ (the reference's answers to BSDF queries, tests/golden/make_bsdf_golden.py) against the float64 forms of
tests/bsdf_forms.py, on the CPU: the stored ref_err is the forms' distance from the reference and nothing else, the exclusion rule stays under the
project's cap, the integer outputs agree, every wrong twin is told from the truth, the forms agree with analytic_forms.Material.f, and the Python
side of the call (structure, constants) matches the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import analytic_cases as A
import analytic_forms as F
import bsdf_cases as BC
import bsdf_forms as B
from conftest import GOLDEN, ROOT

CASES = list(BC.CASES)
_memo = {}


def fixture(name):
    if name not in _memo:
        z = np.load(os.path.join(GOLDEN, "bsdf", name + ".npz"))
        fx = {k: z[k] for k in z.files}
        _memo[name] = (fx, BC.ref_err(name, fx, fx["answers"]))
    return _memo[name]


def bar(name, output):
    """the GPU test's bar: 4 x max(ref_err(case, output), the median ref_err of that output over the cases)"""
    i = BC.OUTPUTS.index(output)
    return A.BAR_FACTOR * max(float(fixture(name)[0]["ref_err"][i]), float(np.median([fixture(c)[0]["ref_err"][i] for c in CASES])))


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_what_the_generator_makes_of_the_case(name):
    fx, _ = fixture(name)
    assert str(fx["scene"]) == BC.scene_text(name)
    q = BC.queries(name, int(fx["seed"]))
    for k, v in q.items():
        assert v.dtype == fx[k].dtype and np.array_equal(v, fx[k]), (name, k)
    n = len(fx["ridx"])
    assert n <= 4096 and fx["answers"].shape == (n, 36) and fx["answers"].dtype == np.float32
    assert os.path.getsize(os.path.join(GOLDEN, "bsdf", name + ".npz")) < 320 * 1024
    # the special points of the sampling maps are among the queries
    top = np.float32(1) - np.float32(2.0 ** -24)
    for a in (0, .5, top):
        for b in (0, .5, top):
            for c in (0, top):
                assert ((fx["u"] == np.array([a, b, c], np.float32)).all(-1)).sum() >= 2, (a, b, c)
    assert set(np.unique(fx["flags"])) == set(B.FLAG_CYCLE)
    assert np.abs(np.linalg.norm(fx["rays"][:, 3:6].astype(np.float64), axis=-1) - 1).max() < 1e-7
    miss = 1 - (fx["answers"][:, 0] > 0).mean()
    assert .03 <= miss <= .45, miss


@pytest.mark.parametrize("name", CASES)
def test_ref_err_is_the_references_distance_from_the_float64_forms(name):
    """recomputed here and equal to what the fixture stores (to the last digits a matrix product may differ in); small enough that the forms lack no
    term; the left-out share is the stored one and under the cap; s_type and n_components are the forms' on every included query"""
    fx, (err, left_out, w) = fixture(name)
    inc = ~w["excluded"]
    print("BSDF-FORM %s left out %.4f %s" % (name, left_out, {k: "%.3g" % v for k, v in err.items()}))
    assert left_out <= A.BAND_CAP and left_out == pytest.approx(float(fx["left_out"]), abs=1e-12)
    for i, k in enumerate(BC.OUTPUTS):
        assert err[k] == pytest.approx(float(fx["ref_err"][i]), rel=1e-6, abs=1e-12), (name, k)
        assert err[k] < 2e-3, (name, k, err[k])
    ans = fx["answers"]
    assert np.array_equal(BC.answer(ans, "s_type")[inc], w["s_type"][inc])
    assert np.array_equal(BC.answer(ans, "n_components")[inc], w["n_components"][inc])
    assert np.array_equal(BC.answer(ans, "n_lobes")[inc & w["hit"]] > 0, np.ones(int((inc & w["hit"]).sum()), bool))
    # a miss is all zeros in the reference's record too
    assert not ans[~w["hit"], 1:].any()


def test_cases_cover_what_they_are_for():
    """all seven materials; every lobe type sampled; both accelerators; transmission across a sheet where the normals disagree; total internal
    reflection; textured parameters that vary over the hits; emitters seen from both sides"""
    types = set()
    for name in CASES:
        fx, (_, _, w) = fixture(name)
        types |= set(np.unique(w["s_type"][~w["excluded"]]))
    assert types == {0, B.REFLECTION | B.DIFFUSE, B.REFLECTION | B.GLOSSY, B.REFLECTION | B.SPECULAR, B.TRANSMISSION | B.DIFFUSE, B.TRANSMISSION | B.GLOSSY,
                     B.TRANSMISSION | B.SPECULAR}
    assert {s["material"][0] for s in BC.CASES["gallery_flat"]["surfaces"]} == {"matte", "plastic", "uber", "shinymetal", "translucent", "mirror", "glass"}
    assert BC.CASES["gallery_smooth_grid"]["accel"] == "grid" and 'Accelerator "grid"' in str(fixture("gallery_smooth_grid")[0]["scene"])
    # uber with all four lobes, translucent with all four
    fx, (_, _, w) = fixture("gallery_flat")
    assert (BC.answer(fx["answers"], "n_lobes") == 4).sum() > 200
    # total internal reflection: the glass quad asked for its transmission lobe alone and refusing
    glass_t = (fx["flags"] == (B.TRANSMISSION | B.SPECULAR)) & (BC.answer(fx["answers"], "n_lobes") == 2) & w["hit"] & ~w["excluded"]
    assert (w["s_pdf"][glass_t] == 0).sum() > 5 and (w["s_pdf"][glass_t] > 0).sum() > 5
    # the shading and the geometric normal disagree about the hemisphere of part of the wi
    fx, (_, _, w) = fixture("gallery_smooth_grid")
    a = fx["answers"]
    wi = fx["wi"].astype(np.float64)
    disagree = w["hit"] & ~w["excluded"] & ((wi * BC.answer(a, "ng")).sum(-1) * (wi * BC.answer(a, "nn")).sum(-1) < 0)
    assert disagree.sum() > 10
    # textured: the resolved parameters differ from hit to hit (f of one flag class takes many values per surface)
    fx, (_, _, w) = fixture("gallery_textured")
    assert len(np.unique(np.round(w["f"][w["hit"] & (fx["flags"] == 31)], 4), axis=0)) > 100
    # emitters: both answers of Le on quads and on spheres
    fx, (_, _, w) = fixture("gallery_emitters")
    lit = np.abs(w["le"]).max(-1) > 0
    assert (lit & w["hit"]).sum() > 300 and (~lit & w["hit"]).sum() > 300
    assert len(np.unique(w["le"][lit], axis=0)) == 2


@pytest.mark.parametrize("output,twin,name", [(o, t, c) for o, lst in BC.TWINS.items() for t, c in lst])
def test_wrong_twin_exceeds_the_bar_on_the_references_values(output, twin, name):
    fx, (_, _, w) = fixture(name)
    inc = ~w["excluded"]
    wrong = BC.evaluate(name, fx, fx["answers"], twin=twin)
    ans = fx["answers"]
    if output in ("s_type", "n_components"):
        differ = int((BC.answer(ans, output)[inc] != wrong[output][inc]).sum())
        print("BSDF-TWIN %s %s %s differing %d" % (output, twin, name, differ))
        assert differ > 10
        return
    e = B.query_error(BC.answer(ans, output), wrong[output], inc, unit_scale=(output == "s_wi"))[inc]
    print("BSDF-TWIN %s %s %s e %.3g on %d queries, bar %.3g" % (output, twin, name, e.max(), int((e > bar(name, output)).sum()), bar(name, output)))
    assert e.max() > bar(name, output) and (e > bar(name, output)).sum() >= 3       # (Blinn's zero is reached by three of the flat case's samples; every other twin by dozens)


def test_the_forms_f_is_analytic_forms_material_f():
    """with one normal for the geometry and the shading and flags = ALL, Bsdf.f is Material.f -- the form tests/test_analytic_host.py holds the
    reference's films to -- for the five materials that answer f"""
    rng = np.random.default_rng(5)
    n = 2000
    nn = F._norm(rng.standard_normal((n, 3)))
    dpdu = np.cross(nn, F._norm(rng.standard_normal((n, 3))))
    wo, wi = F._norm(rng.standard_normal((n, 3))), F._norm(rng.standard_normal((n, 3)))
    for s in BC.CASES["gallery_flat"]["surfaces"]:
        kind, kw = s["material"]
        if kind in ("mirror", "glass"):
            continue
        got = B.Bsdf(kind, kw, nn, dpdu, nn).f(wo, wi, np.full(n, B.ALL))
        want = F.Material(kind, **kw).f(wo, wi, nn)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), kind
        # ... and the four flag classes partition it
        parts = sum(B.Bsdf(kind, kw, nn, dpdu, nn).f(wo, wi, np.full(n, fl)) for fl in (B.REFLECTION | B.DIFFUSE, B.REFLECTION | B.GLOSSY, B.TRANSMISSION | B.DIFFUSE, B.TRANSMISSION | B.GLOSSY))
        assert np.abs(parts - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), kind


def test_sampled_pdf_is_the_pdf_of_the_sampled_direction():
    """the forms' own consistency: Sample_f's pdf equals Pdf(wo, s_wi, flags) for a non-specular sample, and f at s_wi is s_f.  (A glossy lobe that drew
    a direction in the other hemisphere keeps Blinn's pdf in Sample_f, reflection.cpp:235-240, where Pdf gives 0, :241-245: those are left out.)"""
    rng = np.random.default_rng(6)
    n = 3000
    nn = F._norm(rng.standard_normal((n, 3)))
    dpdu = np.cross(nn, F._norm(rng.standard_normal((n, 3))))
    wo, u = F._norm(rng.standard_normal((n, 3))), rng.random((n, 3))
    for s in BC.CASES["gallery_flat"]["surfaces"]:
        kind, kw = s["material"]
        b = B.Bsdf(kind, kw, nn, dpdu, nn)
        flags = np.full(n, B.ALL & ~B.SPECULAR)
        smp = b.sample(wo, u, flags)
        ok = smp["s_pdf"] > 0
        if kind in ("mirror", "glass"):
            assert not ok.any()
            continue
        side = (wo * nn).sum(-1) * (smp["s_wi"] * nn).sum(-1)
        # (... and so is a transmitted glossy sample: BRDFToBTDF::Sample_f mirrors the drawn direction in z, :67-72, where its Pdf asks at -wi, :231-234)
        ok &= ~(((smp["s_type"] == (B.REFLECTION | B.GLOSSY)) & (side <= 0)) | (smp["s_type"] == (B.TRANSMISSION | B.GLOSSY)))
        assert ok.mean() > .6, kind
        assert np.abs(b.pdf(wo, smp["s_wi"], flags)[ok] - smp["s_pdf"][ok]).max() <= 1e-9 * smp["s_pdf"][ok].max(), kind
        assert np.abs(b.f(wo, smp["s_wi"], flags)[ok] - smp["s_f"][ok]).max() <= 1e-9 * max(1.0, np.abs(smp["s_f"][ok]).max()), kind


def test_python_side_matches_the_header(pkg):
    """RtBsdfQuery: eleven pointers in the header's order; the BSDF_* constants are the header's enum and bsdf_forms'"""
    head = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    body = re.search(r"typedef struct RtBsdfQuery \{(.*?)\} RtBsdfQuery;", head, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*\s*(\w+)", decl)]
    assert names == [f for f, _ in pkg.RtBsdfQuery._fields_] and C.sizeof(pkg.RtBsdfQuery) == 11 * C.sizeof(C.c_void_p)
    enum = dict(re.findall(r"RT_(BSDF_\w+) = (\d+)", head))
    assert enum and all(getattr(pkg, k) == int(v) for k, v in enum.items())
    assert (pkg.BSDF_REFLECTION, pkg.BSDF_TRANSMISSION, pkg.BSDF_DIFFUSE, pkg.BSDF_GLOSSY, pkg.BSDF_SPECULAR, pkg.BSDF_ALL) == \
           (B.REFLECTION, B.TRANSMISSION, B.DIFFUSE, B.GLOSSY, B.SPECULAR, B.ALL)
    assert "int rt_bsdf_device(RtScene *s, const RtRay *dev_rays, const RtHit *dev_hits, uint32_t n, const RtBsdfQuery *q);" in head
    assert pkg.BSDF_FIELDS == ("f", "pdf", "s_wi", "s_f", "s_pdf", "s_type", "n_components", "le")
