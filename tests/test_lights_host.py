"""The fixtures of tests/golden/lights/ (the reference's answers to light queries, tests/golden/make_light_golden.py) against the float64 forms of
tests/light_forms.py, on the CPU: the stored ref_err is the forms' distance from the reference and nothing else, the exclusion rule stays under the
project's cap, the discrete outputs agree, every light, triangle, zone and branch is reached; and the library's side of the call: the header's
declaration, the exported symbol, the ctypes structure, the kernel's resource report, the parsed scenes' light order and the wrapper's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import analytic_cases as A
import light_cases as LC
import light_forms as LF
from conftest import GOLDEN, ROOT

CASES = list(LC.CASES)
_memo = {}


def fixture(name):
    if name not in _memo:
        z = np.load(os.path.join(GOLDEN, "lights", name + ".npz"))
        fx = {k: z[k] for k in z.files}
        _memo[name] = (fx, LC.ref_err(name, fx, fx["answers"], int(fx["seed"])))
    return _memo[name]


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_what_the_generator_makes_of_the_case(name):
    fx, _ = fixture(name)
    assert str(fx["scene"]) == LC.scene_text(name) and int(fx["seed"]) == LC.SEED
    q = LC.queries(name)
    for k, v in q.items():
        assert v.dtype == fx[k].dtype and np.array_equal(v, fx[k]), (name, k)
    n = len(fx["p"])
    assert n <= 4096 and fx["answers"].shape == (n, 24) and fx["answers"].dtype == np.float32
    assert os.path.getsize(os.path.join(GOLDEN, "lights", name + ".npz")) < 320 * 1024
    # u1 at 0 and at 1 - 2^-24 are among the queries of every light, in both forms
    for l in range(len(LC.CASES[name])):
        for wn in (0, 1):
            sel = (fx["light"] == l) & (fx["with_normal"] == wn)
            assert (fx["u"][sel, 0] == 0).sum() >= 2 and (fx["u"][sel, 0] == LC.TOP).sum() >= 2, (name, l, wn)
    assert np.abs(np.linalg.norm(fx["wi"].astype(np.float64), axis=-1) - 1).max() < 1e-6


@pytest.mark.parametrize("name", CASES)
def test_ref_err_is_the_references_distance_from_the_float64_forms(name):
    """recomputed here and equal to what the fixture stores; small enough that the forms lack no term; the left-out share is the stored one and under
    the cap; draws, IsDeltaLight, the shadow ray's mint and maxt and which outputs are zero are the forms' on every included query; and every light,
    emitter triangle, spot zone, sphere branch and side of the z flip is reached by an included query"""
    fx, (err, left_out, w) = fixture(name)
    inc = ~w["excluded"]
    print("LIGHT-FORM %s left out %.4f %s" % (name, left_out, {k: "%.3g" % v for k, v in err.items()}))
    assert left_out <= A.BAND_CAP and left_out == pytest.approx(float(fx["left_out"]), abs=1e-12)
    for i, k in enumerate(LC.OUTPUTS):
        assert err[k] == pytest.approx(float(fx["ref_err"][i]), rel=1e-6, abs=1e-12), (name, k)
        assert err[k] < 2e-3, (name, k, err[k])
    ans = fx["answers"]
    for k in ("s_draws", "is_delta", "mint", "maxt"):
        assert np.array_equal(LC.answer(ans, k)[inc], w[k][inc]), (name, k)
    zero = lambda a: ~np.asarray(a).reshape(len(a), -1).any(-1)
    for k in LC.OUTPUTS:
        assert np.array_equal(zero(LC.answer(ans, k))[inc], zero(w[k])[inc]), (name, k)
    assert not LC.coverage(name, fx, w)


def test_cases_cover_what_they_are_for():
    fx, (_, _, w) = fixture("emitters_tri")
    inc, ans = ~w["excluded"], fx["answers"]
    # the tent: Pdf directions that cross both triangles, and the last one of the set is the one that answers
    tent = LF.TriEmitter(LC.world_tris(LC.CASES["emitters_tri"][3]), False, (1, 1, 1))
    sel = inc & (fx["light"] == 3)
    p, wi = fx["p"][sel].astype(np.float64), fx["wi"][sel].astype(np.float64)
    only = [LF.TriEmitter(tent.t[k:k + 1][::-1], False, (1, 1, 1)).shape_pdf(p, wi)[2] >= 0 for k in (0, 1)]
    both = only[0] & only[1]
    assert both.sum() >= 10 and (tent.shape_pdf(p, wi)[2][both] == 1).all()
    # points in the plane of the one-triangle emitter: pdf = 0 in the reference, black L, and the sample is still returned
    flat = inc & (fx["light"] == 0) & (fx["p"][:, 2] == 0)
    assert flat.sum() >= 20 and not LC.answer(ans, "s_pdf")[flat].any() and not LC.answer(ans, "s_L")[flat].any()
    assert (np.abs(LC.answer(ans, "s_wi")[flat]).max(-1) > 0).all()
    # both sides of every emitter: black and lit samples
    for l in range(4):
        lit = LC.answer(ans, "s_L")[inc & (fx["light"] == l)].any(-1)
        assert lit.sum() > 20 and (~lit).sum() > 20, l
    # Pdf directions that miss
    assert (LC.answer(ans, "pdf")[inc] == 0).sum() > 100 and (LC.answer(ans, "pdf")[inc] > 0).sum() > 100
    # the lights are listed in mixed order
    assert [l["kind"] for l in LC.CASES["delta"]] == ["spot", "distant", "point"]
    assert [l["kind"] for l in LC.CASES["infinite"]] == ["point", "infinite", "tri"]


def test_keyed_draw_is_the_streams_definition():
    """light_forms.keyed_draw against the definition written out for single values (oracle/ref/keyed_rng.cpp)"""
    def pcg(v):
        s = (v * 747796405 + 2891336453) & 0xFFFFFFFF
        w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
        return ((w >> 22) ^ w) & 0xFFFFFFFF
    for key, ctr, seed in ((0, 0, 0), (7, 3, 5), (0xFFFFFFF3, 6, 5), (123456, 1, 0xFFFFFFFF)):
        want = np.float32((pcg((ctr + pcg((key + seed * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF) & 0xFFFFFF) / float(1 << 24))
        assert LF.keyed_draw(np.array([key]), np.array([ctr]), seed)[0] == want


def test_python_side_matches_the_header(pkg):
    """RtLightQuery: the header's fields in the header's order, its size and offsets as the C compiler lays them out (pointers, one uint32 padded to 8)"""
    head = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    assert "int rt_light_device(RtScene *s, uint32_t n, const RtLightQuery *q);" in head
    body = re.search(r"typedef struct RtLightQuery \{(.*?)\} RtLightQuery;", head, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f for f, _ in pkg.RtLightQuery._fields_], names
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(pkg.RtLightQuery) == 15 * ptr
    want = {n: i * ptr for i, n in enumerate(("p", "nrm", "light", "u", "rng", "wi", "seed", "s_wi", "s_L", "s_pdf", "s_ray", "s_draws", "pdf", "le", "is_delta"))}
    assert {n: getattr(pkg.RtLightQuery, n).offset for n in want} == want
    assert getattr(pkg.RtLightQuery, "seed").size == 4
    assert pkg.LIGHT_FIELDS == ("s_wi", "s_L", "s_pdf", "s_ray", "s_draws", "pdf", "le", "is_delta")
    lib = C.CDLL(pkg.HIP_LIB)
    assert lib.rt_light_device is not None


def test_the_kernels_resource_report(pkg):
    """lib/obj/rt_light.resources.txt: light_query_kernel takes no scratch and no LDS"""
    path = os.path.join(os.path.dirname(pkg.HIP_LIB), "obj", "rt_light.resources.txt")
    text = open(path).read()
    assert "light_query_kernel" in text
    block = text[text.index("light_query_kernel"):]
    scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
    lds = re.search(r"LDS Size \[bytes/block\]: (\d+)", block)
    assert scratch and lds and int(scratch.group(1)) == 0 and int(lds.group(1)) == 0, block[:1200]


@pytest.mark.parametrize("name", CASES)
def test_parsed_scene_lists_the_lights_in_the_cases_order(pkg, name):
    ps = pkg.ParsedScene(text=LC.product_text(LC.scene_text(name)))
    assert ps.valid and ps.errors == 0
    kinds = {"tri": "area", "sphere": "area", "disk": "area", "cylinder": "area"}
    assert [l["type"] for l in ps.lights()] == [kinds.get(l["kind"], l["kind"]) for l in LC.CASES[name]]
    assert ps.render_view()["seed"] == LC.SEED
    for got, l in zip(ps.lights(), LC.CASES[name]):
        if l["kind"] == "tri":
            assert got["n_tris"] == len(l["indices"]) // 3


def test_wrapper_refuses_wrong_tensors_before_the_library(pkg):
    """DeviceScene.light's own checks need no device: dtype, shape, contiguity, missing inputs and unknown fields raise ValueError (a scene object that
    was never opened stands in: the checks come before anything touches it)"""
    import torch
    ds = object.__new__(pkg.DeviceScene)
    p, li = torch.zeros((8, 3)), torch.zeros(8, dtype=torch.int32)
    u, wi = torch.zeros((8, 2)), torch.zeros((8, 3))
    for args, kw, word in (((p.double(), li), dict(u=u, fields=("s_wi",)), "float32"),
                           ((p[:, :2].contiguous(), li), dict(u=u, fields=("s_wi",)), "shape"),
                           ((p, li.long()), dict(u=u, fields=("s_wi",)), "int32"),
                           ((p, li[:4]), dict(u=u, fields=("s_wi",)), "shape"),
                           ((p, li), dict(fields=("s_wi",)), "u: needed"),
                           ((p, li), dict(u=u, fields=("pdf",)), "wi: needed"),
                           ((p, li), dict(u=torch.zeros((8, 3)), fields=("s_wi",)), "shape"),
                           ((p, li), dict(u=u, wi=wi.t().contiguous().t(), fields=("le",)), "contiguous"),
                           ((p, li), dict(u=u, n=torch.zeros((8, 2)), fields=("s_wi",)), "shape"),
                           ((p, li), dict(u=u, rng=torch.zeros((8, 2)), fields=("s_wi",)), "dtype"),
                           ((p, li), dict(u=u, fields=("nope",)), "unknown field"),
                           ((p, li), dict(u=u, fields=()), "at least one"),
                           ((np.zeros((8, 3), np.float32), li), dict(u=u, fields=("s_wi",)), "torch tensor"),
                           ((p, li), dict(u=u, fields=("s_wi",)), "device memory")):
        with pytest.raises(ValueError) as e:
            ds.light(*args, **kw)
        assert word in str(e.value), (word, str(e.value))
