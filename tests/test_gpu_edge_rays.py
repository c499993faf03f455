"""Degenerate caller-supplied rays on the GPU: the rays of tests/edge_rays_cases.py (axis-aligned directions with either sign of zero, origins on
kd splits, voxel boundaries, the world bound and triangles, mint / maxt around the hit, scaled and denormal directions, quadric poles, seams and
tangents) through DeviceScene.intersect / occluded / trace_closest / trace_any / radiance, held to the reference's own Scene::Intersect /
IntersectP records (tests/golden/rays/edge_<scene>_<accel>.npz) and to oracle.trace's traversal counters.  tests/test_edge_rays_host.py runs the
same rays through the CPU restatement first."""
import os

import numpy as np
import pytest
# torch BEFORE the device library is loaded (tests/test_gpu_rays.py)
import torch

import edge_rays_cases as E
from conftest import GOLDEN
from gpu_checks import need_gpu
from test_gpu_rays import ROUNDING, TRAV_KEYS, host, open_scene, to_device
import analytic_cases as A
import rays_cases as R

pytestmark = pytest.mark.gpu

PAD_SIZES = (63, 64, 65, 257)


def load(name):
    z = np.load(os.path.join(GOLDEN, "rays", name + ".npz"))
    return str(z["scene"]), z["records"], z["cls"], z["h_base"], z["h_k"]


def same_bits(a, b):
    """bit for bit, and a NaN equals a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    return bool(((E.bits(a) == E.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def where_differs(a, b, cls):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    bad = np.nonzero(~((E.bits(a) == E.bits(b)) | (np.isnan(a) & np.isnan(b))))[0]
    return [(int(i), E.CODES[cls[i]], float(a[i]), float(b[i])) for i in bad[:8]]


# ---------------------------------------------------------------------------------------------- 1. the reference's records
@pytest.mark.parametrize("name", E.FIXTURES)
def test_intersect_and_occluded_against_the_reference(pkg, name):
    """hit mask and t of the reference bit for bit (NaN with NaN), occluded = IntersectP of the ray itself; p, ng, (u, v) against its record under
    the bars of tests/test_gpu_rays.py -- triangles: float32 rounding (ROUNDING); quadrics: BAR_FACTOR x the deviations recorded in
    tests/golden/rays/rays_mixed_grid.npz, relative to t for p, sign-free for the normal.  Left out of the field comparison only: hits whose
    REFERENCE record is non-finite in p, nn, u or v (the device's field must then be non-finite too) and hits at whose t the ray meets more than
    one triangle (edge_rays_cases.equal_t_ties: which one is reported is list order and the reference's mailbox; p is still held)."""
    need_gpu(pkg)
    text, rec, cls, _, h_k = load(name)
    ps, ds = open_scene(pkg, E.product_text(text))
    dev = to_device(E.rays_of_records(pkg, rec))
    got = host(ds.intersect(dev))
    occ = ds.occluded(dev).cpu().numpy()
    bounds = np.array(list(ds.accel_info().bounds), np.float32)
    ds.close()
    # the rays on which the reference's own answer is undefined behaviour ran with the others (no fault); they are compared with nothing
    keep = ~E.outside_contract(rec, cls, h_k, bounds, name.rsplit("_", 1)[1])
    assert (~keep).sum() == (4 if name.endswith("_grid") else 0)
    rec, cls, occ, got = rec[keep], cls[keep], occ[keep], {k: v[keep] for k, v in got.items()}
    hit = rec[:, 8] > 0
    dhit = got["prim"] >= 0
    bad = np.nonzero(dhit != hit)[0]
    print("EDGE-GPU %s rays %d hits %d (device %d) IntersectP %d (device %d)" % (name, len(rec), hit.sum(), dhit.sum(), (rec[:, 18] > 0).sum(), occ.sum()))
    for c, (n, h, o) in E.class_table(rec, cls).items():
        k = cls == E.CODES.index(c)
        print("    class %s rays %3d hits %3d IntersectP %3d | device hits %3d occluded %3d" % (c, n, h, o, dhit[k].sum(), occ[k].sum()))
    assert len(bad) == 0, (name, "hit mask", [(int(i), E.CODES[cls[i]]) for i in bad[:10]])
    assert same_bits(got["t"][hit], rec[hit, 9]), (name, "t", where_differs(got["t"], np.where(hit, rec[:, 9], 0), cls))
    obad = np.nonzero((occ > 0) != (rec[:, 18] > 0))[0]
    assert len(obad) == 0, (name, "occluded", [(int(i), E.CODES[cls[i]]) for i in obad[:10]])
    # the fields
    tv = ps.tri_verts()
    is_tri = np.abs(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])).sum(1) > 0
    on_tri = hit & is_tri[np.where(hit, got["prim"], 0)]
    nonfinite = E.nonfinite_reference_fields(rec)
    ties = E.equal_t_ties(tv, rec)
    print("    non-finite reference fields on %d hits, equal-t ties on %d, of %d" % (nonfinite.sum(), ties.sum(), hit.sum()))
    assert nonfinite.sum() <= 0.10 * hit.sum()
    for f, cols in (("p", slice(10, 13)), ("ng", slice(13, 16)), ("uv", slice(16, 18))):
        nf = hit & ~np.isfinite(rec[:, cols]).all(1)
        assert (~np.isfinite(got[f][nf]).all(1)).all(), (name, f, "finite where the reference's is not")
    tri = on_tri & ~nonfinite
    for f, cols, sel in (("p", slice(10, 13), tri), ("ng", slice(13, 16), tri & ~ties), ("uv", slice(16, 18), tri & ~ties)):
        print("    triangles %s largest difference %.3g on %d hits" % (f, float(np.abs(got[f][sel] - rec[sel, cols]).max()), sel.sum()))
    for f, cols, sel in (("p", slice(10, 13), tri), ("ng", slice(13, 16), tri & ~ties), ("uv", slice(16, 18), tri & ~ties)):
        assert sel.sum() >= 20 and np.allclose(got[f][sel], rec[sel, cols], rtol=ROUNDING, atol=ROUNDING), (name, f)
    quad = hit & ~on_tri & ~nonfinite
    if "quadrics" in name:
        bars = np.load(os.path.join(GOLDEN, "rays", "rays_mixed_grid.npz"))
        t = np.abs(rec[quad, 9].astype(np.float64))           # (a negative mint finds hits behind the origin; a ray from the surface itself has t = 0)
        assert quad.sum() >= 100
        dp = np.abs(got["p"][quad].astype(np.float64) - rec[quad, 10:13]).max(-1)
        dev_n = float(R.sign_free(got["ng"][quad].astype(np.float64), rec[quad, 13:16].astype(np.float64)).max())
        dev_uv = float(np.abs(got["uv"][quad].astype(np.float64) - rec[quad, 16:18]).max())
        print("    quadrics p / t %.3g (bar %.3g) on %d hits, %d of them at t = 0" % (float((dp[t > 0] / t[t > 0]).max()), A.BAR_FACTOR * float(bars["dev_p"]), quad.sum(), (t == 0).sum()))
        for what, d, bar in (("ng", dev_n, float(bars["dev_n"])), ("uv", dev_uv, float(bars["dev_uv"]))):
            print("    quadrics %s %.3g (bar %.3g)" % (what, d, A.BAR_FACTOR * bar))
        assert (dp <= A.BAR_FACTOR * float(bars["dev_p"]) * t).all(), (name, "p")          # relative to t, as the bar is: at t = 0 the point is the origin itself
        for what, d, bar in (("ng", dev_n, float(bars["dev_n"])), ("uv", dev_uv, float(bars["dev_uv"]))):
            assert d <= A.BAR_FACTOR * bar, (name, what, d, bar)
    else:
        assert quad.sum() == 0


# ---------------------------------------------------------------------------------------------- 2. the host-array entry points and the counters
@pytest.mark.parametrize("name", E.FIXTURES)
def test_host_entry_points_and_the_oracles_counters(pkg, oracle, name):
    """trace_closest / trace_any give intersect's / occluded's bits; with counting on, nodes visited, leaf references and primitive tests are those
    of oracle.trace on the same tree (tests/test_edge_rays_host.py: the CPU restatement gives the reference's hits on these rays)"""
    need_gpu(pkg)
    text, rec, cls, _, h_k = load(name)
    ps, ds = open_scene(pkg, E.product_text(text))
    keep = ~E.outside_contract(rec, cls, h_k, np.array(list(ds.accel_info().bounds), np.float32), name.rsplit("_", 1)[1])
    rec, cls = rec[keep], cls[keep]
    rays = E.rays_of_records(pkg, rec)
    dev = to_device(rays)
    got, occ = host(ds.intersect(dev, fields=())), ds.occluded(dev).cpu().numpy()
    ds.set_counting(True); ds.reset_counters()
    hits = ds.trace_closest(rays)
    c_closest = ds.counters()
    ds.reset_counters()
    hocc = ds.trace_any(rays)
    c_any = ds.counters()
    ds.reset_counters()
    ds.intersect(dev, fields=()); ds.sync()
    c_dev = ds.counters()
    ds.set_counting(False)
    nodes, refs = ds.accel_arrays()
    info = ds.accel_info()
    ds.close()
    for k in ("prim", "t", "b1", "b2"):
        assert same_bits(got[k], hits[k]), (name, k)
    assert np.array_equal(occ, hocc)
    want, oc_closest = oracle.trace(ps, rays, False, nodes, refs, np.array(list(info.bounds), np.float32), info=info)
    want_occ, oc_any = oracle.trace(ps, rays, True, nodes, refs, np.array(list(info.bounds), np.float32), info=info)
    print("EDGE-GPU-COUNT %s closest %s any %s" % (name, {k: c_closest[k] for k in TRAV_KEYS}, {k: c_any[k] for k in TRAV_KEYS}))
    for k in ("prim", "t", "b1", "b2"):
        assert same_bits(hits[k], want[k]), (name, k, where_differs(hits[k].astype(np.float32), want[k].astype(np.float32), cls))
    assert np.array_equal(hocc, want_occ)
    for k in TRAV_KEYS:
        assert c_closest[k] == oc_closest[k] == c_dev[k], (name, "closest", k, c_closest[k], oc_closest[k], c_dev[k])
        assert c_any[k] == oc_any[k], (name, "any", k, c_any[k], oc_any[k])


# ---------------------------------------------------------------------------------------------- 3. scaling, no reference needed
@pytest.mark.parametrize("name", E.FIXTURES)
def test_scaled_directions_give_the_unscaled_hit(pkg, name):
    """class (h): d * 2^k with mint, maxt * 2^-k gives the unscaled ray's prim, b1, b2 bit for bit and t * 2^-k exactly -- every product and quotient
    of the slab test, the kd step, the DDA and the triangle test scales by a power of two without rounding.  Triangles: k = +-20, +-60.  The
    quadrics scene: k = +-20 only -- a quadric's discriminant B^2 - 4AC holds |d|^2 |o|^2 (2^120 x 2^8 overflows float32) and the disk's
    |d.z| < 1e-7 test is absolute, so those intersectors are not scale-free at 2^+-60."""
    need_gpu(pkg)
    text, rec, cls, h_base, h_k = load(name)
    ps, ds = open_scene(pkg, E.product_text(text))
    got = host(ds.intersect(to_device(E.rays_of_records(pkg, rec)), fields=()))
    ds.close()
    ks = (-20, 20) if "quadrics" in name else E.H_SCALES
    twins = np.nonzero((cls == E.CODES.index("h")) & np.isin(h_k, ks))[0]
    assert len(twins) == 10 * len(ks)
    base = h_base[twins].astype(np.int64)
    assert (got["prim"][base] >= 0).sum() >= len(ks) * 3
    for k in ("prim", "b1", "b2"):
        assert same_bits(got[k][twins], got[k][base]), (name, k)
    want_t = (got["t"][base].astype(np.float64) * 2.0 ** -h_k[twins].astype(np.float64)).astype(np.float32)
    assert same_bits(got["t"][twins], want_t), (name, where_differs(got["t"][twins], want_t, cls[twins]))


# ---------------------------------------------------------------------------------------------- 4. the megakernel sees the same rays
@pytest.mark.parametrize("name", [n for n in E.FIXTURES if "quadrics" not in n])
def test_radiance_alpha_is_the_hit_mask(pkg, name):
    """DeviceScene.radiance (Whitted, one point light; the frame kernels' restatement of the traversal) returns alpha 1 exactly where intersect (the
    ray-query kernels') hits and 0 elsewhere"""
    need_gpu(pkg)
    text, rec, cls, _, _ = load(name)
    ps, ds = open_scene(pkg, E.product_text(text, res=32))
    assert ps.n_camera_samples >= len(rec) and ps.n_lights == 1
    dev = to_device(E.rays_of_records(pkg, rec))
    prim = ds.intersect(dev, fields=())["prim"].cpu().numpy()
    out = ds.radiance(dev).cpu().numpy()
    ds.close()
    alpha = out[:, 3]
    bad = np.nonzero(alpha != (prim >= 0).astype(np.float32))[0]
    print("EDGE-GPU-LI %s alpha 1 on %d of %d rays" % (name, int((alpha == 1).sum()), len(rec)))
    assert len(bad) == 0, (name, [(int(i), E.CODES[cls[i]], float(alpha[i]), int(prim[i])) for i in bad[:10]])
    assert 0 < (alpha == 1).sum() < len(rec)


# ---------------------------------------------------------------------------------------------- 5. position in the wave
@pytest.mark.parametrize("name", E.FIXTURES)
def test_results_do_not_depend_on_position(pkg, name):
    """the ray set padded by repetition so that the last block holds 63, 64, 65 and 257 mod 256 = 1 rays, rolled by those amounts, and interleaved
    with the ordinary rays of class (d) so that every degenerate lane sits between ordinary lanes: each ray's hit and occlusion are those of the
    plain call, bit for bit"""
    need_gpu(pkg)
    text, rec, cls, _, _ = load(name)
    ps, ds = open_scene(pkg, E.product_text(text))
    rays = E.rays_of_records(pkg, rec).view(np.float32).reshape(-1, 8)
    n = len(rays)
    base = host(ds.intersect(to_device(rays), fields=()))
    base_occ = ds.occluded(to_device(rays)).cpu().numpy()
    ordinary = np.nonzero((cls == E.CODES.index("d")) & (rec[:, 6] == 0) & (E.zero_components(rec) == 0))[0]
    assert len(ordinary) >= 4

    def check(index, label):
        dev = to_device(rays[index])
        got, occ = host(ds.intersect(dev, fields=())), ds.occluded(dev).cpu().numpy()
        for k in ("prim", "t", "b1", "b2"):
            assert same_bits(got[k], base[k][index]), (name, label, k)
        assert np.array_equal(occ, base_occ[index]), (name, label)
    for size in PAD_SIZES:
        total = n + (size - n) % 256
        assert total % 256 == size % 256
        check(np.arange(total) % n, "padded to %d mod 256" % size)
        check(np.roll(np.arange(n), size), "rolled by %d" % size)
    mixed = np.empty(2 * n, np.int64)
    mixed[0::2] = np.arange(n)
    mixed[1::2] = ordinary[np.arange(n) % len(ordinary)]
    check(mixed, "interleaved")
    ds.close()
