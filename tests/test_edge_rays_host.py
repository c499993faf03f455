"""Degenerate caller-supplied rays on the host (no GPU): the fixtures of tests/golden/rays/edge_<scene>_<accel>.npz (the reference's own
Scene::Intersect / IntersectP on the rays of tests/edge_rays_cases.py) against oracle.trace, the CPU restatement of the device's traversal --
closest and any-hit, kd-tree and grid -- and the class-membership checks of the generator recomputed from the fixture and the current tree.
This is the executable half of the argument that such rays are safe to hand to the device: the same steps on the same values terminate on the
host with every index in range, and tests/test_gpu_edge_rays.py holds the device to the counters recorded here."""
import os

import numpy as np
import pytest

import edge_rays_cases as E
from conftest import GOLDEN

TRAV_KEYS = ("nodes_visited", "leaf_refs", "tri_tests")
NONFINITE_CAP = 0.10


def load(name):
    z = np.load(os.path.join(GOLDEN, "rays", name + ".npz"))
    return str(z["scene"]), z["records"], z["cls"], z["h_base"], z["h_k"]


def same_floats(a, b):
    """bit for bit, and a NaN equals a NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((E.bits(a) == E.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def oracle_trace(pkg, oracle, name):
    """(closest hits, occluded, counters of the closest pass, counters of the any-hit pass) of oracle.trace on a fixture's rays"""
    text, rec, _, _, _ = load(name)
    ps, nodes, refs, bounds, info = E.accel_of(pkg, text, name.rsplit("_", 1)[1])
    rays = E.rays_of_records(pkg, rec)
    hits, c_closest = oracle.trace(ps, rays, False, nodes, refs, bounds, info=info)
    occ, c_any = oracle.trace(ps, rays, True, nodes, refs, bounds, info=info)
    return hits, occ, c_closest, c_any


@pytest.mark.parametrize("name", E.FIXTURES)
def test_oracle_trace_gives_the_references_hits(pkg, oracle, name):
    """hit mask, t (bit for bit; NaN with NaN) and IntersectP of every ray of every class; it returns, so it terminates"""
    _, rec, cls, _, _ = load(name)
    hits, occ, c_closest, c_any = oracle_trace(pkg, oracle, name)
    hit = rec[:, 8] > 0
    got = hits["prim"] >= 0
    bad = np.nonzero(got != hit)[0]
    assert len(bad) == 0, (name, "hit mask", [(int(i), E.CODES[cls[i]]) for i in bad[:10]])
    tbad = np.nonzero(hit & ~((E.bits(hits["t"]) == E.bits(rec[:, 9])) | (np.isnan(hits["t"]) & np.isnan(rec[:, 9]))))[0]
    assert len(tbad) == 0, (name, "t", [(int(i), E.CODES[cls[i]], float(hits["t"][i]), float(rec[i, 9])) for i in tbad[:10]])
    obad = np.nonzero((occ > 0) != (rec[:, 18] > 0))[0]
    assert len(obad) == 0, (name, "IntersectP", [(int(i), E.CODES[cls[i]]) for i in obad[:10]])
    # triangles with the default uv: u = b1 + b2, v = b2 (trianglemesh.cpp:266-268, :321-326) -- wherever the ray meets ONE triangle at its t
    if "quadrics" not in name:
        text = load(name)[0]
        ties = E.equal_t_ties(E.accel_of(pkg, text, "kdtree")[0].tri_verts(), rec)
        one = hit & np.isfinite(rec[:, 16:18]).all(1) & ~ties
        print("EDGE-HOST %s equal-t ties on %d of %d hits" % (name, int(ties.sum()), int(hit.sum())))
        assert ties.sum() <= 0.25 * hit.sum() and one.sum() >= 200         # (classes c, f and what g takes from them meet edges and vertices on purpose)
        assert np.array_equal((hits["b1"] + hits["b2"])[one], rec[one, 16]) and np.array_equal(hits["b2"][one], rec[one, 17])
        # and the reference's per-primitive mailbox changes the primitive only on such a tie
        oracle.set_mailbox(-1)
        try:
            boxed = oracle_trace(pkg, oracle, name)[0]
        finally:
            oracle.set_mailbox(0)
        assert np.array_equal(boxed["prim"][~ties], hits["prim"][~ties]) and same_floats(boxed["t"], hits["t"])
    print("EDGE-HOST %s closest %s any %s" % (name, {k: c_closest[k] for k in TRAV_KEYS}, {k: c_any[k] for k in TRAV_KEYS}))
    assert c_closest["nodes_visited"] > 0 and c_closest["tri_tests"] > 0 and c_any["tri_tests"] > 0


@pytest.mark.parametrize("name", E.FIXTURES)
def test_every_class_is_what_its_name_says(pkg, name):
    """the generator's refusals, recomputed from the fixture and the tree the host library builds today: a changed tree cannot empty a class silently"""
    text, rec, cls, h_base, h_k = load(name)
    accel = name.rsplit("_", 1)[1]
    assert os.path.getsize(os.path.join(GOLDEN, "rays", name + ".npz")) < 64 * 1024
    present = set(E.CODES[c] for c in cls)
    assert present == set(E.CODES) - (set() if "quadrics" in name else {"i"})
    for c, (n, hits, occ) in E.class_table(rec, cls).items():
        assert n >= 20 and 0 < hits < n, (name, c, n, hits)
    _, kd_nodes, _, _, _ = E.accel_of(pkg, text, "kdtree")
    _, _, _, _, grid = E.accel_of(pkg, text, "grid")
    _, nodes, _, bounds, info = E.accel_of(pkg, text, accel)
    is_ = lambda c: cls == E.CODES.index(c)
    # a. exactly one non-zero component, and all four sign patterns of the two zeros, per travel axis and sense
    a = rec[is_("a")]
    assert (E.zero_components(a) == 2).all()
    patterns = set()
    for r in a:
        axis = int(np.nonzero(r[3:6])[0][0])
        patterns.add((axis, bool(r[3 + axis] > 0), bool(np.signbit(r[3 + (axis + 1) % 3])), bool(np.signbit(r[3 + (axis + 2) % 3]))))
    assert len(patterns) == 24
    # b. on a stored split of the top three levels; the tree is several levels deep and its bounds are integers where the scene's are
    splits = E.top_splits(kd_nodes)
    assert len(splits) >= 3 and E.class_b_on_split(rec, kd_nodes)[is_("b")].all()
    if "lattice" in name:
        assert np.array_equal(bounds, np.array([0, 0, 0, 16, 16, 16], np.float32))
        assert len(splits) == 7 and any(E.bits(s) & 3 for _, s in splits)        # stored splits on y and z are not the integers themselves
    # c. on the world bound; e. on a voxel boundary
    assert E.class_c_on_bound(rec, bounds)[is_("c")].all()
    assert E.class_e_on_voxel_boundary(rec, grid)[is_("e")].all()
    # d. every origin inside the bound, a third each of mint = 0, mint beyond the bound, mint < 0
    d = rec[is_("d")]
    assert ((d[:, 0:3] > bounds[:3]) & (d[:, 0:3] < bounds[3:])).all()
    pm = d[:, 0:3] + d[:, 3:6] * d[:, 6:7]
    outside = ((pm < bounds[:3]) | (pm > bounds[3:])).any(1)
    assert (d[:, 6] == 0).sum() * 3 == len(d) and (d[:, 6] < 0).sum() * 3 == len(d) and outside[d[:, 6] > 0].all() and (d[:, 6] > 0).sum() * 3 == len(d)
    # g. the seven variants
    gr = rec[is_("g")]
    assert len(gr) % 7 == 0 and np.isinf(gr[4::7, 7]).all() and (gr[5::7, 6] == gr[5::7, 7]).all() and (gr[6::7, 6] > gr[6::7, 7]).all()
    assert (gr[6::7, 8] == 0).all() and (gr[6::7, 18] == 0).all()                    # mint > maxt: an ordinary empty ray
    # h. the scaled twins are the base ray scaled, and the denormal twins are denormal
    for i in np.nonzero(is_("h") & (h_k != 0))[0]:
        b, k = int(h_base[i]), int(h_k[i])
        assert h_k[b] == 0 and h_base[b] == b and np.array_equal(rec[i, 0:3], rec[b, 0:3])
        if k == E.H_DENORMAL:
            dd = rec[i, 3:6]
            with np.errstate(over="ignore"):
                assert (np.abs(dd[dd != 0]) < np.finfo(np.float32).tiny).all() and np.isinf(np.float32(1) / np.abs(dd[dd != 0])).all()
        else:
            assert k in E.H_SCALES and np.array_equal(rec[i, 3:6], (rec[b, 3:6].astype(np.float64) * 2.0 ** k).astype(np.float32))
            assert rec[i, 7] == np.float32(float(rec[b, 7]) * 2.0 ** -k)
    # the share of hits whose reference record is non-finite in p, nn, u, v: left out of the field comparison on the device, capped
    nf = E.nonfinite_reference_fields(rec)
    assert nf.sum() <= NONFINITE_CAP * (rec[:, 8] > 0).sum()


def test_scenes_are_what_the_fixtures_hold():
    """the fixtures' scene texts are those tests/edge_rays_cases.py writes today (the lattice is seeded)"""
    for scene in E.SCENES:
        for accel in E.ACCELS:
            assert load("edge_%s_%s" % (scene, accel))[0] == E.scene_text(scene, accel)
    tv = E.lattice_tris()
    assert 250 <= len(tv) <= 350 and (tv == np.round(tv)).all() and tv.min() == 0 and tv.max() == 16
