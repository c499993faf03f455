"""Generate tests/golden/rays/edge_<scene>_<accel>.npz: the reference's Intersection records for the degenerate rays of tests/edge_rays_cases.py.
Runs only where the reference sources exist.

    python tests/golden/make_edge_rays_golden.py [edge_<scene>_<accel> ...]

The UNMODIFIED reference (oracle/_ref/pbrt_ref, the non-keyed build: no random number is involved) runs each scene with the SurfaceIntegrator
"rayfile" plugin (oracle/ref/rayfile_integrator.cpp), which reads 8-float rays from a file in Preprocess and writes 20 floats per ray:
o d mint maxt | hit t p nn u v | IntersectP of the ray itself.  Two passes: the second adds class (g), built around the first pass' own t.
Each fixture stores the scene text, the records, each ray's class and, for class (h), the unscaled ray's index and the exponent k.
The generator refuses a fixture in which a class has no hit or no miss, class (b) holds a ray whose coordinate is not bit-equal to a stored split
of the tree the host library builds from the scene text (likewise (c): the world bound, (e): a voxel boundary), more than 10 % of the hits hold
a non-finite p, nn, u or v, or the file is above 64 KB.  Fixtures are DATA (scene text, arrays); no reference source text is stored."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import __graft_entry__ as g  # noqa: E402
import edge_rays_cases as E  # noqa: E402

OUT = os.path.join(HERE, "rays")
MAX_BYTES = 64 * 1024
NONFINITE_CAP = 0.10


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed time stamp per member: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


def reference_records(REF, text, rays):
    d = tempfile.mkdtemp()
    np.ascontiguousarray(rays, np.float32).tofile(os.path.join(d, "rays.bin"))
    REF.run_reference(text, keyed=False, workdir=d, timeout=120)
    rec = np.fromfile(os.path.join(d, "hits.bin"), np.float32).reshape(-1, 20)
    assert len(rec) == len(rays) and np.array_equal(E.bits(rec[:, :8]), E.bits(rays)), "the plugin did not read the rays it was given"
    return rec


def check(pkg, name, text, rec, cls):
    """the refusals (tests/test_edge_rays_host.py recomputes the same from the fixture and the current tree)"""
    accel = name.rsplit("_", 1)[1]
    table = E.class_table(rec, cls)
    for c, (n, hits, occ) in table.items():
        assert 0 < hits < n, "%s: class %s has %d hits among %d rays" % (name, c, hits, n)
    _, kd_nodes, _, _, _ = E.accel_of(pkg, text, "kdtree")
    _, _, _, _, grid = E.accel_of(pkg, text, "grid")
    _, _, _, bounds, _ = E.accel_of(pkg, text, accel)
    is_ = lambda c: cls == E.CODES.index(c)
    assert E.class_b_on_split(rec, kd_nodes)[is_("b")].all(), name + ": a ray of class (b) is on no stored split"
    assert E.class_c_on_bound(rec, bounds)[is_("c")].all(), name + ": a ray of class (c) is not on the world bound"
    assert E.class_e_on_voxel_boundary(rec, grid)[is_("e")].all(), name + ": a ray of class (e) is on no voxel boundary"
    nf = E.nonfinite_reference_fields(rec)
    share = nf.sum() / max(1, (rec[:, 8] > 0).sum())
    assert share <= NONFINITE_CAP, "%s: %.3f of the hits hold non-finite fields" % (name, share)
    return table, share


def main():
    REF = g.load_ref_runner()
    pkg = g.load_package()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for scene in E.SCENES:
        for accel in E.ACCELS:
            name = "edge_%s_%s" % (scene, accel)
            if only and name not in only:
                continue
            text = E.scene_text(scene, accel)
            rays, cls, base, k, seeds = E.first_pass(pkg, scene, accel, text)
            rec = reference_records(REF, text, rays)
            rays, cls, base, k = E.second_pass(rays, cls, base, k, seeds, rec)
            rec = reference_records(REF, text, rays)
            table, share = check(pkg, name, text, rec, cls)
            print("%s: %d rays, non-finite fields in %.3f of the hits" % (name, len(rec), share))
            for c, (n, hits, occ) in table.items():
                print("    %s  rays %3d  hits %3d  IntersectP %3d" % (c, n, hits, occ))
            path = os.path.join(OUT, name + ".npz")
            save_npz(path, scene=np.array(text), records=rec, cls=cls, h_base=base, h_k=k)
            assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))
            print("    %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
