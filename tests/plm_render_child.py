"""Child process of tests/test_gpu_plm.py: renders every fixture of tests/golden/plm/ on the device with the library named by PBRT_HIP_LIB_PATH
(the -DRT_PORTABLE_LIBM build), as counting twin and as timed kernel, and writes films and counters to one .npz.

    PBRT_HIP_TUNE=1 PBRT_HIP_LIB_PATH=.../libpbrt_hip_plm.so python tests/plm_render_child.py OUT.npz

With oracle/_ref/pbrt_ref_keyed_plm present it also draws the mix seeds LIVE_SEEDS (never committed ones), renders them through that binary on the
CPU and on the device, and stores both.  The first error ends the process with a non-zero status: nothing more starts on the device."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import __graft_entry__ as entry  # noqa: E402

LIVE_SEEDS = (10000, 10001, 10002, 10003)


def render_both(pkg, text):
    ps = pkg.ParsedScene(text=text)
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    ds.set_counting(False); ds.clear_film(); ds.render()
    trgb, talpha = ds.film()
    ds.close()
    ps.close()
    return rgb, alpha, cnt, trgb, talpha


def main():
    out_path = sys.argv[1]
    pkg = entry.load_package()
    import make_plm_golden as gen
    want = os.environ.get("PBRT_HIP_LIB_PATH", "")
    assert os.environ.get("PBRT_HIP_TUNE") and os.path.realpath(pkg.HIP_LIB) == os.path.realpath(want) == os.path.realpath(entry.PLM_LIB), (pkg.HIP_LIB, want)
    product = os.path.join(pkg.LIB_DIR, "libpbrt_hip.so")
    ids = dict(variant=pkg.code_id(pkg.HIP_LIB), product=pkg.code_id(product))
    assert ids["variant"] != ids["product"], ids
    if pkg.device_count() < 1:
        raise RuntimeError("no HIP device visible")
    out = {"code_ids": np.array(json.dumps(ids))}
    names = sorted(f[:-4] for f in os.listdir(gen.OUT) if f.endswith(".npz"))
    for name in names:
        fx = np.load(os.path.join(gen.OUT, name + ".npz"))
        text = gen.scene_text(name, str(fx["source"]))
        assert gen.sha(text) == str(fx["scene_sha256"]), name
        rgb, alpha, cnt, trgb, talpha = render_both(pkg, text)
        out.update({name + "/rgb": rgb, name + "/alpha": alpha, name + "/trgb": trgb, name + "/talpha": talpha, name + "/cnt": np.array(json.dumps(cnt))})
    live = []
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "pbrt_ref_keyed_plm")):
        import make_mix_golden as mixes
        REF = entry.load_ref_runner()
        for seed in LIVE_SEEDS:
            text, f = mixes.mix_scene(seed)
            ref_rgb, ref_alpha, st = REF.run_reference(text, keyed=True, libm="portable")
            assert st["stderr_lines"] == 0
            rgb, alpha, cnt, trgb, talpha = render_both(pkg, text)
            name = "live_%d" % seed
            live.append(name)
            out.update({name + "/rgb": rgb, name + "/alpha": alpha, name + "/trgb": trgb, name + "/talpha": talpha, name + "/cnt": np.array(json.dumps(cnt)),
                        name + "/ref_rgb": ref_rgb, name + "/ref_alpha": ref_alpha, name + "/stats": np.array(json.dumps(st))})
    out["names"] = np.array(json.dumps(names))
    out["live"] = np.array(json.dumps(live))
    np.savez(out_path, **out)
    print("plm_render_child: ok (%d fixtures, %d live)" % (len(names), len(live)))


if __name__ == "__main__":
    main()
