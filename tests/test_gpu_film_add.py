"""Film::AddSample for radiances in device memory on the GPU: DeviceScene.add_samples (rt_film_add_device) and DeviceScene.sample_positions_device
(rt_sample_positions_device).  The defining property is a round trip: the records a render() leaves in samples(), added to a cleared film, give
that render's film_accum() bit for bit -- in one call or in ascending chunks -- and so does the composed loop
add_samples(radiance(camera_rays_device(0, N))).  The films of the fixtures used are held to the reference by the tests of their own features; the
equality carries that pin over.  Then: radiances that are the caller's own against the float32 restatement of tests/film_add_forms.py, the add as
not-a-frame, the refusals and a prebuilt scene."""
import ctypes as C

import numpy as np
import pytest
# torch BEFORE the device library is loaded, as bench.py does (pbrt-v1_amd/__init__.py, "rays and hits in device memory")
import torch

import film_add_forms as forms
from conftest import load_golden
from gpu_checks import COUNTER_KEYS, assert_prebuilt_agrees, need_gpu
from test_gpu_parity import GATHER_CASES
from test_gpu_radiance import ROUND_TRIP

pytestmark = pytest.mark.gpu

ALL_KEYS = COUNTER_KEYS + ("stack_overflows",)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gather_text(scenes, name):
    """the scene of a GATHER_CASES entry, made the way test_the_three_film_gathers_agree_bit_for_bit makes it"""
    return scenes.cornell_scene(keyed=True, seed=11, soup_tris=200, **GATHER_CASES[name])


def open_scene(pkg, text):
    ps = pkg.ParsedScene(text=str(text))
    assert ps.valid and ps.errors == 0
    ds = pkg.DeviceScene(ps)
    ds.bind_film()
    return ps, ds


def rendered(ds):
    """(film_accum() F, samples() S) of a render() into a cleared film"""
    ds.clear_film()
    ds.render()
    return ds.film_accum(), ds.samples()


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def assert_same_film(got, want, *what):
    assert got.shape == want.shape and got.shape[0] == 5
    assert np.array_equal(bits(got), bits(want)), what + (int((bits(got) != bits(want)).sum()), float(np.abs(got - want).max()))


# ---------------------------------------------------------------------------------------------- 1. the round trip, records in, film out
# beyond GATHER_CASES: a filter that reaches 6 pixels, more than the packed form of the add's gather holds (rt_film_add.hip)
WIDE = dict(xres=30, yres=22, integrator="whitted", xsamples=2, ysamples=1, jitter=True, pixel_filter="gaussian", filter_params='"float xwidth" [5.6] "float ywidth" [2.0]')


@pytest.mark.parametrize("name", sorted(GATHER_CASES) + ["gaussian_reach6"])
def test_records_in_film_out(pkg, scenes, name):
    """by default and with each form of the gather forced (PBRT_HIP_FILM_ADD): the same bits, the frame's"""
    need_gpu(pkg)
    wide = name == "gaussian_reach6"
    text = scenes.cornell_scene(keyed=True, seed=11, soup_tris=200, **WIDE) if wide else gather_text(scenes, name)
    ps, ds = open_scene(pkg, text)
    F, S = rendered(ds)
    assert S.shape == (ps.n_camera_samples, 8) and np.isfinite(F).all() and F[4].max() > 0 and (S[:, :3] != 0).any()
    L = on_device(S[:, :4])
    for form in (None, "general") + (() if wide else ("packed",)):
        with pytest.MonkeyPatch.context() as mp:
            if form:
                mp.setenv("PBRT_HIP_FILM_ADD", form)
            ds.clear_film()
            ds.add_samples(L)
        assert_same_film(ds.film_accum(), F, name, form)
    # a form that cannot serve the filter, and a form nobody knows, are refused before anything is added
    ds.clear_film()
    for form, word in ((("packed", "reaches more than 5 pixels"),) if wide else ()) + (("fast", "packed or general"),):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PBRT_HIP_FILM_ADD", form)
            with pytest.raises(pkg.RtError) as e:
                ds.add_samples(L)
        assert "PBRT_HIP_FILM_ADD" in str(e.value) and word in str(e.value)
    assert (ds.film_accum() == 0).all()
    ds.close()


# ---------------------------------------------------------------------------------------------- 2. positions
def position_scenes(scenes):
    unjittered = dict(xres=31, yres=17, integrator="whitted", xsamples=3, ysamples=2, jitter=False, pixel_filter="mitchell")
    return {"mitchell_4spp": lambda: gather_text(scenes, "mitchell_4spp"), "mitchell_ld8_lens": lambda: gather_text(scenes, "mitchell_ld8_lens"),
            "random_whitted_lens": lambda: load_golden("random_whitted_lens")["scene"], "unjittered": lambda: scenes.cornell_scene(keyed=True, seed=3, **unjittered),
            "materials/shiny_mesh_direct_all_grid_ld": lambda: load_golden("materials/shiny_mesh_direct_all_grid_ld")["scene"]}


@pytest.mark.parametrize("name", ["mitchell_4spp", "mitchell_ld8_lens", "random_whitted_lens", "unjittered", "materials/shiny_mesh_direct_all_grid_ld"])
def test_positions_are_the_frames_records(pkg, scenes, name):
    need_gpu(pkg)
    assert "materials/shiny_mesh_direct_all_grid_ld" in ROUND_TRIP
    ps, ds = open_scene(pkg, position_scenes(scenes)[name]())
    n = ps.n_camera_samples
    _, S = rendered(ds)
    want = S[:, 4:6]
    got = ds.sample_positions_device(0, n)
    assert tuple(got.shape) == (n, 2) and got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).any(1).sum()))
    assert n > 130
    for first, cnt in ((0, 1), (1, 63), (63, 2), (n - 65, 65)):
        part = ds.sample_positions_device(first, cnt).cpu().numpy()
        assert part.shape == (cnt, 2) and np.array_equal(bits(part), bits(want[first:first + cnt])), (name, first, cnt)
    assert tuple(ds.sample_positions_device(5, 0).shape) == (0, 2)
    ds.close()


# ---------------------------------------------------------------------------------------------- 3. the composed loop
@pytest.mark.parametrize("name", ["materials/sheet_whitted", "direct_spot_area", "materials/shiny_mesh_path", "vol_single_whitted"])
def test_the_composed_loop_gives_the_frames_film(pkg, name):
    need_gpu(pkg)
    ps, ds = open_scene(pkg, load_golden(name)["scene"])
    n = ps.n_camera_samples
    F, _ = rendered(ds)
    assert F[4].max() > 0 and (F[:3] != 0).any()
    ds.clear_film()
    ds.add_samples(ds.radiance(ds.camera_rays_device(0, n)))
    assert_same_film(ds.film_accum(), F, name)
    # ... and in two halves, each half traced and added on its own
    ds.clear_film()
    for first, cnt in ((0, n // 2), (n // 2, n - n // 2)):
        ds.add_samples(ds.radiance(ds.camera_rays_device(first, cnt), first=first), first=first)
    assert_same_film(ds.film_accum(), F, name, "halves")
    ds.close()


# ---------------------------------------------------------------------------------------------- 4. chunks
def add_in_chunks(ds, L, size):
    ds.clear_film()
    for first in range(0, len(L), size):
        ds.add_samples(L[first:first + size], first=first)


@pytest.mark.parametrize("sizes", [(1,), (5, 6, 7), (63, 64, 65), ("row-1", "row", "row+1", "third")], ids=["1", "5-6-7", "63-64-65", "rows"])
def test_ascending_chunks_give_the_frames_film(pkg, scenes, sizes):
    """6 spp: chunk edges fall inside pixels, inside sample rows and on them"""
    need_gpu(pkg)
    ps, ds = open_scene(pkg, gather_text(scenes, "gaussian_6spp"))
    n = ps.n_camera_samples
    rd = ps.render_struct()
    row = (rd.x_end - rd.x_start) * 6                     # the samples of one sample row
    assert n == row * (rd.y_end - rd.y_start)
    named = {"row-1": row - 1, "row": row, "row+1": row + 1, "third": n // 3}
    F, S = rendered(ds)
    L = on_device(S[:, :4])
    for size in sizes:
        add_in_chunks(ds, L, named.get(size, size))
        assert_same_film(ds.film_accum(), F, "gaussian_6spp", size)
    ds.close()


@pytest.mark.parametrize("name,size", [("box_16spp_crop", 1000), ("sinc_reach4", 777)])
def test_chunks_with_a_crop_window_and_a_wide_filter(pkg, scenes, name, size):
    need_gpu(pkg)
    ps, ds = open_scene(pkg, gather_text(scenes, name))
    rd = ps.render_struct()
    if name == "box_16spp_crop":
        assert rd.x_start > 0 and rd.y_start > 0              # the sample extent does not start at 0
    F, S = rendered(ds)
    add_in_chunks(ds, on_device(S[:, :4]), size)
    assert_same_film(ds.film_accum(), F, name, size)
    ds.close()


# ---------------------------------------------------------------------------------------------- 5. radiances that are the caller's own
@pytest.mark.parametrize("name", ["mitchell_4spp", "box_wide", "triangle_1spp"])
def test_the_callers_own_radiances_on_top_of_a_film(pkg, scenes, name):
    need_gpu(pkg)
    ps, ds = open_scene(pkg, gather_text(scenes, name))
    n = ps.n_camera_samples
    geom = forms.film_geometry(ps.render_struct())
    ds.set_counting(True)
    F, S = rendered(ds)
    # the helper first: the frame's own records give the frame's film
    helped, n_bad = forms.add_samples(S[:, :6], geom)
    assert n_bad == 0
    assert_same_film(helped, F, name, "helper")
    gen = torch.Generator().manual_seed(20240611)
    L = (torch.rand((n, 4), generator=gen) * 10).numpy()
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = np.arange(7, n, max(1, n // 300))
    assert 200 <= len(rows) <= 400
    for k, r in enumerate(rows):
        L[r, :3] = ((nan, 1, 1), (1, 1, nan), (inf, inf, inf), (-inf, 0, 0), (0, -1 / 0.715160, 0), (-1, -1, -1))[k % 6]
    xy = ds.sample_positions_device(0, n).cpu().numpy()
    assert np.array_equal(bits(xy), bits(S[:, 4:6]))
    want, n_bad = forms.add_samples(np.concatenate([L, xy], 1), geom, accum=F)
    assert n_bad == len(rows)
    before = ds.counters()
    ds.add_samples(on_device(L))                           # on top of F
    got, after = ds.film_accum(), ds.counters()
    assert np.isfinite(got).all()
    assert_same_film(got, want, name, "own radiances")
    assert after["bad_samples"] == before["bad_samples"] + len(rows)
    assert [after[k] for k in ALL_KEYS if k != "bad_samples"] == [before[k] for k in ALL_KEYS if k != "bad_samples"]
    # the timed scene counts nothing, as its frames and queries count nothing; the film is the same
    ds.set_counting(False)
    ds.clear_film(); ds.add_samples(on_device(S[:, :4])); ds.add_samples(on_device(L))
    assert_same_film(ds.film_accum(), want, name, "timed")
    assert ds.counters() == after
    ds.close()


# ---------------------------------------------------------------------------------------------- 6. not a frame
def test_an_add_leaves_the_last_frame_as_it_was(pkg, scenes):
    need_gpu(pkg)
    ps, ds = open_scene(pkg, gather_text(scenes, "mitchell_4spp"))
    n = ps.n_camera_samples
    F, S = rendered(ds)
    stats, ms = ds.last_stats(), ds.last_ms()
    L = on_device(S[:, :4])
    for part, first in ((L, 0), (L[100:900], 100), (L[:1], n - 1)):
        ds.add_samples(part.contiguous(), first=first)
        ds.sync()
        assert np.array_equal(bits(ds.samples()), bits(S))
        assert ds.last_stats() == stats and ds.last_ms() == ms
    assert not np.array_equal(bits(ds.film_accum()), bits(F))          # (the film did change)
    F2, S2 = rendered(ds)
    assert_same_film(F2, F, "render after adds")
    assert np.array_equal(bits(S2), bits(S))
    ds.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_through_the_c_abi_and_through_python(pkg, scenes):
    need_gpu(pkg)
    ps, ds = open_scene(pkg, gather_text(scenes, "mitchell_4spp"))
    n = ps.n_camera_samples
    lib = pkg.hip_lib()
    F, S = rendered(ds)
    L = on_device(S[:64, :4])
    xy = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.clear_film()
    Lp, XYp, rd = L.data_ptr(), xy.data_ptr(), ps.render_desc

    def refused(rc, fn, *words, code=-1):                  # RT_EINVAL
        msg = lib.rt_last_error().decode()
        assert rc == code and fn in msg and all(w in msg for w in words), (rc, msg)

    refused(lib.rt_film_add_device(ds._s, rd, C.c_void_p(Lp + 4), 0, 8), "rt_film_add_device", "dev_L", "16-byte aligned")
    refused(lib.rt_sample_positions_device(ds._s, rd, 0, 8, C.c_void_p(XYp + 4)), "rt_sample_positions_device", "dev_xy", "8-byte aligned")
    refused(lib.rt_film_add_device(ds._s, rd, C.c_void_p(Lp), n - 7, 8), "rt_film_add_device", "beyond the frame's camera samples")
    refused(lib.rt_sample_positions_device(ds._s, rd, n - 7, 8, C.c_void_p(XYp)), "rt_sample_positions_device", "beyond the frame's camera samples")
    refused(lib.rt_film_add_device(ds._s, rd, None, 0, 8), "rt_film_add_device", "null radiance pointer")
    refused(lib.rt_sample_positions_device(ds._s, rd, 0, 8, None), "rt_sample_positions_device", "null output pointer")
    refused(lib.rt_film_add_device(ds._s, None, C.c_void_p(Lp), 0, 8), "rt_film_add_device", "null render description")
    try:
        ps.set_shard(1, 3, 16)
        refused(lib.rt_film_add_device(ds._s, rd, C.c_void_p(Lp), 0, 8), "rt_film_add_device", "shard_count")
        refused(lib.rt_sample_positions_device(ds._s, rd, 0, 8, C.c_void_p(XYp)), "rt_sample_positions_device", "shard_count")
        with pytest.raises(pkg.RtError) as e:
            ds.add_samples(L)
        assert "rt_film_add_device" in str(e.value) and "shard_count" in str(e.value)
    finally:
        ps.set_shard(0, 1, 64)
    # n == 0 with null pointers
    assert lib.rt_film_add_device(ds._s, rd, None, 0, 0) == 0 and lib.rt_film_add_device(ds._s, rd, None, n, 0) == 0
    assert lib.rt_sample_positions_device(ds._s, rd, 5, 0, None) == 0
    ds.add_samples(torch.zeros((0, 4), dtype=torch.float32, device="cuda"), first=5)
    # nothing was launched: the film is still clear, the output buffer untouched
    ds.sync()
    assert (ds.film_accum() == 0).all() and (xy == 0).all().item()
    # through Python, each with a ValueError that names the argument
    good = L
    for what, t in (("a numpy array", S[:64, :4]), ("float64", good.double()), ("shape [n, 3]", good[:, :3].contiguous()),
                    ("a non-contiguous view", torch.zeros((64, 8), dtype=torch.float32, device="cuda")[:, ::2]), ("a CPU tensor", good.cpu())):
        with pytest.raises(ValueError) as e:
            ds.add_samples(t)
        assert str(e.value).startswith("L:"), (what, str(e.value))
    assert (ds.film_accum() == 0).all()
    # a film of another size than the frame's, and none at all: what render() does in these two cases
    small = torch.zeros((5, 4, 4), dtype=torch.float32, device="cuda")
    assert lib.rt_film_bind(ds._s, C.c_void_p(small.data_ptr()), 4, 4) == 0
    refused(lib.rt_film_add_device(ds._s, rd, C.c_void_p(Lp), 0, 8), "rt_film_add_device", "does not match the bound film")
    assert lib.rt_render(ds._s, rd) == -1 and "does not match the bound film" in lib.rt_last_error().decode()
    ds.sync()
    assert (small == 0).all().item()
    ds.close()
    ps2 = pkg.ParsedScene(text=gather_text(scenes, "mitchell_4spp"))
    bare = pkg.DeviceScene(ps2)
    assert lib.rt_render(bare._s, ps2.render_desc) == -3 and "no film bound" in lib.rt_last_error().decode()      # RT_ESTATE: a scene nobody bound a film to
    refused(lib.rt_film_add_device(bare._s, ps2.render_desc, C.c_void_p(Lp), 0, 8), "rt_film_add_device", "no film bound", code=-3)
    bare.close()
    # the scene still renders its film
    ps3, ds3 = open_scene(pkg, gather_text(scenes, "mitchell_4spp"))
    assert_same_film(rendered(ds3)[0], F, "after the refusals")
    ds3.close()


# ---------------------------------------------------------------------------------------------- 8. a prebuilt scene
def test_prebuilt_scene_adds_the_same(pkg, scenes):
    need_gpu(pkg)
    ps, a = open_scene(pkg, gather_text(scenes, "mitchell_4spp"))
    F, S = rendered(a)
    a.close()
    b = assert_prebuilt_agrees(pkg, ps, F)
    b.clear_film()
    b.add_samples(on_device(S[:, :4]))
    assert_same_film(b.film_accum(), F, "prebuilt")
    b.close()
