"""pbrt-v1 Scene::Render hot path on MI355X -- Python harness over the C ABI.

This package is *plumbing*: ctypes bindings of ``lib/libpbrt_hip.so`` (include/pbrt_hip.h,
the HIP kernels + C ABI) and ``lib/libpbrt_host.so`` (the C++ host mirror of pbrt-v1's scene
API), used by tests/, bench.py and __graft_entry__.py.  There is no CPU fallback anywhere:
if the HIP library is missing or no GPU is visible, calls raise.

The directory name ``pbrt-v1_amd`` is not an importable identifier; load it with
``__graft_entry__.load_package()`` (importlib, module name ``pbrt_v1_amd``).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
HIP_LIB = os.path.join(LIB_DIR, "libpbrt_hip.so")
if os.environ.get("PBRT_HIP_TUNE") and os.environ.get("PBRT_HIP_LIB_PATH"):      # A/B measurements: a variant built by tools/build_variant.py
    HIP_LIB = os.environ["PBRT_HIP_LIB_PATH"]
HOST_LIB = os.path.join(LIB_DIR, "libpbrt_host.so")
CSRC = os.path.join(_HERE, "csrc")

# -fno-slp-vectorize: with the SLP vectorizer on, hipcc (ROCm 7.2) packs the y / z components of the integrators' 3-vectors into
# v_pk_*_f32 pairs, and the megakernel of the volume workload then computes (x, 0, 0) for 3 of 16.8 M camera samples of the C5 frame
# (deterministic, every flavour; tests/test_gpu_configs.py::test_pipeline_workloads_full_size_properties found it, the pipeline
# and the oracle agree on the right value; any added printf hides it).  Without it the results are right AND the kernels are faster
# (C3 kernel 16.8 -> 14.6 ms, C2 59.0 -> 57.4 ms: the packing costs registers).
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared",
               "-Wno-unused-value"]
HOST_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-msse2", "-mfpmath=sse", "-fvisibility=hidden", "-fvisibility-inlines-hidden"]


HIP_UNITS = ("rt_kernels.hip", "rt_scene.hip", "rt_film.hip", "rt_trace.hip", "rt_mega_w.hip", "rt_mega_d.hip", "rt_mega_dw.hip", "rt_mega_p.hip", "rt_mega_b.hip", "rt_mega_g.hip", "rt_mega_f.hip", "rt_mega_fsd.hip", "rt_mega_fsp.hip", "rt_mega_rw.hip", "rt_mega_rd.hip", "rt_mega_rp.hip", "rt_pipe_w.hip", "rt_pipe_d.hip",
             "rt_pipe_p.hip", "rt_pipe_v.hip", "rt_march.hip", "rt_rays.hip", "rt_bsdf.hip", "rt_light.hip", "rt_medium.hip", "rt_film_add.hip", "kd_build.cpp", "grid_build.cpp", "leaf_layout.cpp")


def _include_closure(path, seen=None):
    """the files `path` includes with #include "..." (transitively): a unit is rebuilt only when one of ITS headers changed"""
    import re
    seen = set() if seen is None else seen
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        _include_closure(os.path.normpath(os.path.join(os.path.dirname(path), inc)), seen)
    return seen


def _compile_unit(cmd, verbose=False):
    """one hipcc -c command (source at cmd[-3], object at cmd[-1]).  A .hip unit keeps the compiler's per-kernel resource report (VGPRs,
    spills, occupancy) next to the object: tests/test_abi.py checks that the timed kernels stay inside their occupancy step (gfx950:
    <= 168 VGPRs for 3 waves per SIMD, <= 64 for 8)"""
    if verbose:
        print(" ".join(cmd))
    if not cmd[-3].endswith(".hip"):
        subprocess.check_call(cmd)
        return
    r = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    keep = [ln for ln in r.stderr.splitlines() if "remark:" in ln and any(k in ln for k in ("Function Name", " VGPRs:", "VGPRs Spill", "Occupancy", "ScratchSize", "LDS Size"))]
    open(cmd[-1][:-2] + ".resources.txt", "w").write("\n".join(keep) + "\n")
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])


def build(force: bool = False, verbose: bool = False, defines=(), jobs: int | None = None) -> None:
    """Compile both shared libraries in-tree (hipcc cross-compiles gfx950 without a GPU).  The HIP library is ten translation
    units (the megakernel and the pipeline's shade kernel per integrator, the trace kernel, the C ABI, the two host builders)
    compiled in parallel and linked; `defines` (-D knobs; tools/build_variant.py builds variants side by side) force a rebuild into the same place."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(LIB_DIR, exist_ok=True)
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    hip_dir = os.path.join(CSRC, "hip")
    hip_dep = [os.path.join(hip_dir, f) for f in os.listdir(hip_dir)] + [os.path.join(_HERE, "..", "include", "pbrt_hip.h")]
    headers = [d for d in hip_dep if d.endswith((".h", ".inc"))]
    host_src = [os.path.join(CSRC, "host", "scene_api.cpp")]
    host_dep = [os.path.join(CSRC, "host", f) for f in os.listdir(os.path.join(CSRC, "host"))] + \
               [os.path.join(_HERE, "..", "include", f) for f in ("pbrt_hip.h", "pbrt_hip_desc.h", "pbrt_hip_plugin.h", "pbrt_hip_material.h", "pbrt_hip_texture.h")]

    def stale(out, deps):
        return force or not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)

    stamp = os.path.join(obj_dir, "defines.txt")
    # the stamp holds the compiler flags too: an object built with other flags (e.g. before -fno-slp-vectorize, a correctness fix) must
    # not survive an incremental build just because it is newer than its sources
    dtext = " ".join(HIPCC_FLAGS) + " | " + " ".join(HOST_FLAGS) + " | " + " ".join(defines)
    if (open(stamp).read() if os.path.exists(stamp) else "") != dtext:
        force = True
    todo = []
    for u in HIP_UNITS:
        obj = os.path.join(obj_dir, u.rsplit(".", 1)[0] + ".o")
        if stale(obj, sorted(_include_closure(os.path.join(hip_dir, u)))):
            todo.append(["hipcc"] + [f for f in HIPCC_FLAGS if f != "-shared"] + list(defines) + ["-c", os.path.join(hip_dir, u), "-o", obj])
    if todo:
        run = lambda cmd: _compile_unit(cmd, verbose)
        with ThreadPoolExecutor(max_workers=jobs or min(len(todo), os.cpu_count() or 4)) as ex:
            list(ex.map(run, todo))
        open(stamp, "w").write(dtext)
    objs = [os.path.join(obj_dir, u.rsplit(".", 1)[0] + ".o") for u in HIP_UNITS]
    if stale(HIP_LIB, objs):
        cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", HIP_LIB]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    if stale(HOST_LIB, host_dep):
        cmd = ["g++"] + HOST_FLAGS + host_src + ["-Wl,--version-script=" + os.path.join(CSRC, "host", "exports.map"), "-ldl", "-o", HOST_LIB]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)


def build_variant(name: str, defines=(), units=None, arch: str | None = None, verbose: bool = False) -> str:
    """A variant of libpbrt_hip.so next to the product library (tools/build_variant.py is its command line): the translation units `units`
    (default: all) compiled with the extra `defines` into lib/obj_NAME/, the others taken from the product build, linked as
    lib/libpbrt_hip_NAME.so.  Like build(): a stamp of flags and defines forces a rebuild when they change, otherwise a unit is compiled again
    only when a file of its include closure is newer than its object.  A process picks the variant with PBRT_HIP_LIB_PATH (read only when
    PBRT_HIP_TUNE is set).  Returns the library's path."""
    from concurrent.futures import ThreadPoolExecutor
    units = list(HIP_UNITS if units is None else units)
    if len(units) < len(HIP_UNITS):
        build()                                                  # the product objects the variant borrows
    obj_dir = os.path.join(LIB_DIR, "obj_" + name)
    os.makedirs(obj_dir, exist_ok=True)
    hip_dir = os.path.join(CSRC, "hip")
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    if arch:
        flags = ["--offload-arch=" + arch if f.startswith("--offload-arch=") else f for f in flags]
    out = os.path.join(LIB_DIR, "libpbrt_hip_%s.so" % name)
    stamp = os.path.join(obj_dir, "defines.txt")
    dtext = " ".join(flags) + " | " + " ".join(defines) + " | " + " ".join(units)
    lib_ok = os.path.exists(out) and (open(stamp).read() if os.path.exists(stamp) else "") == dtext
    obj_of = lambda d, u: os.path.join(d, u.rsplit(".", 1)[0] + ".o")

    def stale(u):
        # a tree that arrives with the linked library but without its objects is judged by the library's time: nothing is stale there
        obj = obj_of(obj_dir, u)
        if not lib_ok:
            return True
        t = os.path.getmtime(obj if os.path.exists(obj) else out)
        return any(os.path.getmtime(d) > t for d in _include_closure(os.path.join(hip_dir, u)))
    todo = [u for u in units if stale(u)]
    borrowed = [obj_of(os.path.join(LIB_DIR, "obj"), u) for u in HIP_UNITS if u not in units]
    if not todo and lib_ok and not any(os.path.getmtime(o) > os.path.getmtime(out) for o in borrowed):
        return out
    todo += [u for u in units if u not in todo and not os.path.exists(obj_of(obj_dir, u))]       # the link needs every object
    cmds = [["hipcc"] + flags + list(defines) + ["-c", os.path.join(hip_dir, u), "-o", obj_of(obj_dir, u)] for u in todo]
    if cmds:
        with ThreadPoolExecutor(max_workers=min(len(cmds), os.cpu_count() or 4)) as ex:
            list(ex.map(lambda cmd: _compile_unit(cmd, verbose), cmds))
    objs = [obj_of(obj_dir if u in units else os.path.join(LIB_DIR, "obj"), u) for u in HIP_UNITS]
    subprocess.check_call(["hipcc", "--offload-arch=" + (arch or "gfx950"), "-shared", "-fPIC"] + objs + ["-o", out])
    open(stamp, "w").write(dtext)
    return out


# --------------------------------------------------------------------------- C ABI structs
class RtCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("camera_rays", "closest_rays", "any_rays", "nodes_visited", "leaf_refs",
                                          "tri_tests", "bad_samples", "stack_overflows")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RtAccelInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_leaf_refs", C.c_uint32), ("max_depth", C.c_uint32), ("n_tris", C.c_uint32),
                ("bounds", C.c_float * 6), ("build_seconds", C.c_double), ("kind", C.c_int32),
                ("grid_nvoxels", C.c_int32 * 3), ("grid_width", C.c_float * 3), ("grid_inv_width", C.c_float * 3)]


class RtLeafLayoutInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_slots", C.c_uint64), ("n_entries", C.c_uint64), ("stride", C.c_uint32), ("pad", C.c_uint32)]


class RtPrebuiltAccel(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_nodes", C.c_uint32), ("n_leaf_refs", C.c_uint32), ("max_depth", C.c_uint32),
                ("nodes", C.c_void_p), ("leaf_refs", C.c_void_p), ("bounds", C.c_float * 6),
                ("grid_nvoxels", C.c_int32 * 3), ("grid_width", C.c_float * 3), ("grid_inv_width", C.c_float * 3)]


class RtRenderStats(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("render_ms", C.c_float), ("trace_ms", C.c_float), ("gather_ms", C.c_float),
                ("pipeline", C.c_int32), ("iterations", C.c_int32), ("timed_iterations", C.c_int32), ("slots", C.c_uint32), ("shade_ms", C.c_float), ("bands", C.c_int32), ("march_ms", C.c_float),
                ("weighted_points", C.c_uint64), ("weighted_ms", C.c_float * 5), ("fixed_frame", C.c_int32), ("fixed_scene", C.c_int32)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "weighted_ms" else getattr(self, n)) for n, _ in self._fields_}


class RtVolume(C.Structure):
    _fields_ = [("present", C.c_int32), ("world_to_volume", C.c_float * 16), ("p0", C.c_float * 3), ("p1", C.c_float * 3),
                ("sigma_a", C.c_float * 3), ("sigma_s", C.c_float * 3), ("le", C.c_float * 3), ("g", C.c_float)]


class RtDensityRegion(C.Structure):
    _fields_ = [("kind", C.c_int32), ("a", C.c_float), ("b", C.c_float), ("updir", C.c_float * 3),
                ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("density", C.POINTER(C.c_float))]


RT_MATERIAL_NAMES = ("matte", "mirror", "glass", "plastic", "uber", "shinymetal", "translucent")


class RtMaterial(C.Structure):                     # include/pbrt_hip.h (64 bytes)
    _fields_ = [("type", C.c_int32), ("kd", C.c_float * 3), ("kt", C.c_float * 3), ("sigma", C.c_float), ("ior", C.c_float),
                ("ks", C.c_float * 3), ("roughness", C.c_float), ("kr", C.c_float * 3)]


class RtMaterialLobes(C.Structure):                # include/pbrt_hip_material.h
    _fields_ = [(n, C.c_float * 3) for n in ("eta_ks", "eta_kr", "r_kd", "t_kd", "r_ks", "t_ks")] + \
               [(n, C.c_int32) for n in ("has_dr", "has_dt", "has_gr", "has_gt")]


class RtMaterialParams(C.Structure):               # include/pbrt_hip_texture.h: a material's raw parameters by slot
    _fields_ = [("type", C.c_int32), ("c", (C.c_float * 3) * 4), ("f", C.c_float)]


class RtMaterialTextures(C.Structure):             # ... and per slot the texture node that replaces it at every hit, or -1
    _fields_ = [("raw", RtMaterialParams), ("tex", C.c_int32 * 5)]


class RtMaterialResolved(C.Structure):             # ... and what the kernels read (84 bytes)
    _fields_ = [("type", C.c_int32), ("r", C.c_float * 3), ("t", C.c_float * 3), ("on_a", C.c_float), ("on_b", C.c_float), ("ior", C.c_float),
                ("has_r", C.c_int32), ("has_t", C.c_int32), ("ks", C.c_float * 3), ("exponent", C.c_float), ("kr", C.c_float * 3),
                ("has_g", C.c_int32), ("has_kr", C.c_int32)]


class RtTexture(C.Structure):                      # include/pbrt_hip_texture.h: one node of the texture table (168 bytes)
    _fields_ = [("kind", C.c_int32), ("is_color", C.c_int32), ("mapping", C.c_int32), ("child", C.c_int32 * 3), ("value", C.c_float * 12),
                ("map", C.c_float * 8), ("world_to_texture", C.c_float * 16)]


RT_TEXTURE_NAMES = ("constant", "scale", "mix", "bilerp", "uv", "checkerboard")
RT_TEXMAP_NAMES = ("uv", "spherical", "cylindrical", "planar")
# the parameter behind each slot of RtMaterialParams (c[0] .. c[3], f), by material
RT_MATERIAL_SLOTS = {"matte": ("Kd", None, None, None, "sigma"), "mirror": ("Kr", None, None, None, None), "glass": ("Kr", "Kt", None, None, "index"),
                     "plastic": ("Kd", "Ks", None, None, "roughness"), "uber": ("Kd", "Ks", "Kr", "opacity", "roughness"),
                     "shinymetal": (None, "Ks", "Kr", None, "roughness"), "translucent": ("Kd", "Ks", "reflect", "transmit", "roughness")}

RT_DENSITY_NAMES = {1: "exponential", 2: "volumegrid"}

RT_LIGHT_NAMES = ("point", "area", "spot", "distant", "infinite")

# SurfaceIntegrator "debug" (include/pbrt_hip.h): the integrator's value and its channel codes, in the order of the reference's DebugVariable
RT_INTEGRATOR_DEBUG = 0x100
RT_DEBUG_NAMES = ("u", "v", "nx", "ny", "nz", "snx", "sny", "snz", "one", "zero", "hit")
(RT_DEBUG_U, RT_DEBUG_V, RT_DEBUG_NX, RT_DEBUG_NY, RT_DEBUG_NZ, RT_DEBUG_SNX, RT_DEBUG_SNY, RT_DEBUG_SNZ,
 RT_DEBUG_ONE, RT_DEBUG_ZERO, RT_DEBUG_HIT) = range(11)


class RtLight(C.Structure):                        # include/pbrt_hip.h (108 bytes)
    _fields_ = [("type", C.c_int32), ("color", C.c_float * 3), ("pos", C.c_float * 3), ("n_samples", C.c_int32), ("first_tri", C.c_uint32),
                ("n_tris", C.c_uint32), ("reverse_orientation", C.c_int32), ("flip_normal", C.c_int32), ("dir", C.c_float * 3),
                ("world_to_light", C.c_float * 9), ("cos_total_width", C.c_float), ("cos_falloff_start", C.c_float), ("quadric_plus1", C.c_int32)]

class RtRenderDesc(C.Structure):                   # include/pbrt_hip.h (1128 bytes): the frame a ParsedScene hands to rt_render, ParsedScene.render_struct()
    _fields_ = [(n, C.c_int32) for n in ("integrator", "max_depth", "strategy", "volume_integrator")] + [("step_size", C.c_float)] + \
               [(n, C.c_int32) for n in ("sampler", "x_samples", "y_samples", "jitter", "pixel_samples")] + [("seed", C.c_uint32)] + \
               [(n, C.c_int32) for n in ("x_res", "y_res", "x_pixel_start", "y_pixel_start", "x_pixel_count", "y_pixel_count", "x_start", "x_end", "y_start", "y_end")] + \
               [("filter_x_width", C.c_float), ("filter_y_width", C.c_float), ("filter_table", C.c_float * 256)] + \
               [(n, C.c_int32) for n in ("shard_index", "shard_count", "tile_pixels")]


class RtHitGeometry(C.Structure):                  # include/pbrt_hip.h: six device pointers, NULL = field not wanted
    _fields_ = [(n, C.c_void_p) for n in ("p", "ng", "ns", "uv", "material", "light")]


HIT_FIELDS = ("p", "ng", "ns", "uv", "material", "light")      # DeviceScene.intersect(fields=...): name -> (columns, integer?)
_HIT_FIELD_SHAPE = {"p": (3, False), "ng": (3, False), "ns": (3, False), "uv": (2, False), "material": (0, True), "light": (0, True)}

# BxDFType bits (core/reflection.h; include/pbrt_hip.h RT_BSDF_*): the `flags` of DeviceScene.bsdf and what its `s_type` holds
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_SPECULAR, BSDF_ALL = 1, 2, 4, 8, 16, 31


class RtBsdfQuery(C.Structure):                    # include/pbrt_hip.h: device pointers, three inputs and eight outputs, NULL = not given / not wanted
    _fields_ = [(n, C.c_void_p) for n in ("wi", "u", "flags", "f", "pdf", "s_wi", "s_f", "s_pdf", "s_type", "n_components", "le")]


BSDF_FIELDS = ("f", "pdf", "s_wi", "s_f", "s_pdf", "s_type", "n_components", "le")      # DeviceScene.bsdf(fields=...): name -> (columns, integer?)
_BSDF_FIELD_SHAPE = {"f": (3, False), "pdf": (0, False), "s_wi": (3, False), "s_f": (3, False), "s_pdf": (0, False), "s_type": (0, True),
                     "n_components": (0, True), "le": (3, False)}


class RtLightQuery(C.Structure):                   # include/pbrt_hip.h: device pointers (six inputs, eight outputs; NULL = not given / not wanted) and the host value seed
    _fields_ = ([(n, C.c_void_p) for n in ("p", "nrm", "light", "u", "rng", "wi")] + [("seed", C.c_uint32)] +
                [(n, C.c_void_p) for n in ("s_wi", "s_L", "s_pdf", "s_ray", "s_draws", "pdf", "le", "is_delta")])


LIGHT_FIELDS = ("s_wi", "s_L", "s_pdf", "s_ray", "s_draws", "pdf", "le", "is_delta")      # DeviceScene.light(fields=...): name -> (columns, integer?)
_LIGHT_FIELD_SHAPE = {"s_wi": (3, False), "s_L": (3, False), "s_pdf": (0, False), "s_ray": (8, False), "s_draws": (0, True), "pdf": (0, False),
                      "le": (3, False), "is_delta": (0, True)}

class RtMediumQuery(C.Structure):                  # include/pbrt_hip.h: seven input pointers, the host values seed, step_size and volume_integrator, twelve output pointers
    _fields_ = ([(n, C.c_void_p) for n in ("p", "w", "wp", "rays", "u", "u_scatter", "rng")] +
                [("seed", C.c_uint32), ("step_size", C.c_float), ("volume_integrator", C.c_int32)] +
                [(n, C.c_void_p) for n in ("sigma_a", "sigma_s", "sigma_t", "lve", "phase", "hit", "t01", "tau", "tr", "lv", "draws", "status")])


MEDIUM_POINT_FIELDS = ("sigma_a", "sigma_s", "sigma_t", "lve", "phase")
MEDIUM_RAY_FIELDS = ("hit", "t01", "tau", "tr", "lv", "draws", "status")
MEDIUM_FIELDS = MEDIUM_POINT_FIELDS + MEDIUM_RAY_FIELDS      # DeviceScene.medium(fields=...): name -> (columns, integer?)
_MEDIUM_FIELD_SHAPE = {"sigma_a": (3, False), "sigma_s": (3, False), "sigma_t": (3, False), "lve": (3, False), "phase": (0, False), "hit": (0, True),
                       "t01": (2, False), "tau": (3, False), "tr": (3, False), "lv": (3, False), "draws": (0, True), "status": (0, True)}
VOLUME_EMISSION, VOLUME_SINGLE = 1, 2            # RT_VOLUME_*

RAY_DTYPE = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("mint", np.float32), ("maxt", np.float32)])
HIT_DTYPE = np.dtype([("prim", np.int32), ("t", np.float32), ("b1", np.float32), ("b2", np.float32)])

_hip = None
_host = None


def code_id(path: str | None = None) -> str:
    """Identity of the DEVICE code in libpbrt_hip.so: sha256 (16 hex digits) of its .hip_fatbin section (the gfx950 code objects of every
    kernel).  tools/publish_profile.py stores it with the PMC summaries under profiles/, bench.py compares it with the library it has
    loaded and refuses to print counters that were collected on other kernels."""
    import hashlib, struct
    data = open(path or HIP_LIB, "rb").read()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        raise RuntimeError("not a 64-bit ELF file: " + (path or HIP_LIB))
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    def sh(i):
        name, typ, flags, addr, off, size = struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize)
        return name, off, size
    _, stroff, _ = sh(shstrndx)
    h = hashlib.sha256()
    found = False
    for i in range(shnum):
        name, off, size = sh(i)
        end = data.index(b"\0", stroff + name)
        if data[stroff + name:end] == b".hip_fatbin":
            h.update(data[off:off + size]); found = True
    if not found:
        raise RuntimeError("no .hip_fatbin section in " + (path or HIP_LIB))
    return h.hexdigest()[:16]


def hip_lib():
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise RuntimeError("libpbrt_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(HIP_LIB)
        L.rt_last_error.restype = C.c_char_p
        for name in ("rt_scene_create", "rt_scene_destroy", "rt_scene_set_stream", "rt_scene_accel_info",
                     "rt_scene_accel_copy", "rt_camera_rays", "rt_trace_closest", "rt_trace_any", "rt_film_bind",
                     "rt_film_clear", "rt_film_read", "rt_film_resolve", "rt_render", "rt_sync", "rt_counters",
                     "rt_counters_reset", "rt_last_render_ms", "rt_last_render_stats", "rt_samples_read", "rt_device_count", "rt_set_counting",
                     "rt_kdtree_build", "rt_kdtree_info", "rt_kdtree_copy", "rt_kdtree_destroy",
                     "rt_accel_build", "rt_accel_info", "rt_accel_copy", "rt_accel_destroy", "rt_scene_create_prebuilt", "rt_film_resolve_device",
                     "rt_film_resolve_device_rgba", "rt_film_pack_parts", "rt_accel_leaf_layout", "rt_scene_set_density", "rt_scene_set_textures", "rt_scene_set_light_transforms",
                     "rt_trace_closest_device", "rt_trace_any_device", "rt_hit_geometry_device", "rt_camera_rays_device", "rt_scene_get_stream", "rt_radiance_device",
                     "rt_sample_positions_device", "rt_film_add_device", "rt_bsdf_device", "rt_light_device", "rt_medium_device", "rt_volume_samples_device"):
            getattr(L, name).restype = C.c_int
        L.rt_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.rt_scene_set_density.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_scene_set_light_transforms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_scene_set_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.rt_scene_create_prebuilt.argtypes = [C.c_void_p, C.c_int, C.POINTER(RtPrebuiltAccel), C.POINTER(C.c_void_p)]
        L.rt_scene_destroy.argtypes = [C.c_void_p]
        L.rt_scene_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_scene_accel_info.argtypes = [C.c_void_p, C.POINTER(RtAccelInfo)]
        L.rt_scene_accel_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_camera_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        L.rt_trace_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_trace_any.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_trace_closest_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_trace_any_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_hit_geometry_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RtHitGeometry)]
        L.rt_bsdf_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RtBsdfQuery)]
        L.rt_light_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtLightQuery)]
        L.rt_medium_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtMediumQuery)]
        L.rt_volume_samples_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        L.rt_camera_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        L.rt_radiance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        L.rt_sample_positions_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        L.rt_film_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        L.rt_scene_get_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.rt_film_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.rt_film_clear.argtypes = [C.c_void_p]
        L.rt_film_read.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_film_resolve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rt_render.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_film_resolve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        L.rt_film_resolve_device_rgba.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        L.rt_film_pack_parts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.rt_sync.argtypes = [C.c_void_p]
        L.rt_counters.argtypes = [C.c_void_p, C.POINTER(RtCounters)]
        L.rt_counters_reset.argtypes = [C.c_void_p]
        L.rt_last_render_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.rt_last_render_stats.argtypes = [C.c_void_p, C.POINTER(RtRenderStats)]
        L.rt_samples_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.rt_device_count.argtypes = [C.POINTER(C.c_int)]
        L.rt_set_counting.argtypes = [C.c_void_p, C.c_int]
        L.rt_kdtree_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        L.rt_kdtree_info.argtypes = [C.c_void_p, C.POINTER(RtAccelInfo)]
        L.rt_kdtree_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_kdtree_destroy.argtypes = [C.c_void_p]
        L.rt_accel_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        L.rt_accel_info.argtypes = [C.c_void_p, C.POINTER(RtAccelInfo)]
        L.rt_accel_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_accel_destroy.argtypes = [C.c_void_p]
        L.rt_accel_leaf_layout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtLeafLayoutInfo)]
        _hip = L
    return _hip


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError("libpbrt_host.so is not built (run __graft_entry__.build())")
        L = C.CDLL(HOST_LIB)
        L.pbrt_host_parse_file.restype = C.c_void_p
        L.pbrt_host_parse_file.argtypes = [C.c_char_p, C.c_int]
        L.pbrt_host_parse_string.restype = C.c_void_p
        L.pbrt_host_parse_string.argtypes = [C.c_char_p, C.c_int]
        L.pbrt_host_free.argtypes = [C.c_void_p]
        L.pbrt_host_frame_count.argtypes = [C.c_void_p]
        L.pbrt_host_frame_valid.argtypes = [C.c_void_p, C.c_int]
        L.pbrt_host_scene_desc.restype = C.c_void_p
        L.pbrt_host_scene_desc.argtypes = [C.c_void_p, C.c_int]
        L.pbrt_host_render_desc.restype = C.c_void_p
        L.pbrt_host_render_desc.argtypes = [C.c_void_p, C.c_int]
        L.pbrt_host_premultiply.argtypes = [C.c_void_p, C.c_int]
        L.pbrt_host_filename.restype = C.c_char_p
        L.pbrt_host_filename.argtypes = [C.c_void_p, C.c_int]
        L.pbrt_host_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.pbrt_host_set_seed.argtypes = [C.c_void_p, C.c_uint]
        L.pbrt_host_film_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int * 8)]
        L.pbrt_host_scene_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint * 4)]
        L.pbrt_host_camera.restype = C.POINTER(C.c_float)
        L.pbrt_host_camera.argtypes = [C.c_void_p]
        L.pbrt_host_tri_verts.restype = C.POINTER(C.c_float)
        L.pbrt_host_tri_verts.argtypes = [C.c_void_p]
        L.pbrt_host_write_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6
        L.pbrt_host_read_exr_info.argtypes = [C.c_char_p, C.POINTER(C.c_int * 6)]
        L.pbrt_host_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
        L.pbrt_host_format_f32.restype = C.c_longlong
        L.pbrt_host_format_f32.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong]
        L.pbrt_host_format_iota.restype = C.c_longlong
        L.pbrt_host_format_iota.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong]
        L.pbrt_host_accel_params.restype = C.c_void_p
        L.pbrt_host_accel_params.argtypes = [C.c_void_p]
        L.pbrt_host_volume.restype = C.POINTER(RtVolume)
        L.pbrt_host_volume.argtypes = [C.c_void_p]
        L.pbrt_host_light_to_world.restype = C.c_void_p
        L.pbrt_host_light_to_world.argtypes = [C.c_void_p, C.c_int]
        L.pbrt_host_density_desc.restype = C.POINTER(RtDensityRegion)
        L.pbrt_host_density_desc.argtypes = [C.c_void_p, C.c_int]
        L.pbrt_host_materials.restype = C.POINTER(RtMaterial)
        L.pbrt_host_materials.argtypes = [C.c_void_p]
        L.pbrt_host_material_lobes.argtypes = [C.POINTER(RtMaterial), C.POINTER(RtMaterialLobes)]
        L.pbrt_host_textures.restype = C.c_int
        L.pbrt_host_textures.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(RtTexture)), C.POINTER(C.c_uint), C.POINTER(C.POINTER(RtMaterialTextures)), C.POINTER(C.c_uint)]
        L.pbrt_host_texture_name.restype = C.c_char_p
        L.pbrt_host_texture_name.argtypes = [C.c_void_p, C.c_int, C.c_uint]
        L.pbrt_host_texture_eval.restype = C.c_int
        L.pbrt_host_texture_eval.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float)]
        L.pbrt_host_material_resolve.restype = None
        L.pbrt_host_material_resolve.argtypes = [C.POINTER(RtMaterialParams), C.POINTER(RtMaterial), C.POINTER(RtMaterialResolved)]
        L.pbrt_host_lights.restype = C.POINTER(RtLight)
        L.pbrt_host_lights.argtypes = [C.c_void_p]
        _host = L
    return _host


def write_exr(path, rgb, alpha, total_res=None, offset=(0, 0)):
    """WriteRGBAImage (core/exrio.cpp:75-96): RGBA half EXR with data/display windows (own minimal writer)."""
    rgb = np.ascontiguousarray(rgb, np.float32); alpha = np.ascontiguousarray(alpha, np.float32)
    h, w = alpha.shape
    tw, th = total_res if total_res else (w, h)
    if host_lib().pbrt_host_write_exr(path.encode(), rgb.ctypes.data, alpha.ctypes.data, w, h, tw, th, offset[0], offset[1]) != 0:
        raise IOError("cannot write " + path)


def read_exr(path):
    """ReadImage for the files write_exr / WriteRGBAImage produce: uncompressed half RGBA scanline EXR.  LIMIT: compressed files are
    refused (a message on stderr names the compression) -- in particular the PIZ files a stock pbrt-v1 linked against OpenEXR writes
    (RgbaOutputFile's default); nothing in this image can produce one to validate a decoder against."""
    info = (C.c_int * 6)()
    if host_lib().pbrt_host_read_exr_info(path.encode(), C.byref(info)) != 0:
        raise IOError("cannot read " + path)
    w, h = info[0], info[1]
    rgb = np.zeros((h, w, 3), np.float32); alpha = np.zeros((h, w), np.float32)
    host_lib().pbrt_host_read_exr(path.encode(), rgb.ctypes.data, alpha.ctypes.data)
    return rgb, alpha, dict(total_res=(info[2], info[3]), offset=(info[4], info[5]))


TRI_SHADING_DTYPE = np.dtype([("flags", np.uint32), ("xform", np.uint32), ("uv", np.float32, 6), ("n", np.float32, 9), ("s", np.float32, 9)])


def shading_records(parsed):
    """(tri_shading[n_tris] or None, RtTriShading records, xforms[n][32]) of a ParsedScene: the per-vertex uv / N / S data."""
    H = host_lib()
    H.pbrt_host_shading.restype = C.c_int
    H.pbrt_host_shading.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    idx, rec, xf, nrec, nxf = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint(), C.c_uint()
    H.pbrt_host_shading(parsed.scene_desc, C.byref(idx), C.byref(rec), C.byref(xf), C.byref(nrec), C.byref(nxf))
    if not idx.value:
        return None, np.zeros(0, TRI_SHADING_DTYPE), np.zeros((0, 32), np.float32)
    i = np.ctypeslib.as_array(C.cast(idx, C.POINTER(C.c_int32)), shape=(parsed.n_tris,)).copy()
    r = np.frombuffer(C.string_at(rec, nrec.value * TRI_SHADING_DTYPE.itemsize), TRI_SHADING_DTYPE).copy()
    x = np.ctypeslib.as_array(C.cast(xf, C.POINTER(C.c_float)), shape=(nxf.value, 32)).copy() if nxf.value else np.zeros((0, 32), np.float32)
    return i, r, x


def format_f32(values, per_line: int = 9) -> str:
    """Scene-text numbers ("%.9g": round-trips float32) formatted by the host library: 1 s for a 1 M-triangle mesh."""
    v = np.ascontiguousarray(values, np.float32).ravel()
    buf = C.create_string_buffer(int(v.size) * 17 + 64)
    n = host_lib().pbrt_host_format_f32(v.ctypes.data, v.size, per_line, buf, len(buf))
    if n < 0:
        raise RuntimeError("format_f32: buffer too small")
    return buf.raw[:n].decode()


def format_iota(first: int, count: int, per_line: int = 3) -> str:
    buf = C.create_string_buffer(int(count) * 12 + 64)
    n = host_lib().pbrt_host_format_iota(first, count, per_line, buf, len(buf))
    if n < 0:
        raise RuntimeError("format_iota: buffer too small")
    return buf.raw[:n].decode()


def assemble_exr(paths, out) -> float:
    """tools/exrassemble.cpp: merge crop-window EXRs into the display-window image; returns the covered fraction.  LIMIT: the inputs
    must be uncompressed half RGBA scanline files (this library's own output); PIZ tiles written by a stock pbrt are refused, see read_exr."""
    H = host_lib()
    H.pbrt_host_assemble_exr.restype = C.c_float
    H.pbrt_host_assemble_exr.argtypes = [C.c_char_p, C.c_char_p]
    r = H.pbrt_host_assemble_exr("\n".join(paths).encode(), out.encode())
    if r < 0:
        raise IOError("cannot assemble " + out)
    return float(r)


def publish_accel(ds: "DeviceScene", path: str) -> None:
    """Rank 0 of a node: write the accelerator of `ds` where the other ranks can map it (e.g. under /dev/shm): one file, header
    (RtAccelInfo bytes) + nodes + leaf refs, renamed into place when complete."""
    info = ds.accel_info()
    need = 256 + 8 * int(info.n_nodes) + 4 * int(info.n_leaf_refs)
    st = os.statvfs(os.path.dirname(path) or ".")
    if st.f_bavail * st.f_frsize < need + (64 << 20):
        raise OSError("publish_accel: %s has %d MB free, the accelerator needs %d MB" % (os.path.dirname(path), st.f_bavail * st.f_frsize >> 20, need >> 20))
    nodes, refs = ds.accel_arrays()
    tmp = path + ".tmp%d" % os.getpid()
    try:
        with open(tmp, "wb") as f:
            f.write(bytes(info).ljust(256, b"\0"))
            np.ascontiguousarray(nodes, np.uint32).tofile(f); np.ascontiguousarray(refs, np.uint32).tofile(f)     # (no second copy in memory: 6 GB at 10 M triangles)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def attach_accel(path: str):
    """The other ranks: (nodes, leaf_refs, RtAccelInfo) mapped read-only from a file written by publish_accel."""
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    info = RtAccelInfo.from_buffer_copy(bytes(raw[:C.sizeof(RtAccelInfo)]))
    nodes = np.frombuffer(raw, np.uint32, count=2 * info.n_nodes, offset=256).reshape(-1, 2)
    refs = np.frombuffer(raw, np.uint32, count=info.n_leaf_refs, offset=256 + 8 * info.n_nodes)
    return nodes, refs, info


class RtError(RuntimeError):
    pass


def _chk(rc):
    if rc != 0:
        raise RtError("rt error %d: %s" % (rc, hip_lib().rt_last_error().decode()))


def device_count() -> int:
    n = C.c_int(0)
    rc = hip_lib().rt_device_count(C.byref(n))
    return int(n.value) if rc == 0 else 0


def build_kdtree(tri_verts: np.ndarray, accel_params_ptr=None):
    """Host-only kd-tree build (rt_kdtree_build).  Returns (nodes[n,2] u32, leaf_refs u32, bounds[6], info)."""
    tv = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    t = C.c_void_p()
    _chk(hip_lib().rt_accel_build(tv.ctypes.data, len(tv), accel_params_ptr, C.byref(t)))
    info = RtAccelInfo()
    _chk(hip_lib().rt_accel_info(t, C.byref(info)))
    nodes = np.zeros((info.n_nodes, 2), np.uint32)
    refs = np.zeros(max(info.n_leaf_refs, 1), np.uint32)
    _chk(hip_lib().rt_accel_copy(t, nodes.ctypes.data, refs.ctypes.data))
    hip_lib().rt_accel_destroy(t)
    return nodes, refs[:info.n_leaf_refs], np.array(list(info.bounds), np.float32), info


def leaf_layout(tri_verts: np.ndarray, accel_params_ptr=None, runs: bool = False, copies: bool = False):
    """Host-only: the kd-tree of `tri_verts` and its leaves as rt_scene_create lays them out for the flat traversal (rt_accel_leaf_layout).
    Returns (nodes[n,2], leaf_refs, tnodes[n,2], slot_prim, entries, stride)."""
    tv = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    t = C.c_void_p()
    _chk(hip_lib().rt_accel_build(tv.ctypes.data, len(tv), accel_params_ptr, C.byref(t)))
    try:
        info = RtAccelInfo()
        _chk(hip_lib().rt_accel_info(t, C.byref(info)))
        nodes = np.zeros((info.n_nodes, 2), np.uint32)
        refs = np.zeros(max(info.n_leaf_refs, 1), np.uint32)
        _chk(hip_lib().rt_accel_copy(t, nodes.ctypes.data, refs.ctypes.data))
        li = RtLeafLayoutInfo()
        _chk(hip_lib().rt_accel_leaf_layout(t, int(runs), int(copies), None, None, None, C.byref(li)))
        tn = np.zeros((li.n_nodes, 2), np.uint32); sp = np.zeros(max(li.n_slots, 1), np.uint32); en = np.zeros(max(li.n_entries, 1), np.uint32)
        _chk(hip_lib().rt_accel_leaf_layout(t, int(runs), int(copies), tn.ctypes.data, sp.ctypes.data, en.ctypes.data, C.byref(li)))
    finally:
        hip_lib().rt_accel_destroy(t)
    return nodes, refs[:info.n_leaf_refs], tn, sp[:li.n_slots], en[:li.n_entries], int(li.stride)


def fit_tile(extent: int, size: int) -> int:
    """The tile size in [3/4, 5/4] of `size` whose whole tiles overshoot `extent` least (ties: the one nearest `size`)."""
    best = None
    for t in range(max(1, size * 3 // 4), max(2, size * 5 // 4) + 1):
        pad = -(-extent // t) * t - extent
        key = (pad, abs(t - size))
        if best is None or key < best[0]:
            best = (key, t)
    return best[1]


class ParsedScene:
    """A .pbrt description run through the host API mirror (scene_api.cpp): flat scene + frame descriptors."""

    def __init__(self, text: str | None = None, path: str | None = None, quiet: bool = True, frame: int = 0):
        H = host_lib()
        if path is not None:
            self._h = H.pbrt_host_parse_file(path.encode(), int(quiet))
        else:
            from . import scenes as _scenes
            text = _scenes.for_product(text)      # texts written for runs of the compiled reference wrap the sampler / accelerator in oracle-side plugins
            self._h = H.pbrt_host_parse_string(text.encode(), int(quiet))
        self.warnings = H.pbrt_host_warnings()
        self.errors = H.pbrt_host_errors()
        self.n_frames = H.pbrt_host_frame_count(self._h)
        if self.n_frames == 0:
            raise RtError("scene description has no WorldEnd (errors: %d)" % self.errors)
        self.frame = frame
        self.valid = bool(H.pbrt_host_frame_valid(self._h, frame))
        self.scene_desc = H.pbrt_host_scene_desc(self._h, frame)
        self.render_desc = H.pbrt_host_render_desc(self._h, frame)
        self.premultiply = bool(H.pbrt_host_premultiply(self._h, frame))
        dims = (C.c_int * 8)()
        H.pbrt_host_film_dims(self.render_desc, C.byref(dims))
        self.width, self.height = dims[0], dims[1]
        self.sample_extent = (dims[2], dims[3], dims[4], dims[5])
        self.spp = dims[6]
        self.integrator = dims[7]
        cnt = (C.c_uint * 4)()
        H.pbrt_host_scene_counts(self.scene_desc, C.byref(cnt))
        self.n_tris, self.n_materials, self.n_lights, self.n_light_tris = (int(c) for c in cnt)

    @property
    def n_camera_samples(self) -> int:
        x0, x1, y0, y1 = self.sample_extent
        return (x1 - x0) * (y1 - y0) * self.spp

    def render_struct(self) -> RtRenderDesc:
        """This frame's RtRenderDesc in place (not a copy): a field written here is what the next rt_render is given."""
        return C.cast(self.render_desc, C.POINTER(RtRenderDesc)).contents

    @property
    def debug_channels(self):
        """("red", "green", "blue") names of a SurfaceIntegrator "debug" frame (RtRenderDesc.strategy = red | green << 8 | blue << 16, read from
        the descriptor as it stands), None for every other integrator."""
        v = self.render_view()
        if v["integrator"] != RT_INTEGRATOR_DEBUG:
            return None
        return tuple(RT_DEBUG_NAMES[c] if c < len(RT_DEBUG_NAMES) else "?" for c in ((v["strategy"] >> (8 * i)) & 0xff for i in range(3)))

    def set_shard(self, index: int, count: int, tile_pixels=64, fit: bool = False):
        """tile_pixels: an int = tiles of that many consecutive pixels of the sample extent (scanline order); a pair (w, h) = 2-D tiles of
        w x h pixels (RtRenderDesc.tile_pixels = -(w | h << 16)).  fit: adjust w and h (within 3/4 .. 5/4 of the request) to the sizes that
        pad the sample extent least -- border tiles are whole tiles whose pixels outside the extent are fetched and dropped, a lane idling for
        about a ray's time per dropped work item (64 x 64 tiles pad a 1025 x 1025 extent by 12.7 %, 61 x 61 by 2.4 %).  Every rank of a job
        computes the same sizes.  Returns the tile size used."""
        if isinstance(tile_pixels, (tuple, list)):
            w, h = int(tile_pixels[0]), int(tile_pixels[1])
            if fit:
                x0, x1, y0, y1 = self.sample_extent
                w, h = fit_tile(x1 - x0, w), fit_tile(y1 - y0, h)
            used = (w, h)
            tile_pixels = -(w | (h << 16))
        else:
            used = int(tile_pixels)
        host_lib().pbrt_host_set_shard(self.render_desc, index, count, int(tile_pixels))
        return used

    def set_seed(self, seed: int):
        host_lib().pbrt_host_set_seed(self.render_desc, seed)

    def camera_matrices(self):
        p = host_lib().pbrt_host_camera(self.scene_desc)
        a = np.ctypeslib.as_array(p, shape=(32,)).copy()
        return a[:16].reshape(4, 4), a[16:].reshape(4, 4)

    def accel_params_ptr(self):
        return host_lib().pbrt_host_accel_params(self.scene_desc)

    def accel_params(self) -> dict:
        """RtAccelParams of this frame (include/pbrt_hip.h)."""
        a = np.ctypeslib.as_array(C.cast(self.accel_params_ptr(), C.POINTER(C.c_int32)), shape=(7,))
        return {"kind": int(a[0]), "isect_cost": int(a[1]), "trav_cost": int(a[2]), "max_prims": int(a[3]), "max_depth": int(a[4]),
                "empty_bonus": float(a[5:6].view(np.float32)[0]), "build_threads": int(a[6])}

    def render_view(self) -> dict:
        """The leading scalar fields of this frame's RtRenderDesc (include/pbrt_hip.h): integrator .. seed."""
        a = np.ctypeslib.as_array(C.cast(self.render_desc, C.POINTER(C.c_int32)), shape=(11,))
        return {"integrator": int(a[0]), "max_depth": int(a[1]), "strategy": int(a[2]), "volume_integrator": int(a[3]),
                "step_size": float(a[4:5].view(np.float32)[0]), "sampler": int(a[5]), "x_samples": int(a[6]), "y_samples": int(a[7]),
                "jitter": int(a[8]), "pixel_samples": int(a[9]), "seed": int(a[10:11].view(np.uint32)[0])}

    def volume(self) -> dict | None:
        """The frame's medium as RtVolume carries it (include/pbrt_hip.h), or None without one: world_to_volume (4x4, row-major), the
        extent p0 / p1, sigma_a, sigma_s, Le, g, and `density`: the DensityRegion handed to rt_scene_set_density (kind "exponential" with
        a, b and the normalised updir, or "volumegrid" with nx, ny, nz and the values [nz][ny][nx]), None for a homogeneous medium."""
        v = host_lib().pbrt_host_volume(self.scene_desc).contents
        if not v.present:
            return None
        out = {"world_to_volume": np.array(v.world_to_volume, np.float32).reshape(4, 4), "p0": list(v.p0), "p1": list(v.p1),
               "sigma_a": list(v.sigma_a), "sigma_s": list(v.sigma_s), "le": list(v.le), "g": float(v.g), "density": None}
        dp = self.density_desc()
        if dp:
            d = dp.contents
            dens = {"kind": RT_DENSITY_NAMES[d.kind]}
            if d.kind == 1:
                dens.update(a=float(d.a), b=float(d.b), updir=[float(x) for x in d.updir])
            else:
                dens.update(nx=int(d.nx), ny=int(d.ny), nz=int(d.nz),
                            values=np.ctypeslib.as_array(d.density, shape=(d.nz, d.ny, d.nx)).copy())
            out["density"] = dens
        return out

    def materials(self) -> list:
        """The parsed material table (RtMaterial, include/pbrt_hip.h) as dictionaries: `type` (the material's name) and its parameters as
        float32 arrays / floats under the reference's parameter names, after .Clamp() and with textures and shape parameters resolved.
        shinymetal and translucent also carry what rt_scene_create derives from them (include/pbrt_hip_material.h): `eta_Ks`, `eta_Kr`
        (FresnelApproxEta), or the products `reflect*Kd`, `transmit*Kd`, `reflect*Ks`, `transmit*Ks` and `lobes`, the lobes present in the
        order the BSDF holds them."""
        H = host_lib()
        tab = H.pbrt_host_materials(self.scene_desc)
        f3 = lambda a: np.array(list(a), np.float32)
        out = []
        for i in range(self.n_materials):
            m = tab[i]
            name = RT_MATERIAL_NAMES[m.type]
            d = {"type": name}
            if name == "matte":
                d.update(Kd=f3(m.kd), sigma=float(m.sigma))
            elif name == "mirror":
                d.update(Kr=f3(m.kd))
            elif name == "glass":
                d.update(Kr=f3(m.kd), Kt=f3(m.kt), index=float(m.ior))
            elif name == "plastic":
                d.update(Kd=f3(m.kd), Ks=f3(m.ks), roughness=float(m.roughness))
            elif name == "uber":          # the colours as the descriptor holds them: opacity already multiplied in (include/pbrt_hip.h)
                d.update({"opacity*Kd": f3(m.kd), "opacity*Ks": f3(m.ks), "opacity*Kr": f3(m.kr), "1-opacity": f3(m.kt), "roughness": float(m.roughness)})
            else:
                lb = RtMaterialLobes()
                H.pbrt_host_material_lobes(C.byref(m), C.byref(lb))
                if name == "shinymetal":
                    d.update(Ks=f3(m.ks), Kr=f3(m.kr), roughness=float(m.roughness), eta_Ks=f3(lb.eta_ks), eta_Kr=f3(lb.eta_kr),
                             lobes=["glossy_reflection", "specular_reflection"])
                else:
                    d.update({"Kd": f3(m.kd), "Ks": f3(m.ks), "reflect": f3(m.kr), "transmit": f3(m.kt), "roughness": float(m.roughness),
                              "reflect*Kd": f3(lb.r_kd), "transmit*Kd": f3(lb.t_kd), "reflect*Ks": f3(lb.r_ks), "transmit*Ks": f3(lb.t_ks)})
                    d["lobes"] = [n for n, on in (("diffuse_reflection", lb.has_dr), ("diffuse_transmission", lb.has_dt),
                                                  ("glossy_reflection", lb.has_gr), ("glossy_transmission", lb.has_gt)) if on]
            out.append(d)
        if self.has_textures():                   # slots a texture supplies at every hit: parameter name -> index into textures(); their values above are the literals / defaults
            _, _, mats, _ = self.texture_table()
            for i, d in enumerate(out):
                d["textured"] = {pn: int(mats[i].tex[k]) for k, pn in enumerate(RT_MATERIAL_SLOTS[d["type"]]) if pn is not None and mats[i].tex[k] >= 0}
        return out

    def texture_table(self):
        """(nodes, n_nodes, mats, n_mats): the frame's RtTexture / RtMaterialTextures arrays as rt_scene_set_textures takes them (owned by this object)."""
        if getattr(self, "_tex_table", None) is None:
            nodes = C.POINTER(RtTexture)(); mats = C.POINTER(RtMaterialTextures)(); nn = C.c_uint(); nm = C.c_uint()
            used = host_lib().pbrt_host_textures(self._h, self.frame, C.byref(nodes), C.byref(nn), C.byref(mats), C.byref(nm))
            self._tex_table = (nodes, int(nn.value), mats, int(nm.value), bool(used))
        return self._tex_table[:4]

    def has_textures(self) -> bool:
        """Does some material have a parameter that a non-constant texture supplies?  Only then is the texture table handed to the device."""
        self.texture_table()
        return self._tex_table[4]

    def textures(self) -> list:
        """The parsed texture table (children before parents) as dictionaries: `name` (of its Texture statement; "" for a literal sub-texture),
        `class`, `type` ("float" / "color") and per class `value` | `tex1`, `tex2`, `amount` (node indices) | `v00` .. `v11` | `mapping` with
        its parameters (`uscale`, `vscale`, `udelta`, `vdelta` | `v1`, `v2`, `udelta`, `vdelta` | `world_to_texture`).  Constant textures a
        Texture statement names are folded into the parameters that use them and do not appear."""
        if getattr(self, "_tex_list", None) is not None:
            return self._tex_list
        nodes, n, _, _ = self.texture_table()
        f = lambda a: np.array(list(a), np.float32)
        out = []
        for i in range(n):
            t = nodes[i]
            cls = RT_TEXTURE_NAMES[t.kind]
            col = bool(t.is_color)
            val = lambda k: f(t.value[3 * k:3 * k + 3]) if col else float(t.value[3 * k])
            d = {"name": host_lib().pbrt_host_texture_name(self._h, self.frame, i).decode(), "class": cls, "type": "color" if col else "float"}
            if cls == "constant":
                d["value"] = val(0)
            if cls in ("scale", "mix", "checkerboard"):
                d.update(tex1=int(t.child[0]), tex2=int(t.child[1]))
            if cls == "mix":
                d["amount"] = int(t.child[2])
            if cls == "bilerp":
                d.update(v00=val(0), v01=val(1), v10=val(2), v11=val(3))
            if cls in ("bilerp", "uv", "checkerboard"):
                mp = RT_TEXMAP_NAMES[t.mapping]
                d["mapping"] = mp
                if mp == "uv":
                    d.update(uscale=float(t.map[0]), vscale=float(t.map[1]), udelta=float(t.map[2]), vdelta=float(t.map[3]))
                elif mp == "planar":
                    d.update(v1=f(t.map[0:3]), v2=f(t.map[3:6]), udelta=float(t.map[6]), vdelta=float(t.map[7]))
                else:
                    d["world_to_texture"] = f(t.world_to_texture).reshape(4, 4)
            out.append(d)
        self._tex_list = out                      # (the parsed table does not change: built once)
        return out

    def eval_texture(self, which, p, u: float, v: float):
        """Host evaluation of a texture (index into textures(), or the name of a Texture statement: the last node of that name) at the world
        point `p` with the surface parameters (u, v) -- the function the device runs (include/pbrt_hip_texture.h), compiled for the host.
        Returns a float for a float texture, a float32 array of 3 for a colour texture."""
        tab = self.textures()
        if isinstance(which, str):
            idx = [i for i, t in enumerate(tab) if t["name"] == which]
            if not idx:
                raise KeyError("no texture named %r" % which)
            which = idx[-1]
        pp = (C.c_float * 3)(*[float(x) for x in p]); out = (C.c_float * 3)()
        if host_lib().pbrt_host_texture_eval(self._h, self.frame, int(which), pp, float(u), float(v), out) != 0:
            raise RtError("texture %r cannot be evaluated (bad index, or a graph beyond RT_TEX_MAX_PROGRAM / RT_TEX_MAX_STACK)" % (which,))
        return np.array(list(out), np.float32) if tab[which]["type"] == "color" else float(np.float32(out[0]))

    def lights(self) -> list:
        """The parsed light table (RtLight, include/pbrt_hip.h) in scene order as dictionaries: `type` (the light's name), `nsamples` and its
        colour as a float32 array under the reference's parameter name (`I` point / spot, `L` area / distant / infinite); point and spot
        lights also carry `from` (world space), distant lights `dir`, area lights `n_tris`."""
        tab = host_lib().pbrt_host_lights(self.scene_desc)
        f3 = lambda a: np.array(list(a), np.float32)
        out = []
        for i in range(self.n_lights):
            l = tab[i]
            name = RT_LIGHT_NAMES[l.type]
            d = {"type": name, "nsamples": int(l.n_samples), ("I" if name in ("point", "spot") else "L"): f3(l.color)}
            if name in ("point", "spot"):
                d["from"] = f3(l.pos)
            elif name == "distant":
                d["dir"] = f3(l.dir)
            elif name == "area":
                d["n_tris"] = int(l.n_tris)
            out.append(d)
        return out

    def density_desc(self):
        """Pointer to the frame's RtDensityRegion (pbrt_host_density_desc), or a null pointer when the medium is homogeneous or absent."""
        return host_lib().pbrt_host_density_desc(self._h, self.frame)

    def kdtree(self):
        """The kd-tree rt_scene_create would build for this scene, built on the host only."""
        return build_kdtree(self.tri_verts(), self.accel_params_ptr())

    def tri_verts(self):
        if self.n_tris == 0:
            return np.zeros((0, 3, 3), np.float32)
        p = host_lib().pbrt_host_tri_verts(self.scene_desc)
        return np.ctypeslib.as_array(p, shape=(self.n_tris, 3, 3)).copy()

    def tri_tables(self):
        """(tri_material uint16 [n_tris], tri_light int32 [n_tris]) of the flat scene (RtSceneDesc, include/pbrt_hip.h): per primitive the index
        into materials() and the area-light index or -1 -- what DeviceScene.intersect returns as `material` and `light` for a hit on it."""
        class _Head(C.Structure):                  # the leading fields of RtSceneDesc
            _fields_ = [("n_tris", C.c_uint32), ("tri_verts", C.c_void_p), ("tri_material", C.POINTER(C.c_uint16)), ("tri_light", C.POINTER(C.c_int32))]
        h = C.cast(self.scene_desc, C.POINTER(_Head)).contents
        if h.n_tris == 0:
            return np.zeros(0, np.uint16), np.zeros(0, np.int32)
        return (np.ctypeslib.as_array(h.tri_material, shape=(h.n_tris,)).copy(), np.ctypeslib.as_array(h.tri_light, shape=(h.n_tris,)).copy())

    def serialize(self) -> bytes:
        """Canonical byte image of this frame's descriptors (include/pbrt_hip_desc.h rt_desc_serialize)."""
        H = host_lib()
        H.pbrt_host_serialize.restype = C.c_longlong
        H.pbrt_host_serialize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        n = H.pbrt_host_serialize(self._h, self.frame, None, 0)
        buf = C.create_string_buffer(int(n))
        H.pbrt_host_serialize(self._h, self.frame, buf, n)
        return buf.raw

    def close(self):
        if self._h:
            host_lib().pbrt_host_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceScene:
    """rt_scene_create: kd-tree build + upload.  Holds the film unless one is bound externally."""

    def __init__(self, parsed: ParsedScene, device: int = -1, prebuilt=None):
        """prebuilt = (nodes[n][2] uint32, leaf_refs uint32, RtAccelInfo) of an accelerator built elsewhere (another rank's
        DeviceScene.accel_arrays() / accel_info(), e.g. through publish_accel / attach_accel): rt_scene_create_prebuilt."""
        self.parsed = parsed
        self._s = C.c_void_p()
        self._device = device
        if prebuilt is None:
            _chk(hip_lib().rt_scene_create(parsed.scene_desc, device, C.byref(self._s)))
        else:
            nodes, refs, info = prebuilt
            nodes = np.ascontiguousarray(nodes, np.uint32); refs = np.ascontiguousarray(refs if len(refs) else np.zeros(1, np.uint32), np.uint32)
            pa = RtPrebuiltAccel(kind=info.kind, n_nodes=info.n_nodes, n_leaf_refs=info.n_leaf_refs, max_depth=info.max_depth,
                                 nodes=nodes.ctypes.data, leaf_refs=refs.ctypes.data)
            for i in range(6): pa.bounds[i] = info.bounds[i]
            for i in range(3):
                pa.grid_nvoxels[i] = info.grid_nvoxels[i]; pa.grid_width[i] = info.grid_width[i]; pa.grid_inv_width[i] = info.grid_inv_width[i]
            _chk(hip_lib().rt_scene_create_prebuilt(parsed.scene_desc, device, C.byref(pa), C.byref(self._s)))
        l2w = host_lib().pbrt_host_light_to_world(parsed._h, parsed.frame)
        if l2w:                                   # spot lights: LightToWorld as the reference holds it (the bidirectional integrator's emission rays)
            rc = hip_lib().rt_scene_set_light_transforms(self._s, l2w, parsed.n_lights)
            if rc != 0:
                err = hip_lib().rt_last_error().decode(errors="replace")
                hip_lib().rt_scene_destroy(self._s); self._s = C.c_void_p()
                raise RtError("rt_scene_set_light_transforms failed (%d): %s" % (rc, err))
        dens = parsed.density_desc()
        if dens:                                  # an exponential / volumegrid medium: DensityRegion on top of the scene's RtVolume
            rc = hip_lib().rt_scene_set_density(self._s, dens)
            if rc != 0:
                err = hip_lib().rt_last_error().decode(errors="replace")
                hip_lib().rt_scene_destroy(self._s); self._s = C.c_void_p()
                raise RtError("rt_scene_set_density failed (%d): %s" % (rc, err))
        if parsed.has_textures():                 # textured material parameters: the node table and the per-material slots
            nodes, n_nodes, mats, n_mats = parsed.texture_table()
            rc = hip_lib().rt_scene_set_textures(self._s, nodes, n_nodes, mats, n_mats)
            if rc != 0:
                err = hip_lib().rt_last_error().decode(errors="replace")
                hip_lib().rt_scene_destroy(self._s); self._s = C.c_void_p()
                raise RtError("rt_scene_set_textures failed (%d): %s" % (rc, err))
        self._film_bound = False

    def accel_info(self) -> RtAccelInfo:
        info = RtAccelInfo()
        _chk(hip_lib().rt_scene_accel_info(self._s, C.byref(info)))
        return info

    def accel_arrays(self):
        info = self.accel_info()
        nodes = np.zeros((info.n_nodes, 2), np.uint32)
        refs = np.zeros(max(info.n_leaf_refs, 1), np.uint32)
        _chk(hip_lib().rt_scene_accel_copy(self._s, nodes.ctypes.data, refs.ctypes.data))
        return nodes, refs[:info.n_leaf_refs]

    def set_stream(self, stream_ptr: int):
        _chk(hip_lib().rt_scene_set_stream(self._s, C.c_void_p(stream_ptr)))

    def bind_film(self, device_ptr: int | None = None):
        _chk(hip_lib().rt_film_bind(self._s, C.c_void_p(device_ptr) if device_ptr else None,
                                     self.parsed.width, self.parsed.height))
        self._film_bound = True

    def clear_film(self):
        _chk(hip_lib().rt_film_clear(self._s))

    def render(self, sync: bool = True):
        if not self._film_bound:
            self.bind_film()
        _chk(hip_lib().rt_render(self._s, self.parsed.render_desc))
        if sync:
            self.sync()

    def sync(self):
        _chk(hip_lib().rt_sync(self._s))

    def resolve_device(self, accum_ptr: int, n: int, rgb_ptr: int, alpha_ptr: int, premultiply: bool | None = None):
        """rt_film_resolve_device: WriteImage's normalisation of a 5-plane accumulator (planes of n floats) in device memory."""
        pm = self.parsed.premultiply if premultiply is None else premultiply
        _chk(hip_lib().rt_film_resolve_device(self._s, C.c_void_p(accum_ptr), n, int(pm), C.c_void_p(rgb_ptr), C.c_void_p(alpha_ptr)))

    def resolve_device_rgba(self, accum_ptr: int, n: int, rgba_ptr: int, premultiply: bool | None = None):
        """rt_film_resolve_device_rgba: the same, interleaved RGBA [n][4] (the payload of one all-gather)."""
        pm = self.parsed.premultiply if premultiply is None else premultiply
        _chk(hip_lib().rt_film_resolve_device_rgba(self._s, C.c_void_p(accum_ptr), n, int(pm), C.c_void_p(rgba_ptr)))

    def pack_parts(self, accum_ptr: int, world: int, rows: int, parts_ptr: int):
        """rt_film_pack_parts: this rank's 5-plane film as `world` parts of `rows` rows, part r = [5][rows][W] (the send buffer of one reduce-scatter)."""
        _chk(hip_lib().rt_film_pack_parts(self._s, C.c_void_p(accum_ptr), self.parsed.width, self.parsed.height, world, rows, C.c_void_p(parts_ptr)))

    def film_accum(self) -> np.ndarray:
        out = np.zeros((5, self.parsed.height, self.parsed.width), np.float32)
        _chk(hip_lib().rt_film_read(self._s, out.ctypes.data))
        return out

    def film(self, premultiply: bool | None = None, out=None):
        """rt_film_resolve: the film as ImageFilm::WriteImage hands it to the image writer.  `out` = (rgb[H,W,3], alpha[H,W])
        float32 C-contiguous arrays to fill (e.g. views of page-locked memory, reused across frames); allocated if omitted."""
        h, w = self.parsed.height, self.parsed.width
        if out is None:
            rgb = np.empty((h, w, 3), np.float32); alpha = np.empty((h, w), np.float32)
        else:
            rgb, alpha = out
            if rgb.shape != (h, w, 3) or alpha.shape != (h, w) or rgb.dtype != np.float32 or alpha.dtype != np.float32 \
                    or not rgb.flags.c_contiguous or not alpha.flags.c_contiguous:
                raise ValueError("film(out=...): need C-contiguous float32 arrays of shape (H,W,3) and (H,W)")
        pm = self.parsed.premultiply if premultiply is None else premultiply
        _chk(hip_lib().rt_film_resolve(self._s, int(pm), rgb.ctypes.data, alpha.ctypes.data))
        return rgb, alpha

    def counters(self) -> dict:
        c = RtCounters()
        _chk(hip_lib().rt_counters(self._s, C.byref(c)))
        return c.as_dict()

    def set_counting(self, enabled: bool):
        _chk(hip_lib().rt_set_counting(self._s, int(enabled)))

    def reset_counters(self):
        _chk(hip_lib().rt_counters_reset(self._s))

    def last_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        _chk(hip_lib().rt_last_render_ms(self._s, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def samples(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """The per-camera-sample records of the last render: [n][8] = L.rgb, alpha, imageX, imageY, -, - in the sampler's order."""
        n = self.parsed.n_camera_samples - first if count is None else count
        out = np.zeros((n, 8), np.float32)
        _chk(hip_lib().rt_samples_read(self._s, first, n, out.ctypes.data))
        return out

    def last_stats(self) -> dict:
        st = RtRenderStats()
        _chk(hip_lib().rt_last_render_stats(self._s, C.byref(st)))
        return st.as_dict()

    def camera_rays(self, first: int, count: int) -> np.ndarray:
        rays = np.zeros(count, RAY_DTYPE)
        _chk(hip_lib().rt_camera_rays(self._s, self.parsed.render_desc, first, count, rays.ctypes.data))
        return rays

    def trace_closest(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        _chk(hip_lib().rt_trace_closest(self._s, rays.ctypes.data, len(rays), hits.ctypes.data))
        return hits

    def trace_any(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        occ = np.zeros(len(rays), np.uint8)
        _chk(hip_lib().rt_trace_any(self._s, rays.ctypes.data, len(rays), occ.ctypes.data))
        return occ

    # ---- rays and hits in device memory (include/pbrt_hip.h, "Rays and hits in DEVICE memory"): torch tensors in, torch tensors out.  The library's
    # calls are asynchronous on the scene's stream, which is not ordered against torch's: each wrapper makes the scene's stream wait for torch's
    # current stream before its launches and torch's current stream wait for the scene's after them (events, no host synchronisation), so the
    # next torch op may use the result.  torch is imported only here.  A process that uses them imports torch BEFORE this package loads libpbrt_hip.so (hip_lib():
    # the first DeviceScene), as bench.py does: torch carries a HIP runtime of its own, the first one loaded serves both, and a stream of one
    # runtime means nothing to another (loaded after the library, torch finds no device at all).
    @staticmethod
    def _check_ray_tensor(torch, rays, device):
        if not isinstance(rays, torch.Tensor):
            raise ValueError("rays: a torch tensor is needed, got %s" % type(rays).__name__)
        if rays.dtype != torch.float32:
            raise ValueError("rays: dtype float32 is needed, got %s" % rays.dtype)
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError("rays: shape [n, 8] (o, d, mint, maxt) is needed, got %s" % (tuple(rays.shape),))
        if not rays.is_contiguous():
            raise ValueError("rays: a contiguous tensor is needed")
        if not rays.is_cuda:
            raise ValueError("rays: a tensor in device memory is needed, got one on %s" % rays.device)
        if device is not None and device >= 0 and rays.device.index != device:
            raise ValueError("rays: the tensor is on %s, the scene on device %d" % (rays.device, device))

    def _scene_stream(self, torch, device):
        """(torch's current stream, the scene's stream as a torch stream or None when they are the same)"""
        p = C.c_void_p()
        _chk(hip_lib().rt_scene_get_stream(self._s, C.byref(p)))
        cur = torch.cuda.current_stream(device)
        if (p.value or 0) == cur.cuda_stream:
            return cur, None
        return cur, (torch.cuda.ExternalStream(p.value, device=device) if p.value else torch.cuda.default_stream(device))

    def intersect(self, rays, fields=HIT_FIELDS) -> dict:
        """Scene::Intersect for rays in device memory (rt_trace_closest_device) and the hit geometry asked for (rt_hit_geometry_device).
        rays: contiguous float32 [n, 8] torch tensor on the scene's device.  Returns torch tensors on that device: `prim` (int32 [n], -1 = miss),
        `t`, `b1`, `b2` (float32 [n]; views of one [n, 4] record array) and per requested field `p`, `ng`, `ns` (float32 [n, 3]), `uv` ([n, 2]),
        `material`, `light` (int32 [n]).  fields=() gives the hits only."""
        import torch
        fields = tuple(fields)
        for f in fields:
            if f not in _HIT_FIELD_SHAPE:
                raise ValueError("fields: unknown field %r (known: %s)" % (f, ", ".join(HIT_FIELDS)))
        self._check_ray_tensor(torch, rays, getattr(self, "_device", None))
        n, dev = int(rays.shape[0]), rays.device
        hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        extra = {f: (torch.empty(n, dtype=torch.int32, device=dev) if _HIT_FIELD_SHAPE[f][1] else torch.empty((n, _HIT_FIELD_SHAPE[f][0]), dtype=torch.float32, device=dev))
                 for f in fields}
        if n:
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_trace_closest_device(self._s, C.c_void_p(rays.data_ptr()), n, C.c_void_p(hits.data_ptr())))
            if fields:
                g = RtHitGeometry(**{f: t.data_ptr() for f, t in extra.items()})
                _chk(hip_lib().rt_hit_geometry_device(self._s, C.c_void_p(rays.data_ptr()), C.c_void_p(hits.data_ptr()), n, C.byref(g)))
            if mine is not None:
                cur.wait_stream(mine)
        out = {"prim": hits.view(torch.int32)[:, 0], "t": hits[:, 1], "b1": hits[:, 2], "b2": hits[:, 3]}
        out.update(extra)
        return out

    @staticmethod
    def _check_query_tensor(torch, t, name, n, cols, dtype, like):
        """an input of bsdf() beside the rays: the checks of _check_ray_tensor for a [n, cols] (cols = 0: [n]) tensor of `dtype` on the rays' device"""
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: a torch tensor is needed, got %s" % (name, type(t).__name__))
        if t.dtype != dtype:
            raise ValueError("%s: dtype %s is needed, got %s" % (name, dtype, t.dtype))
        shape = (n, cols) if cols else (n,)
        if tuple(t.shape) != shape:
            raise ValueError("%s: shape %s is needed, got %s" % (name, list(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s: a contiguous tensor is needed" % name)
        if t.device != like.device:
            raise ValueError("%s: the tensor is on %s, the rays on %s" % (name, t.device, like.device))

    def bsdf(self, rays, hits, wi=None, u=None, flags=None, fields=BSDF_FIELDS) -> dict:
        """What an integrator asks of a hit (rt_bsdf_device): Intersection::GetBSDF, then BSDF::f / Pdf / Sample_f / NumComponents, and Intersection::Le,
        with wo = -d of each ray (directions of unit length).  rays: the [n, 8] tensor given to intersect(); hits: the dict intersect() returned for
        it (or its [n, 4] record tensor).  wi: float32 [n, 3] world directions (needed for `f`, `pdf`); u: float32 [n, 3] = u1, u2, u3 of Sample_f
        (needed for the `s_*` fields); flags: int32 [n] BSDF_* masks, None = BSDF_ALL for all.  Returns per requested field a torch tensor on the
        scene's device: `f`, `s_wi`, `s_f`, `le` float32 [n, 3], `pdf`, `s_pdf` float32 [n], `s_type`, `n_components` int32 [n].  A miss gives zeros;
        a failed sample (s_pdf == 0) gives s_wi = s_f = 0 and s_type = 0.  Nothing of a frame is touched."""
        import torch
        fields = tuple(fields)
        for f in fields:
            if f not in _BSDF_FIELD_SHAPE:
                raise ValueError("fields: unknown field %r (known: %s)" % (f, ", ".join(BSDF_FIELDS)))
        if not fields:
            raise ValueError("fields: at least one of %s is needed" % ", ".join(BSDF_FIELDS))
        self._check_ray_tensor(torch, rays, getattr(self, "_device", None))
        n, dev = int(rays.shape[0]), rays.device
        rec = hits
        if isinstance(hits, dict):                     # intersect()'s prim / t / b1 / b2 are views of one [n, 4] record array: column 0 starts it
            rec = hits["prim"]
            if n and (rec.stride(0) != 4 or hits["t"].data_ptr() != rec.data_ptr() + 4):
                raise ValueError("hits: the dict intersect() returned is needed (prim, t, b1, b2 as views of one [n, 4] record array)")
            rec = torch.as_strided(rec.view(torch.float32), (n, 4), (4, 1)) if n else torch.empty((0, 4), dtype=torch.float32, device=dev)
        self._check_query_tensor(torch, rec, "hits", n, 4, torch.float32, rays)
        if wi is None and ("f" in fields or "pdf" in fields):
            raise ValueError("wi: needed for the fields f and pdf")
        if u is None and any(f.startswith("s_") for f in fields):
            raise ValueError("u: needed for the fields s_wi, s_f, s_pdf and s_type")
        if wi is not None:
            self._check_query_tensor(torch, wi, "wi", n, 3, torch.float32, rays)
        if u is not None:
            self._check_query_tensor(torch, u, "u", n, 3, torch.float32, rays)
        if flags is not None:
            self._check_query_tensor(torch, flags, "flags", n, 0, torch.int32, rays)
        out = {f: (torch.empty(n, dtype=torch.int32 if _BSDF_FIELD_SHAPE[f][1] else torch.float32, device=dev) if not _BSDF_FIELD_SHAPE[f][0]
                   else torch.empty((n, _BSDF_FIELD_SHAPE[f][0]), dtype=torch.float32, device=dev)) for f in fields}
        if n:
            q = RtBsdfQuery(wi=wi.data_ptr() if wi is not None else None, u=u.data_ptr() if u is not None else None,
                            flags=flags.data_ptr() if flags is not None else None, **{f: t.data_ptr() for f, t in out.items()})
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_bsdf_device(self._s, C.c_void_p(rays.data_ptr()), C.c_void_p(rec.data_ptr()), n, C.byref(q)))
            if mine is not None:
                cur.wait_stream(mine)
        return out

    def occluded(self, rays):
        """Scene::IntersectP for rays in device memory (rt_trace_any_device): a uint8 [n] torch tensor, 1 = something lies in (mint, maxt)."""
        import torch
        self._check_ray_tensor(torch, rays, getattr(self, "_device", None))
        n, dev = int(rays.shape[0]), rays.device
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_trace_any_device(self._s, C.c_void_p(rays.data_ptr()), n, C.c_void_p(occ.data_ptr())))
            if mine is not None:
                cur.wait_stream(mine)
        return occ

    def light(self, p, light, n=None, u=None, rng=None, wi=None, seed=None, fields=LIGHT_FIELDS) -> dict:
        """What EstimateDirect asks of a light (rt_light_device): Light::Sample_L, Pdf, Le and IsDeltaLight at points in device memory.
        p: float32 [m, 3] reference points; light: int32 [m] indices into the scene's lights (scene order; group queries by light for speed);
        n: float32 [m, 3] normals at p -- given, the forms EstimateDirect uses (the infinite light samples a cosine about +-n), None: the forms
        without a normal; u: float32 [m, 2] = u1, u2 (needed for the `s_*` fields); rng: uint32 (or int32 bit patterns) [m, 2] = key and first
        counter of the keyed stream the sample's RandomFloat() comes from, None = (i, 0); wi: float32 [m, 3] unit directions (needed for `pdf`, `le`);
        seed: None = the parsed frame's.  Returns per requested field a torch tensor on the device: `s_wi`, `s_L`, `le` float32 [m, 3], `s_pdf`, `pdf`
        float32 [m], `s_ray` float32 [m, 8] (the shadow ray, ready for occluded()), `s_draws`, `is_delta` int32 [m].  Nothing of a frame is touched."""
        import torch
        fields = tuple(fields)
        for f in fields:
            if f not in _LIGHT_FIELD_SHAPE:
                raise ValueError("fields: unknown field %r (known: %s)" % (f, ", ".join(LIGHT_FIELDS)))
        if not fields:
            raise ValueError("fields: at least one of %s is needed" % ", ".join(LIGHT_FIELDS))
        if not isinstance(p, torch.Tensor):
            raise ValueError("p: a torch tensor is needed, got %s" % type(p).__name__)
        if p.dim() != 2:
            raise ValueError("p: shape [m, 3] is needed, got %s" % (tuple(p.shape),))
        m = int(p.shape[0])
        self._check_query_tensor(torch, p, "p", m, 3, torch.float32, p)
        self._check_query_tensor(torch, light, "light", m, 0, torch.int32, p)
        if u is None and any(f.startswith("s_") for f in fields):
            raise ValueError("u: needed for the fields s_wi, s_L, s_pdf, s_ray and s_draws")
        if wi is None and ("pdf" in fields or "le" in fields):
            raise ValueError("wi: needed for the fields pdf and le")
        if n is not None:
            self._check_query_tensor(torch, n, "n", m, 3, torch.float32, p)
        if u is not None:
            self._check_query_tensor(torch, u, "u", m, 2, torch.float32, p)
        if wi is not None:
            self._check_query_tensor(torch, wi, "wi", m, 3, torch.float32, p)
        if rng is not None:
            if isinstance(rng, torch.Tensor) and rng.dtype == torch.int32:
                self._check_query_tensor(torch, rng, "rng", m, 2, torch.int32, p)
            else:
                self._check_query_tensor(torch, rng, "rng", m, 2, getattr(torch, "uint32", torch.int32), p)
        if not p.is_cuda:
            raise ValueError("p: a tensor in device memory is needed, got one on %s" % p.device)
        d = getattr(self, "_device", None)
        if d is not None and d >= 0 and p.device.index != d:
            raise ValueError("p: the tensor is on %s, the scene on device %d" % (p.device, d))
        if seed is None:
            seed = self.parsed.render_view()["seed"]
        dev = p.device
        out = {f: (torch.empty(m, dtype=torch.int32 if _LIGHT_FIELD_SHAPE[f][1] else torch.float32, device=dev) if not _LIGHT_FIELD_SHAPE[f][0]
                   else torch.empty((m, _LIGHT_FIELD_SHAPE[f][0]), dtype=torch.float32, device=dev)) for f in fields}
        if m:
            ptr = lambda t: t.data_ptr() if t is not None else None
            q = RtLightQuery(p=ptr(p), nrm=ptr(n), light=ptr(light), u=ptr(u), rng=ptr(rng), wi=ptr(wi), seed=int(seed) & 0xFFFFFFFF,
                             **{f: t.data_ptr() for f, t in out.items()})
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_light_device(self._s, m, C.byref(q)))
            if mine is not None:
                cur.wait_stream(mine)
        return out

    def medium(self, p=None, w=None, wp=None, rays=None, u=None, u_scatter=None, rng=None, seed=None, step_size=None, fields=MEDIUM_FIELDS) -> dict:
        """What an integrator asks of the participating medium (rt_medium_device), one query per row.  p: float32 [n, 3] points (needed for
        `sigma_a`, `sigma_s`, `sigma_t`, `lve`, `phase`); w, wp: float32 [n, 3] directions (needed for `phase`); rays: float32 [n, 8] (needed for
        `hit`, `t01`, `tau`, `tr`, `lv`, `draws`, `status`); u: float32 [n] Tau's offset (needed for `tau`; given, `tr` is the volume integrator's
        Transmittance with a sample, None: Scene::Transmittance(ray), which draws its offset); u_scatter: float32 [n] (needed for `lv`); rng: uint32
        (or int32 bit patterns) [n, 2] = key and first counter of the keyed stream, None = (i, 0); seed, step_size: None = the parsed frame's.
        Returns per requested field a torch tensor on the device: float32 [n, 3] (`t01` [n, 2], `phase` [n]), `hit`, `draws`, `status` int32 [n].
        `lv` is EmissionIntegrator::Li; a frame under VolumeIntegrator "single" is refused for it.  Nothing of a frame is touched."""
        import torch
        fields = tuple(fields)
        for f in fields:
            if f not in _MEDIUM_FIELD_SHAPE:
                raise ValueError("fields: unknown field %r (known: %s)" % (f, ", ".join(MEDIUM_FIELDS)))
        if not fields:
            raise ValueError("fields: at least one of %s is needed" % ", ".join(MEDIUM_FIELDS))
        want_point = any(f in MEDIUM_POINT_FIELDS for f in fields)
        want_ray = any(f in MEDIUM_RAY_FIELDS for f in fields)
        if want_point and p is None:
            raise ValueError("p: needed for the fields %s" % ", ".join(MEDIUM_POINT_FIELDS))
        if "phase" in fields and (w is None or wp is None):
            raise ValueError("w, wp: needed for the field phase")
        if want_ray and rays is None:
            raise ValueError("rays: needed for the fields %s" % ", ".join(MEDIUM_RAY_FIELDS))
        if "tau" in fields and u is None:
            raise ValueError("u: needed for the field tau")
        if "lv" in fields and u_scatter is None:
            raise ValueError("u_scatter: needed for the field lv")
        like = rays if rays is not None else p
        if not isinstance(like, torch.Tensor):
            raise ValueError("%s: a torch tensor is needed, got %s" % ("rays" if rays is not None else "p", type(like).__name__))
        first = "rays" if rays is not None else "p"
        if like.dim() != 2:
            raise ValueError("%s: shape [n, %d] is needed, got %s" % (first, 8 if rays is not None else 3, tuple(like.shape)))
        m = int(like.shape[0])
        for t, name, cols in ((rays, "rays", 8), (p, "p", 3), (w, "w", 3), (wp, "wp", 3), (u, "u", 0), (u_scatter, "u_scatter", 0)):
            if t is not None:
                self._check_query_tensor(torch, t, name, m, cols, torch.float32, like)
        if rng is not None:
            if isinstance(rng, torch.Tensor) and rng.dtype == torch.int32:
                self._check_query_tensor(torch, rng, "rng", m, 2, torch.int32, like)
            else:
                self._check_query_tensor(torch, rng, "rng", m, 2, getattr(torch, "uint32", torch.int32), like)
        if not like.is_cuda:
            raise ValueError("%s: a tensor in device memory is needed, got one on %s" % (first, like.device))
        d = getattr(self, "_device", None)
        if d is not None and d >= 0 and like.device.index != d:
            raise ValueError("%s: the tensor is on %s, the scene on device %d" % (first, like.device, d))
        view = self.parsed.render_view()
        if seed is None:
            seed = view["seed"]
        if step_size is None:
            step_size = view["step_size"]
        dev = like.device
        out = {f: (torch.empty(m, dtype=torch.int32 if _MEDIUM_FIELD_SHAPE[f][1] else torch.float32, device=dev) if not _MEDIUM_FIELD_SHAPE[f][0]
                   else torch.empty((m, _MEDIUM_FIELD_SHAPE[f][0]), dtype=torch.float32, device=dev)) for f in fields}
        if m:
            ptr = lambda t: t.data_ptr() if t is not None else None
            q = RtMediumQuery(p=ptr(p), w=ptr(w), wp=ptr(wp), rays=ptr(rays), u=ptr(u), u_scatter=ptr(u_scatter), rng=ptr(rng),
                              seed=int(seed) & 0xFFFFFFFF, step_size=float(step_size), volume_integrator=int(view["volume_integrator"]),
                              **{f: t.data_ptr() for f, t in out.items()})
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_medium_device(self._s, m, C.byref(q)))
            if mine is not None:
                cur.wait_stream(mine)
        return out

    def volume_samples(self, first: int, count: int) -> dict:
        """rt_volume_samples_device: what the volume integrator of camera samples first .. first + count - 1 of the parsed frame starts from, as torch
        tensors on the scene's device: `u` float32 [count] (the tau request's value), `u_scatter` float32 [count] (the scatter request's) and `rng`
        int32 [count, 2] (the bit patterns of the stream's key and of the counter at which the integrators' draws start) -- medium()'s arguments
        of those names."""
        import torch
        if first < 0 or count < 0:
            raise ValueError("volume_samples: first and count must not be negative")
        if not torch.cuda.is_available():
            raise RtError("torch sees no HIP device.  torch carries a HIP runtime of its own and the first one a process loads serves both: "
                          "import torch before this package loads libpbrt_hip.so (before the first DeviceScene), as bench.py does")
        d = getattr(self, "_device", -1)
        dev = torch.device("cuda", d if d is not None and d >= 0 else torch.cuda.current_device())
        words = torch.empty((int(count), 4), dtype=torch.int32, device=dev)
        if count:
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_volume_samples_device(self._s, self.parsed.render_desc, int(first), int(count), C.c_void_p(words.data_ptr())))
            if mine is not None:
                cur.wait_stream(mine)
        return {"u": words[:, 0].view(torch.float32).contiguous(), "u_scatter": words[:, 1].view(torch.float32).contiguous(), "rng": words[:, 2:4].contiguous()}

    def radiance(self, rays, first: int = 0):
        """Scene::Li for rays in device memory (rt_radiance_device): a float32 [n, 4] torch tensor (L.r, L.g, L.b, alpha) on the scene's device.
        rays: contiguous float32 [n, 8] torch tensor on that device, directions of unit length.  Ray i is evaluated with the sample set of camera
        sample first + i of the parsed frame (its RNG stream, sampler values, integrator): for the frame's own rays (camera_rays_device(first, n))
        the result is samples()[first:first + n, :4] of a render() bit for bit.  Neither the film nor the sample buffer is touched."""
        import torch
        self._check_ray_tensor(torch, rays, getattr(self, "_device", None))
        if first < 0:
            raise ValueError("radiance: first must not be negative")
        n, dev = int(rays.shape[0]), rays.device
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        if n:
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_radiance_device(self._s, self.parsed.render_desc, C.c_void_p(rays.data_ptr()), int(first), n, C.c_void_p(out.data_ptr())))
            if mine is not None:
                cur.wait_stream(mine)
        return out

    def camera_rays_device(self, first: int, count: int):
        """rt_camera_rays_device: the rays of camera samples first .. first + count - 1 of the parsed frame as a float32 [count, 8] torch tensor on
        the scene's device (bit for bit camera_rays(first, count))."""
        import torch
        if first < 0 or count < 0:
            raise ValueError("camera_rays_device: first and count must not be negative")
        if not torch.cuda.is_available():
            raise RtError("torch sees no HIP device.  torch carries a HIP runtime of its own and the first one a process loads serves both: "
                          "import torch before this package loads libpbrt_hip.so (before the first DeviceScene), as bench.py does")
        d = getattr(self, "_device", -1)
        dev = torch.device("cuda", d if d is not None and d >= 0 else torch.cuda.current_device())
        rays = torch.empty((int(count), 8), dtype=torch.float32, device=dev)
        if count:
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_camera_rays_device(self._s, self.parsed.render_desc, int(first), int(count), C.c_void_p(rays.data_ptr())))
            if mine is not None:
                cur.wait_stream(mine)
        return rays

    def sample_positions_device(self, first: int, count: int):
        """rt_sample_positions_device: Sample::imageX, imageY of camera samples first .. first + count - 1 of the parsed frame as a float32
        [count, 2] torch tensor on the scene's device (bit for bit samples()[first:first + count, 4:6] of a render())."""
        import torch
        if first < 0 or count < 0:
            raise ValueError("sample_positions_device: first and count must not be negative")
        if not torch.cuda.is_available():
            raise RtError("torch sees no HIP device.  torch carries a HIP runtime of its own and the first one a process loads serves both: "
                          "import torch before this package loads libpbrt_hip.so (before the first DeviceScene), as bench.py does")
        d = getattr(self, "_device", -1)
        dev = torch.device("cuda", d if d is not None and d >= 0 else torch.cuda.current_device())
        xy = torch.empty((int(count), 2), dtype=torch.float32, device=dev)
        if count:
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_sample_positions_device(self._s, self.parsed.render_desc, int(first), int(count), C.c_void_p(xy.data_ptr())))
            if mine is not None:
                cur.wait_stream(mine)
        return xy

    def add_samples(self, L, first: int = 0):
        """Film::AddSample for radiances in device memory (rt_film_add_device).  L: contiguous float32 [n, 4] torch tensor (L.r, L.g, L.b, alpha:
        what radiance() returns) on the scene's device; row i is added to the bound film as camera sample first + i of the parsed frame, on top
        of what the film holds.  clear_film(); add_samples(radiance(camera_rays_device(0, N))) is the film of render() bit for bit, and so is the
        same in contiguous chunks added in ascending order."""
        import torch
        if not isinstance(L, torch.Tensor):
            raise ValueError("L: a torch tensor is needed, got %s" % type(L).__name__)
        if L.dtype != torch.float32:
            raise ValueError("L: dtype float32 is needed, got %s" % L.dtype)
        if L.dim() != 2 or L.shape[1] != 4:
            raise ValueError("L: shape [n, 4] (L.r, L.g, L.b, alpha) is needed, got %s" % (tuple(L.shape),))
        if not L.is_contiguous():
            raise ValueError("L: a contiguous tensor is needed")
        if not L.is_cuda:
            raise ValueError("L: a tensor in device memory is needed, got one on %s" % L.device)
        device = getattr(self, "_device", None)
        if device is not None and device >= 0 and L.device.index != device:
            raise ValueError("L: the tensor is on %s, the scene on device %d" % (L.device, device))
        if first < 0:
            raise ValueError("add_samples: first must not be negative")
        n, dev = int(L.shape[0]), L.device
        if n:
            cur, mine = self._scene_stream(torch, dev)
            if mine is not None:
                mine.wait_stream(cur)
            _chk(hip_lib().rt_film_add_device(self._s, self.parsed.render_desc, C.c_void_p(L.data_ptr()), int(first), n))
            if mine is not None:
                cur.wait_stream(mine)

    def close(self):
        if self._s:
            hip_lib().rt_scene_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_text(scene_text: str, device: int = -1):
    """Convenience: parse -> create -> render -> (rgb, alpha, counters)."""
    ps = ParsedScene(text=scene_text)
    ds = DeviceScene(ps, device)
    ds.render()
    rgb, alpha = ds.film()
    cnt = ds.counters()
    ms = ds.last_ms()[0]
    ds.close()
    return rgb, alpha, cnt, ms
