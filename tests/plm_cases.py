"""Arguments for the portable libm functions (pbrt-v1_amd/csrc/hip/rt_libm_portable.h), shared by tests/test_plm_host.py (accuracy against float64)
and tests/test_gpu_plm.py (device against host, bit for bit), and the ctypes binding of oracle/_build/libplm.so.
Per function 2^20 seeded arguments over the domain the renderer uses and beyond, then the edge list (for the two-argument functions its square)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("sinf", "cosf", "sincosf", "acosf", "atan2f", "powf", "expf")        # plm_eval's function numbers
TWO_ARGS = ("atan2f", "powf")
N_RANDOM = 1 << 20

F32_MAX = float(np.finfo(np.float32).max)
EDGES = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 1.5, -1.5, 0.25, 1e-3, 0.99999994, 1.0000001, -0.99999994,
                  np.pi, -np.pi, np.pi / 2, -np.pi / 2, np.pi / 4, 3 * np.pi / 4, 2 * np.pi, 100 * np.pi, 1e5, -1e5, 1e6, 1e9, 1.0995116e12, 1e20, -1e20,
                  88.0, 88.72283, 88.72284, 89.0, -87.0, -87.33655, -103.0, -103.97, -104.0, -150.0, 16777216.0, 16777217.0, -16777216.0, 1e-20,
                  1.1754944e-38, -1.1754944e-38, 1e-40, -1e-40, 1.4e-45, -1.4e-45, F32_MAX, -F32_MAX, np.inf, -np.inf, np.nan], np.float32)


def _log_uniform(rng, n, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def arguments(n=N_RANDOM, seed=20240911):
    """{function: (a, b)} float32 arrays of n seeded arguments followed by the edges; b is the second argument (atan2f(a, b), powf(a, b)), else zeros."""
    rng = np.random.default_rng(seed)
    q = n // 4
    sign = lambda k: rng.choice([-1.0, 1.0], k)
    angle = np.concatenate([rng.uniform(-1e5, 1e5, n - 2 * q), rng.uniform(-7.0, 7.0, q), sign(q) * _log_uniform(rng, q, 1e-30, 1e5)])
    unit = np.concatenate([rng.uniform(-1.0, 1.0, n - 2 * q), sign(q) * (1.0 - _log_uniform(rng, q, 1e-8, 1.0)), sign(q) * _log_uniform(rng, q, 1e-30, 1.0)])
    scale = _log_uniform(rng, n, 1e-20, 1e20)
    ys, xs = rng.normal(0, 1, n) * scale, rng.normal(0, 1, n) * np.where(rng.random(n) < 0.5, scale, _log_uniform(rng, n, 1e-20, 1e20))
    # Blinn: powf(cos, exponent) and powf(u, 1 / (exponent + 1)); the phase function: powf(1 + g^2 - 2 g cos, 1.5); and a general quarter
    base = np.concatenate([rng.uniform(0.0, 1.0, n - 3 * q), rng.uniform(0.0, 1.0, q), rng.uniform(0.0, 4.0, q), _log_uniform(rng, q, 1e-10, 1e10)])
    expo = np.concatenate([_log_uniform(rng, n - 3 * q, 1e-3, 1e4), 1.0 / (1.0 + _log_uniform(rng, q, 1e-3, 1e4)), np.full(q, 1.5), rng.uniform(-10.0, 10.0, q)])
    ex = np.concatenate([rng.uniform(-104.0, 89.0, n - q), rng.uniform(-1.0, 1.0, q)])
    e2a, e2b = (m.ravel() for m in np.meshgrid(EDGES, EDGES, indexing="ij"))
    one = lambda v: (np.concatenate([v.astype(np.float32), e2a]), np.zeros(len(v) + len(e2a), np.float32))      # (the same length for every function)
    two = lambda a, b: (np.concatenate([a.astype(np.float32), e2a]), np.concatenate([b.astype(np.float32), e2b]))
    return {"sinf": one(angle), "cosf": one(angle), "sincosf": one(angle), "acosf": one(unit), "atan2f": two(ys, xs), "powf": two(base, expo), "expf": one(ex)}


def float64_reference(fn, a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(all="ignore"):
        return {"sinf": lambda: np.sin(a), "cosf": lambda: np.cos(a), "acosf": lambda: np.arccos(a), "atan2f": lambda: np.arctan2(a, b),
                "powf": lambda: np.power(a, b), "expf": lambda: np.exp(a)}[fn]()


_lib = None


def host_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(os.path.join(ROOT, "oracle", "_build", "libplm.so"))
        _lib.plm_eval.restype = C.c_int
        _lib.plm_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    return _lib


def host_eval(fn, a, b):
    """(out, out2) of libplm.so's plm_eval: out2 is sincosf's cosine, zeros otherwise"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    out, out2 = np.zeros_like(a), np.zeros_like(a)
    assert host_lib().plm_eval(FUNCS.index(fn), a.ctypes.data, b.ctypes.data, out.ctypes.data, out2.ctypes.data, a.size) == 0
    return out, out2
