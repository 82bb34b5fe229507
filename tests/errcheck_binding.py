"""Builds and binds tests/hostcheck/error_check.cpp: the error estimate's per-pixel bodies (csrc/pt_error.h) compiled
for the CPU and driven in the kernels' order.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "error_check.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "blenderraytracer_amd", "csrc", f)
                for f in ("pt_core.h", "pt_path.h", "pool_order.h", "pt_error.h")]
LIB = os.path.join(HERE, "hostcheck", "_build", "liberror_check.so")
_lib = None


class ErrorWords(C.Structure):
    """pt_error.h ErrorWords"""
    _fields_ = [("frame_error", C.c_double), ("max_error", C.c_double), ("nonfinite", C.c_longlong),
                ("pixels", C.c_longlong), ("samples", C.c_int32), ("groups", C.c_int32), ("pad", C.c_int32 * 2)]


def build():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = "%s.tmp%d" % (LIB, os.getpid())        # parallel test workers: build aside, rename atomically
    subprocess.check_call([hipcc, "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I", os.path.join(ROOT, "include"), SRC, "-o", tmp])
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        L.pte_moments.argtypes = [C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, C.c_int]
        L.pte_estimate.argtypes = [C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, dp, fp, C.c_double, C.c_int,
                                   C.POINTER(ErrorWords)]
        assert L.pte_words_size() == C.sizeof(ErrorWords)
        _lib = L
    return _lib


def partials_layout(groups_hwc):
    """Group sums (chunks, h, w, 3) -> the pool's partials part[c][tile][ch][m] (chunks, tiles, 3, 64), zero where a
    tile has no pixel."""
    g = np.asarray(groups_hwc, dtype=np.float64)
    chunks, h, w, _ = g.shape
    tx, ty = (w + 7) // 8, (h + 7) // 8
    part = np.zeros((chunks, tx * ty, 3, 64))
    for t in range(tx * ty):
        x0, y0 = (t % tx) * 8, (t // tx) * 8
        vw, vh = min(8, w - x0), min(8, h - y0)
        for m in range(vw * vh):
            part[:, t, :, m] = g[:, y0 + m // vw, x0 + m % vw, :]
    return part


def host_moments(q, groups_hwc, chunk, ns):
    """error_moments_kernel on the CPU: q (h, w, 3) += the moments of one batch's group sums (chunks, h, w, 3), chunks
    of `chunk` samples over `ns` samples.  Returns the new q."""
    q = np.ascontiguousarray(q, dtype=np.float64).copy()
    h, w, _ = q.shape
    part = np.ascontiguousarray(partials_layout(groups_hwc))
    dp = C.POINTER(C.c_double)
    assert lib().pte_moments(w, h, q.ctypes.data_as(dp), part.ctypes.data_as(dp), part.shape[0], int(chunk), int(ns)) == 0
    return q


def host_estimate(sums, q, groups, samples, threshold=0.0, min_samples=0):
    """error_tile_kernel + error_frame_kernel on the CPU: (var_mean (h, w, 3), rel_error (h, w) float32, figures dict,
    converged)."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    h, w, _ = sums.shape
    var = np.zeros((h, w, 3))
    rel = np.zeros((h, w), dtype=np.float32)
    words = ErrorWords()
    dp = C.POINTER(C.c_double)
    rc = lib().pte_estimate(w, h, sums.ctypes.data_as(dp), q.ctypes.data_as(dp), int(groups), int(samples),
                            var.ctypes.data_as(dp), rel.ctypes.data_as(C.POINTER(C.c_float)), float(threshold),
                            int(min_samples), C.byref(words))
    assert rc >= 0
    fig = {"frame_error": words.frame_error, "max_error": words.max_error, "nonfinite_pixels": words.nonfinite,
           "pixels": words.pixels, "samples": words.samples, "groups": words.groups}
    return var, rel, fig, bool(rc)
