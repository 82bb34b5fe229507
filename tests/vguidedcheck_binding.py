"""Builds and binds tests/hostcheck/vguided_check.cpp: the variance-guided filter's body of the product header
(pt_vguided.h vguided_pixel) compiled for the CPU.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from blenderraytracer_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "vguided_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "include", "rt_hip.h")] + [
    os.path.join(ROOT, "blenderraytracer_amd", "csrc", f)
    for f in ("pt_core.h", "pt_path.h", "pt_guided.h", "pt_vguided.h", "js_math.h")]
LIB = os.path.join(HERE, "hostcheck", "_build", "libvguided_check.so")
_lib = None


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
        L.ptv_sigma_ok.argtypes = [C.c_double]
        L.ptv_filter.argtypes = [C.c_int, C.c_int, C.POINTER(capi.GuidedParams), C.c_double, dp, dp, fp, dp, dp]
        _lib = L
    return _lib


def params(levels, sigmas):
    """rt_guided_params; sigmas = (color, albedo, normal, depth)"""
    return capi.GuidedParams(int(levels), 0, *(float(s) for s in sigmas))


def host_filter(color, var, guides, levels, sigmas, sigma_variance):
    """The CPU build of rt_guided_filter_variance_device: color, var (h, w, 3) float64, guides (h, w, 8) float32
    -> (c', v') of the last level."""
    color = np.ascontiguousarray(color, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.float64)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    h, w = color.shape[:2]
    assert var.shape == (h, w, 3) and guides.shape == (h, w, 8)
    out, vout = np.empty_like(color), np.empty_like(color)
    p = params(levels, sigmas)
    dp = C.POINTER(C.c_double)
    rc = lib().ptv_filter(w, h, C.byref(p), float(sigma_variance), color.ctypes.data_as(dp), var.ctypes.data_as(dp),
                          guides.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(dp), vout.ctypes.data_as(dp))
    assert rc == 0
    return out, vout
