"""Builds and binds tests/hostcheck/filterx_check.cpp (the expanded sphere filter of the product headers
compiled for the CPU).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

from blenderraytracer_amd import capi
import hostcheck_binding

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "filterx_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "include", "rt_hip.h")] + [
    os.path.join(ROOT, "blenderraytracer_amd", "csrc", f) for f in ("pt_core.h", "pt_path.h", "scene_pack.h", "js_math.h")]
LIB = os.path.join(HERE, "hostcheck", "_build", "libfilterx_check.so")
_lib = None


def build():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = "%s.tmp%d" % (LIB, os.getpid())        # parallel test workers: build aside, rename atomically
    subprocess.check_call([hipcc, "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-DRT_HOST_COUNTERS=1", "-I", os.path.join(ROOT, "include"), SRC, "-o", tmp])
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.fxc_filter_check.argtypes = [C.c_longlong, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.fxc_work.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), C.c_int, C.POINTER(C.c_double)]
        _lib = L
    return _lib


def filter_check(n, seed, mode, mutation=0):
    """dict of the new filter's violations, the old one's, the worst |X' - Y - margin| / Q, the fractions of sure
    misses the new / old filter rejects, and their number (fxc_filter_check)"""
    out = (C.c_double * 6)()
    assert lib().fxc_filter_check(n, seed, mode, mutation, out) == 0
    return {"violations": int(out[0]), "violations_old": int(out[1]), "worst": out[2], "rejected": out[3],
            "rejected_old": out[4], "misses": int(out[5])}



def work(packed, settings_list, lean):
    """Totals over the crops of the grid walk on the CPU (fxc_work): lean=True the binary64 lean grid kernel's walk
    as the device runs it (the LDS copy in the expanded filter's form), lean=False the walk of
    hostcheck_binding.event_counts.  dict of segments, cells, sphere_records, draws, sum (r, g, b) and the events of
    hostcheck_binding.EVENTS, counted as event_counts counts them (with the scene set-up's probe rays, once per
    crop); "setup": those rays' share of each event."""
    tot = [0.0] * 39
    for st in settings_list:
        out = (C.c_double * 39)()
        assert lib().fxc_work(C.byref(packed.desc), C.byref(st), int(lean), out) == 0
        tot = [a + b for a, b in zip(tot, out)]
    res = {"segments": tot[0], "cells": tot[1], "sphere_records": tot[2], "draws": tot[3], "sum": tuple(tot[4:7])}
    res.update({n: tot[7 + k] for k, n in enumerate(hostcheck_binding.EVENTS)})
    res["setup"] = {n: tot[23 + k] for k, n in enumerate(hostcheck_binding.EVENTS)}
    return res
