"""Builds and binds tests/hostcheck/nee_check.cpp (the product's emitter-sampling code compiled for the CPU), once
per RT_NEE_MUTATION (0: the product; 1, 2: the two deliberate errors the statistical test must catch), and holds
what the CPU and GPU emitter tests share: scenes, query sets, renders and the block statistics.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "nee_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "include", "rt_hip.h")] + [
    os.path.join(ROOT, "blenderraytracer_amd", "csrc", f)
    for f in ("pt_core.h", "pt_path.h", "scene_pack.h", "js_math.h", "kernel_select.h")]
_libs = {}


def build(mutation=0):
    lib = os.path.join(HERE, "hostcheck", "_build", "libnee_check%s.so" % ("" if not mutation else "_m%d" % mutation))
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    if os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in DEPS):
        return lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = "%s.tmp%d" % (lib, os.getpid())        # parallel test workers: build aside, rename atomically
    subprocess.check_call([hipcc, "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-DRT_NEE_MUTATION=%d" % mutation, "-I", os.path.join(ROOT, "include"), SRC, "-o", tmp])
    os.replace(tmp, lib)
    return lib


def lib(mutation=0):
    if mutation not in _libs:
        L = C.CDLL(build(mutation))
        dp, bp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        sd = C.POINTER(capi.SceneDesc)
        L.ptn_emitters.argtypes = [sd, ip, ip, dp, C.c_int]
        L.ptn_emitter_limit.argtypes = [C.c_longlong]
        L.ptn_samples.argtypes = [sd, C.c_int, dp, up, C.c_longlong, ip, dp, dp, dp, bp, dp]
        L.ptn_render.argtypes = [sd, C.POINTER(capi.Settings), C.c_int, dp, up, up]
        L.ptn_select.argtypes = [sd, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.ptn_shadow_queries.argtypes = [sd, C.POINTER(capi.Settings), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        _libs[mutation] = L
    return _libs[mutation]


# ---- scenes ------------------------------------------------------------------------------------------
SCENES = ("cornell", "nee_mixed")


def tracer(scene, width=32, height=32, seed=1, samples=16, max_bounces=5, **kw):
    """GpuRayTracer of a scene file (or None: the default scene) with the tests' settings; no device is touched
    until it renders."""
    rt = GpuRayTracer(width, height, seed=seed, **kw)
    if scene is not None:
        assert rt.load_from_json(load_scene_json(scene))
        rt.resize_canvas(width, height)
    rt.update_render_settings({"samples": samples, "maxBounces": max_bounces})
    return rt


def emitters(packed, records=False):
    """[(kind, idx)] of the scene's emitter list (kind 0 sphere, 1 triangle), and with records the n x 16 array
    g[12], le[3], area."""
    cap = 1 << 12
    kind, idx = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    rec = np.zeros((cap, 16))
    ip = C.POINTER(C.c_int32)
    n = lib().ptn_emitters(C.byref(packed.desc), kind.ctypes.data_as(ip), idx.ctypes.data_as(ip),
                           rec.ctypes.data_as(C.POINTER(C.c_double)), cap)
    assert 0 <= n <= cap
    lst = list(zip(kind[:n].tolist(), idx[:n].tolist()))
    return (lst, rec[:n].copy()) if records else lst


def host_samples(packed, accel, points, keys):
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 6)
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n = len(points)
    res = {"emitter": np.zeros(n, dtype=np.int32), "omega": np.zeros((n, 3)), "p_l": np.zeros(n), "t_e": np.zeros(n),
           "visible": np.zeros(n, dtype=np.uint8), "pO_hit": np.zeros(n)}
    dp = C.POINTER(C.c_double)
    rc = lib().ptn_samples(C.byref(packed.desc), accel, points.ctypes.data_as(dp), keys.ctypes.data_as(C.POINTER(C.c_uint32)),
                           n, res["emitter"].ctypes.data_as(C.POINTER(C.c_int32)), res["omega"].ctypes.data_as(dp),
                           res["p_l"].ctypes.data_as(dp), res["t_e"].ctypes.data_as(dp),
                           res["visible"].ctypes.data_as(C.POINTER(C.c_uint8)), res["pO_hit"].ctypes.data_as(dp))
    assert rc == 0
    res["visible"] = res["visible"].astype(bool)
    return res


def host_render(packed, settings, on, mutation=0):
    """Sample-order CPU render of the product's trace_pixel, emitter sampling on or off."""
    cw = settings.crop_w or settings.width
    ch = settings.crop_h or settings.height
    s = np.zeros((ch, cw, 3))
    segs = np.zeros((ch, cw), dtype=np.uint32)
    draws = np.zeros((ch, cw), dtype=np.uint32)
    up = C.POINTER(C.c_uint32)
    rc = lib(mutation).ptn_render(C.byref(packed.desc), C.byref(settings), int(on), s.ctypes.data_as(C.POINTER(C.c_double)),
                                  segs.ctypes.data_as(up), draws.ctypes.data_as(up))
    assert rc == 0
    return {"mean": s / settings.samples, "segments": segs, "draws": draws}


def select(packed, on, bvh, pool=True):
    """(mode, walk report) select_kernel gives the scene with emitter sampling on or off"""
    walk = C.c_int()
    acc = lib().ptn_select(C.byref(packed.desc), int(on), int(bvh), int(pool), C.byref(walk))
    assert acc >= 0
    return acc, walk.value


def shadow_queries(packed, settings):
    cast, blocked = C.c_ulonglong(), C.c_ulonglong()
    assert lib().ptn_shadow_queries(C.byref(packed.desc), C.byref(settings), C.byref(cast), C.byref(blocked)) == 0
    return cast.value, blocked.value


def bits(a):
    """float64 array -> its bit patterns (NaNs compare by payload, -0 != +0)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the query set of the bit-identity tests: n hit points with facing normals, and keys --------------------
def query_set(scene, n=10000, seed=7):
    """n queries (x, normal) spread over the scene's box, some of them on or inside emitters, with random unit
    normals, and n keys.  Deterministic."""
    rng = np.random.RandomState(seed + (0 if scene == "cornell" else 1))
    lo, hi = (np.array([-2.4, -2.4, -4.9]), np.array([2.4, 2.4, 2.0])) if scene == "cornell" else \
             (np.array([-3.0, -1.0, -5.9]), np.array([3.0, 2.3, 2.0]))
    x = lo + rng.rand(n, 3) * (hi - lo)
    nrm = rng.randn(n, 3)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    keys = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([x, nrm], axis=1)), keys


# ---- the statistics of "same expectation" (tests 4 / GPU 3) -------------------------------------------------
def block_means(mean, block=4):
    """(h, w, 3) -> (h / block, w / block, 3) block means"""
    h, w, c = mean.shape
    return mean.reshape(h // block, block, w // block, block, c).mean(axis=(1, 3))


def welch(a, b):
    """a, b: (seeds, blocks_y, blocks_x, 3) block means of the two sides.  Returns (t per block-channel, number of
    blocks).  A block-channel both sides render without any variance and with the same value has t = 0."""
    na, nb = a.shape[0], b.shape[0]
    d = a.mean(axis=0) - b.mean(axis=0)
    se = np.sqrt(a.var(axis=0, ddof=1) / na + b.var(axis=0, ddof=1) / nb)
    t = np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d == 0, 0.0, np.inf * np.sign(d)))
    return t, a.shape[1] * a.shape[2]


def expectation_conditions(t, blocks):
    """The three conditions of the same-expectation tests as (max |t|, share of |t| > 3, |mean t|, its bound)"""
    at = np.abs(t)
    return at.max(), float((at > 3).mean()), abs(float(t.mean())), 4.0 / np.sqrt(blocks)


def conditions_hold(t, blocks):
    mx, share, mt, bound = expectation_conditions(t, blocks)
    return mx < 6 and share <= 0.02 and mt <= bound
