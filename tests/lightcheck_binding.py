"""Builds and binds tests/hostcheck/light_check.cpp (the product's direct-lighting code compiled for the CPU) and
loads the reference's lighting fixtures (tests/golden/lights/, made by tests/js/lights_reference.mjs).
TEST INFRASTRUCTURE ONLY."""
import base64
import copy
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np

from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "light_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "include", "rt_hip.h")] + [
    os.path.join(ROOT, "blenderraytracer_amd", "csrc", f) for f in ("pt_core.h", "pt_path.h", "scene_pack.h", "js_math.h")]
LIB = os.path.join(HERE, "hostcheck", "_build", "liblight_check.so")
GOLDEN = os.path.join(HERE, "golden", "lights")
CASES = ("lit_sample_scene", "lit_kitchen_sink", "lit_rtow_crop", "lit_cornell_crop", "lit_tex_mesh_crop")
_lib = None
_manifest = None
_kats = None


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
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.ptl_validate.argtypes = [C.POINTER(capi.SceneDesc), C.c_char_p, C.c_int]
        L.ptl_num_lights.argtypes = [C.POINTER(capi.SceneDesc)]
        L.ptl_illuminate.argtypes = [C.POINTER(capi.LightDesc), dp, C.c_longlong, dp]
        L.ptl_occluded.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, dp, dp, C.c_longlong, bp, bp]
        L.ptl_render.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), dp, C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32)]
        L.ptl_shadow_rays.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), C.POINTER(C.c_ulonglong),
                                      C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


# ---- fixtures ----------------------------------------------------------------------------------------
def dec(v):
    """the generator's encoding of non-finite numbers and of -0 back to floats"""
    if isinstance(v, str) and v in ("NaN", "Infinity", "-Infinity", "-0"):
        return float(v.replace("Infinity", "inf"))
    if isinstance(v, list):
        return [dec(x) for x in v]
    if isinstance(v, dict):
        return {k: dec(x) for k, x in v.items()}
    return v


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(GOLDEN, "manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def kats():
    global _kats
    if _kats is None:
        with gzip.open(os.path.join(GOLDEN, "kats.json.gz")) as f:
            _kats = json.load(f)
    return _kats


def load_array(case, key):
    c = manifest()["cases"][case]
    dt = {"linear": np.float64, "post": np.float64, "rgba8": np.uint8, "segs": np.uint32, "draws": np.uint32}[key]
    raw = gzip.open(os.path.join(GOLDEN, c["files"][key])).read()
    _, _, cw, ch = c["crop"]
    comp = {"linear": 3, "post": 3, "rgba8": 4, "segs": 1, "draws": 1}[key]
    a = np.frombuffer(raw, dtype=dt).reshape(ch, cw, comp)
    return a[..., 0] if comp == 1 else a


def case_json(case):
    """The scene JSON of a case as the generator gave it to the reference's loader: the scene file with `lights`
    replaced by the case's (None: the file's own)."""
    c = manifest()["cases"][case]
    data = copy.deepcopy(load_scene_json(c["scene"]))
    if c["lights_in"] is not None:
        data["lights"] = copy.deepcopy(c["lights_in"])
    return data


def tracer_for(case, direct_lighting=True, **kw):
    """GpuRayTracer configured as the generator configured the reference RayTracer."""
    c = manifest()["cases"][case]
    w, h = c["requested"]
    rt = GpuRayTracer(w, h, seed=c["seed"], direct_lighting=direct_lighting, **kw)
    assert rt.load_from_json(case_json(case))
    rt.update_render_settings(c["settings_in"])
    assert (rt.width, rt.height) == (c["width"], c["height"])
    return rt, c


def crop_of(c):
    x0, y0, cw, ch = c["crop"]
    return None if (x0, y0, cw, ch) == (0, 0, c["width"], c["height"]) else (x0, y0, cw, ch)


def occlusion_queries(case):
    """(rays n x 6, tmax n, verdict n) of a case's occlusion KATs: the render's own shadow rays, then the random
    rays with their limit at the closest hit's t (False), the next double above (True) and below (False); rays
    that hit nothing carry t = inf and are never occluded."""
    with gzip.open(os.path.join(GOLDEN, manifest()["cases"][case]["files"]["occlusion"])) as f:
        k = json.load(f)
    f64 = lambda s: np.frombuffer(base64.b64decode(s), dtype=np.float64)
    u8 = lambda s: np.frombuffer(base64.b64decode(s), dtype=np.uint8)
    r = f64(k["render"]["rays_f64"]).reshape(-1, 7)
    rays, tmax, verdict = [r[:, :6]], [r[:, 6]], [u8(k["render"]["verdict_u8"])]
    q = f64(k["random"]["rays_f64"]).reshape(-1, 7)
    v = u8(k["random"]["verdict_u8"]).reshape(-1, 3)
    t = q[:, 6]
    for j, lim in enumerate((t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf))):
        rays.append(q[:, :6])
        tmax.append(lim)
        verdict.append(v[:, j])
    return (np.ascontiguousarray(np.concatenate(rays)), np.ascontiguousarray(np.concatenate(tmax)),
            np.concatenate(verdict).astype(bool))


def light_records(packed):
    """The packed light records as a list of dicts (the generator's light_records layout)."""
    return [{"type": l.type, "v": list(l.v), "color": list(l.color), "intensity": l.intensity}
            for l in (packed.lights[i] for i in range(packed.num_lights))] if packed.num_lights else []


def host_occluded(desc, accel, rays, tmax):
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    tmax = np.ascontiguousarray(tmax, dtype=np.float64)
    out = np.zeros(len(rays), dtype=np.uint8)
    byc = np.zeros(len(rays), dtype=np.uint8)
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    assert lib().ptl_occluded(C.byref(desc), accel, rays.ctypes.data_as(dp), tmax.ctypes.data_as(dp), len(rays),
                              out.ctypes.data_as(bp), byc.ctypes.data_as(bp)) == 0
    return out.astype(bool), byc.astype(bool)


def host_render(packed, settings):
    """Sample-order CPU render of the product's trace_pixel (lit modes when the descriptor carries lights)."""
    cw = settings.crop_w or settings.width
    ch = settings.crop_h or settings.height
    s = np.zeros((ch, cw, 3))
    segs = np.zeros((ch, cw), dtype=np.uint32)
    draws = np.zeros((ch, cw), dtype=np.uint32)
    rc = lib().ptl_render(C.byref(packed.desc), C.byref(settings), s.ctypes.data_as(C.POINTER(C.c_double)),
                          segs.ctypes.data_as(C.POINTER(C.c_uint32)), draws.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0
    return {"mean": s / settings.samples, "segments": segs, "draws": draws}


def shadow_rays(packed, settings):
    """(shadow rays cast, of them occluded) by the lit render of the settings' crop (sample order, CPU)"""
    cast, blocked = C.c_ulonglong(), C.c_ulonglong()
    assert lib().ptl_shadow_rays(C.byref(packed.desc), C.byref(settings), C.byref(cast), C.byref(blocked)) == 0
    return cast.value, blocked.value


def bits(a):
    """float64 array -> its bit patterns (NaNs compare by payload, -0 != +0)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
