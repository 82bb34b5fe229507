"""Builds and binds tests/hostcheck/tex_check.cpp (the product's texture code compiled for the CPU) and loads
the reference's texture fixtures (tests/golden/textures/, made by tests/js/texture_reference.mjs).
TEST INFRASTRUCTURE ONLY."""
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
SRC = os.path.join(HERE, "hostcheck", "tex_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "include", "rt_hip.h")] + [
    os.path.join(ROOT, "blenderraytracer_amd", "csrc", f) for f in ("pt_core.h", "pt_path.h", "scene_pack.h", "js_math.h")]
LIB = os.path.join(HERE, "hostcheck", "_build", "libtex_check.so")
GOLDEN = os.path.join(HERE, "golden", "textures")
CASES = ("tex_checker_spheres", "tex_kitchen_sink", "tex_mesh_wood_crop")
TEX_CODE = {"checker": capi.RT_TEX_CHECKER, "noise": capi.RT_TEX_NOISE, "marble": capi.RT_TEX_MARBLE,
            "wood": capi.RT_TEX_WOOD}
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
        dp = C.POINTER(C.c_double)
        L.ptx_validate.argtypes = [C.POINTER(capi.SceneDesc), C.c_char_p, C.c_int]
        L.ptx_texture_values.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, C.c_int, dp, C.c_longlong, dp]
        L.ptx_scatter.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, dp, dp, dp, C.c_int, C.c_uint, C.c_uint, C.c_uint,
                                  C.POINTER(C.c_int), dp, C.POINTER(C.c_uint)]
        L.ptx_render.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), dp, C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32)]
        _lib = L
    return _lib


# ---- fixtures ----------------------------------------------------------------------------------------
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


def tracer_for(case, **kw):
    """GpuRayTracer configured as the generator configured the reference RayTracer."""
    c = manifest()["cases"][case]
    w, h = c["requested"]
    rt = GpuRayTracer(w, h, seed=c["seed"], **kw)
    assert rt.load_from_json(load_scene_json(c["scene"]))
    rt.update_render_settings(c["settings_in"])
    assert (rt.width, rt.height) == (c["width"], c["height"])
    return rt, c


def crop_of(c):
    x0, y0, cw, ch = c["crop"]
    return None if (x0, y0, cw, ch) == (0, 0, c["width"], c["height"]) else (x0, y0, cw, ch)


# ---- a descriptor that holds the KAT textures --------------------------------------------------------
class KatScene:
    """rt_scene_desc with one Lambertian and one Metal (roughness 0.35) material per KAT texture, in that
    order (material 2 i / 2 i + 1 <-> texture i), then the extra materials given as (type, albedo, roughness,
    texture): enough for rt_texture_values / ptx_texture_values / ptx_scatter; one sphere gives it an object."""

    def __init__(self, extra=()):
        k = kats()
        texs = k["textures"]
        mats = []
        for i in range(len(texs)):
            mats += [(capi.RT_MAT_LAMBERTIAN, (0, 0, 0), 0.0, i), (capi.RT_MAT_METAL, (0, 0, 0), 0.35, i)]
        mats += list(extra)
        self.materials = (capi.MaterialDesc * len(mats))()
        for d, (t, alb, rough, _) in zip(self.materials, mats):
            d.type, d.roughness = t, rough
            d.albedo[:] = alb
        self.material_texture = np.array([m[3] for m in mats], dtype=np.int32)
        self.textures = (capi.TextureDesc * len(texs))()
        perms = []
        for d, t in zip(self.textures, texs):
            d.type, d.scale = TEX_CODE[t["type"]], t["scale"]
            d.perm = -1
            if t["perm"] is not None:
                d.perm = len(perms)
                perms.append(t["perm"])
            else:
                d.odd[:], d.even[:] = t["odd"], t["even"]
        self.texture_perms = np.array(perms, dtype=np.int32)
        self.objects = (capi.ObjectDesc * 1)()
        self.objects[0].type = capi.RT_OBJ_SPHERE
        self.objects[0].g[:] = (0, 0, -1, 0.5, 0, 0)
        self.triangles = np.zeros((1, 12))
        d = self.desc = capi.SceneDesc()
        d.abi_version = capi.RT_ABI_VERSION
        d.extensions = capi.RT_DESC_TEXTURES
        d.num_objects, d.objects = 1, self.objects
        d.num_materials, d.materials = len(mats), self.materials
        d.triangles = self.triangles.ctypes.data_as(C.POINTER(C.c_double))
        cam = GpuRayTracer(8, 8).camera
        d.camera = cam.desc()
        d.sky_intensity = 1.0
        d.perm[:] = list(range(256)) * 2
        d.num_textures, d.textures = len(texs), self.textures
        d.material_texture = self.material_texture.ctypes.data_as(C.POINTER(C.c_int32))
        d.num_texture_perms = len(perms)
        d.texture_perms = self.texture_perms.ctypes.data_as(C.POINTER(C.c_int32))


def host_texture_values(desc, tex, pts, precision=capi.RT_PREC_F64):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    rgb = np.full_like(pts, np.nan)
    dp = C.POINTER(C.c_double)
    assert lib().ptx_texture_values(C.byref(desc), precision, tex, pts.ctypes.data_as(dp), len(pts), rgb.ctypes.data_as(dp)) == 0
    return rgb


def host_render(packed, settings):
    """Sample-order CPU render of the product's trace_pixel (textured modes included)."""
    cw = settings.crop_w or settings.width
    ch = settings.crop_h or settings.height
    s = np.zeros((ch, cw, 3))
    segs = np.zeros((ch, cw), dtype=np.uint32)
    draws = np.zeros((ch, cw), dtype=np.uint32)
    rc = lib().ptx_render(C.byref(packed.desc), C.byref(settings), s.ctypes.data_as(C.POINTER(C.c_double)),
                          segs.ctypes.data_as(C.POINTER(C.c_uint32)), draws.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0
    return {"mean": s / settings.samples, "segments": segs, "draws": draws}


def bits(a):
    """float64 array -> its bit patterns (NaNs compare by payload, -0 != +0)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
