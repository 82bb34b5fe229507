"""Builds and binds tests/hostcheck (the GPU kernel's per-lane code compiled for the CPU).
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from blenderraytracer_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "pt_hostcheck.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "blenderraytracer_amd", "csrc", f) for f in ("pt_core.h", "pt_path.h", "scene_pack.h",
                                                                          "pool_order.h", "kernel_select.h", "js_math.h",
                                                                          "pool_plan.h", "render_plan.h")]
LIB = os.path.join(HERE, "hostcheck", "_build", "libpt_hostcheck.so")
_lib = None


def build(defines=(), name="libpt_hostcheck.so"):
    target = os.path.join(os.path.dirname(LIB), name)
    os.makedirs(os.path.dirname(target), exist_ok=True)
    if os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in DEPS):
        return target
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = "%s.tmp%d" % (target, os.getpid())     # parallel test workers: build aside, rename atomically
    subprocess.check_call([hipcc, "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           *[f"-D{d}" for d in defines], "-I", os.path.join(ROOT, "include"), SRC, "-o", tmp])
    os.replace(tmp, target)
    return target


def _bind(L):
    L.ptc_render.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), C.POINTER(C.c_double),
                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ptc_bvh_check.argtypes = [C.POINTER(capi.SceneDesc), C.c_longlong, C.c_uint, C.POINTER(C.c_longlong)]
    L.ptc_bvh_check.restype = C.c_longlong
    L.ptc_bvh_info.argtypes = [C.POINTER(capi.SceneDesc)] + [C.POINTER(C.c_int)] * 4
    L.ptc_away_check.argtypes = [C.c_longlong, C.c_uint, C.POINTER(C.c_longlong)]
    L.ptc_away_check.restype = C.c_longlong
    L.ptc_bvh_rays.argtypes = [C.POINTER(capi.SceneDesc), C.c_longlong, C.c_uint, C.c_longlong, C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ptc_bvh_rays.restype = C.c_longlong
    return L


def lib(defines=()):
    """The hostcheck library; `defines` builds (and caches) a variant with -D flags."""
    global _lib
    if defines:
        return _bind(C.CDLL(build(defines, "libpt_hostcheck_%s.so" % "_".join(d.replace("=", "") for d in defines))))
    if _lib is None:
        _lib = _bind(C.CDLL(build()))
    return _lib


def bvh_info(packed, L=None):
    """(deepest leaf of the binary trees, two-child nodes)"""
    return bvh_shape(packed, L)[:2]


def bvh_shape(packed, L=None):
    """(deepest leaf, two-child nodes, sphere indices of the dominant spheres tested before the walk)"""
    depth, nodes2, nbig, big = C.c_int(), C.c_int(), C.c_int(), (C.c_int * 8)()
    (L or lib()).ptc_bvh_info(C.byref(packed.desc), C.byref(depth), C.byref(nodes2), C.byref(nbig), big)
    return depth.value, nodes2.value, list(big[:nbig.value])


def bvh_check(packed, n, seed):
    """(rays whose brute-force and BVH closest hits differ, rays that hit something)"""
    hits = C.c_longlong()
    bad = lib().ptc_bvh_check(C.byref(packed.desc), n, seed, C.byref(hits))
    assert bad >= 0
    return bad, hits.value


def bvh_rays(packed, n, seed, host_n=None):
    """The BVH stress rays (n x 6 float64: origin, direction) and the host's World-order closest hit
    (t, kind, index) of the first host_n of them (default all) — the kernel's own code compiled for the
    CPU."""
    host_n = n if host_n is None else host_n
    rays = np.zeros((n, 6))
    t = np.full(n, np.nan)
    kind = np.full(n, -2, dtype=np.int32)
    idx = np.full(n, -2, dtype=np.int32)
    m = lib().ptc_bvh_rays(C.byref(packed.desc), n, seed, host_n, rays.ctypes.data_as(C.POINTER(C.c_double)),
                           t.ctypes.data_as(C.POINTER(C.c_double)), kind.ctypes.data_as(C.POINTER(C.c_int)),
                           idx.ctypes.data_as(C.POINTER(C.c_int)))
    assert m >= 0
    return rays[:m], t[:m], kind[:m], idx[:m]


WALKS = ("world", "two_child", "stackless", "grid", "grid_lds", "grid_lds_lean")


def walk_hits(packed, walk, rays):
    """Binary64 closest hits (t, sphere index; +inf and -1 on a miss) of n x 6 rays through one of WALKS (the
    kernel's own code compiled for the CPU); None when the scene has no grid for a grid walk."""
    L = lib()
    L.ptc_walk_hits.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, C.POINTER(C.c_double), C.c_longlong,
                                C.POINTER(C.c_double), C.POINTER(C.c_int)]
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    t = np.full(len(rays), np.nan)
    idx = np.full(len(rays), -2, dtype=np.int32)
    rc = L.ptc_walk_hits(C.byref(packed.desc), WALKS.index(walk), rays.ctypes.data_as(C.POINTER(C.c_double)), len(rays),
                         t.ctypes.data_as(C.POINTER(C.c_double)), idx.ctypes.data_as(C.POINTER(C.c_int)))
    if rc == -2:
        return None
    assert rc == 0
    return t, idx


def walk_hits_kind(packed, walk, rays, L=None):
    """walk_hits with rt_closest_hits' outputs: (t, kind, index within the kind); kind = index = -1 on a miss."""
    L = L or lib()
    ip = C.POINTER(C.c_int)
    L.ptc_walk_hits_kind.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, C.POINTER(C.c_double), C.c_longlong,
                                     C.POINTER(C.c_double), ip, ip]
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    t = np.full(len(rays), np.nan)
    kind = np.full(len(rays), -2, dtype=np.int32)
    idx = np.full(len(rays), -2, dtype=np.int32)
    rc = L.ptc_walk_hits_kind(C.byref(packed.desc), WALKS.index(walk), rays.ctypes.data_as(C.POINTER(C.c_double)), len(rays),
                              t.ctypes.data_as(C.POINTER(C.c_double)), kind.ctypes.data_as(ip), idx.ctypes.data_as(ip))
    if rc == -2:
        return None
    assert rc == 0
    return t, kind, idx


def hit_records(packed, precision, accel, rays, L=None):
    """rt_hit_records on the CPU: dict(t, kind, idx, point, normal, front, mat) of n x 6 rays."""
    L = L or lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.ptc_hit_records.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, C.c_int, dp, C.c_longlong, dp, ip, ip, dp, dp,
                                  C.POINTER(C.c_uint8), ip]
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = len(rays)
    out = {"t": np.zeros(n), "kind": np.full(n, -2, dtype=np.int32), "idx": np.full(n, -2, dtype=np.int32),
           "point": np.zeros((n, 3)), "normal": np.zeros((n, 3)), "front": np.full(n, 2, dtype=np.uint8),
           "mat": np.full(n, -2, dtype=np.int32)}
    assert L.ptc_hit_records(C.byref(packed.desc), precision, accel, rays.ctypes.data_as(dp), n, out["t"].ctypes.data_as(dp),
                             out["kind"].ctypes.data_as(ip), out["idx"].ctypes.data_as(ip), out["point"].ctypes.data_as(dp),
                             out["normal"].ctypes.data_as(dp), out["front"].ctypes.data_as(C.POINTER(C.c_uint8)),
                             out["mat"].ctypes.data_as(ip)) == 0
    return out


def shade_segments(packed, precision, accel, rays, keys, depth, variant=0, L=None):
    """rt_shade_segments on the CPU: (out_f n x 12: origin, direction, T, L; out_i n x 4: done, kind, index, draws),
    or None when the scene has what the variant leaves out."""
    L = L or lib()
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    L.ptc_shade_segments.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, C.c_int, C.c_int, dp, up, C.c_int, C.c_longlong, dp, ip]
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
    assert len(keys) == len(rays)
    out_f = np.zeros((len(rays), 12))
    out_i = np.full((len(rays), 4), -2, dtype=np.int32)
    rc = L.ptc_shade_segments(C.byref(packed.desc), precision, accel, variant, rays.ctypes.data_as(dp), keys.ctypes.data_as(up),
                              depth, len(rays), out_f.ctypes.data_as(dp), out_i.ctypes.data_as(ip))
    if rc == -2:
        return None
    assert rc == 0
    return out_f, out_i


def camera_rays(packed, settings, pixels, variant=0, L=None):
    """rt_camera_rays on the CPU: (out n x 6: origin, direction; draws n), or None when the variant refuses the camera
    or the AA mode."""
    L = L or lib()
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    L.ptc_camera_rays.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), C.c_int, ip, C.c_longlong, dp, up]
    pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((len(pixels), 6))
    draws = np.zeros(len(pixels), dtype=np.uint32)
    rc = L.ptc_camera_rays(C.byref(packed.desc), C.byref(settings), variant, pixels.ctypes.data_as(ip), len(pixels),
                           out.ctypes.data_as(dp), draws.ctypes.data_as(up))
    if rc == -2:
        return None
    assert rc == 0
    return out, draws


def grid_geometry(packed):
    """build_grid's result as the walk reads it: dict(lo, cs (binary32 values), n (cells per axis; zeros: no
    grid), far (grid_far), largest (most records in one cell))."""
    L = lib()
    L.ptc_grid_geometry.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    out, n3, largest = (C.c_double * 7)(), (C.c_int * 3)(), C.c_int()
    assert L.ptc_grid_geometry(C.byref(packed.desc), out, n3, C.byref(largest)) == 0
    return {"lo": np.array(out[0:3]), "cs": np.array(out[3:6]), "far": out[6], "n": np.array(n3[:]), "largest": largest.value}


EVENTS = ["f64_sphere_tests", "disc_nonneg", "second_root", "accept", "lambertian", "metal", "dielectric", "emissive",
          "miss", "samples", "sphere_draw_rounds", "disk_draw_rounds", "filter_tests", "dielectric_schlick",
          "tri_filter_tests", "tri_tests"]


def event_counts(packed, settings_list, walk):
    """Events per segment of the kernel's own code run on the CPU over the given crops (pt_core.h
    RT_HCOUNT; the instruction-floor model of bench.py): walk "grid" | "bvh" | "brute" as the GPU runs it."""
    L = lib(("RT_HOST_COUNTERS=1",))
    L.ptc_work.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), C.POINTER(C.c_double)]
    L.ptc_host_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    cnt = (C.c_ulonglong * 16)()
    L.ptc_host_counts(cnt, 1)
    out = (C.c_double * 4)()
    tot = [0.0] * 4
    for st in settings_list:
        st.accel = {"grid": 4, "bvh": capi.RT_ACCEL_BVH, "brute": capi.RT_ACCEL_BRUTE}[walk]
        assert L.ptc_work(C.byref(packed.desc), C.byref(st), out) == 0
        tot = [a + b for a, b in zip(tot, out)]
    L.ptc_host_counts(cnt, 1)
    seg = max(tot[0], 1.0)
    res = {"segments": tot[0], "walk_steps": tot[1] / seg, "sphere_tests_work": tot[2] / seg, "tri_tests": tot[3] / seg}
    res.update({n: cnt[k] / seg for k, n in enumerate(EVENTS)})
    return res


def render(packed, settings, L=None):
    """Per-pixel linear means, segment and draw counts computed by the kernel's own code on the CPU
    (`L`: a variant library from lib(defines))."""
    cw = settings.crop_w or settings.width
    ch = settings.crop_h or settings.height
    s = np.zeros((ch, cw, 3))
    segs = np.zeros((ch, cw), dtype=np.uint32)
    draws = np.zeros((ch, cw), dtype=np.uint32)
    rc = (L or lib()).ptc_render(C.byref(packed.desc), C.byref(settings), s.ctypes.data_as(C.POINTER(C.c_double)),
                          segs.ctypes.data_as(C.POINTER(C.c_uint32)), draws.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0
    return {"mean": s / settings.samples, "segments": segs, "draws": draws}


def pool_order(cw, ch, chunks, one_wave=True):
    """The pool's visiting order (pool_order.h): (items by workgroup / queue position, RT_TILE_BLOCK,
    RT_XCD_RUN, tiles)."""
    import numpy as np
    L = lib()
    L.ptc_pool_order.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    L.ptc_pool_order.restype = C.c_longlong
    tiles = ((cw + 7) // 8) * ((ch + 7) // 8)
    out = np.zeros(tiles * chunks, dtype=np.uint32)
    par = (C.c_int * 3)()
    n = L.ptc_pool_order(cw, ch, chunks, int(one_wave), out.ctypes.data_as(C.POINTER(C.c_uint32)), par)
    assert n == tiles * chunks
    return out, par[0], par[1], par[2]


PLAN_IN = ("cw", "ch", "sample_begin", "sample_end", "samples", "batch_samples", "max_depth", "pool", "first", "tri_bvh",
           "shards", "home_first", "want_segs", "want_draws", "want_preview", "err_active", "err_groups", "knobs",
           "refuse_fused", "refuse_slots_shard")
PLAN_DEFAULTS = dict(sample_begin=0, sample_end=0, batch_samples=0, max_depth=5, pool=1, first=0, tri_bvh=0, shards=1,
                     home_first=1, want_segs=0, want_draws=0, want_preview=0, err_active=0, err_groups=0, knobs=7,
                     refuse_fused=0, refuse_slots_shard=-1)
PLAN_HEAD = ("base", "s0", "s1", "batch", "nb", "devices", "queue", "gated", "preview", "ahead", "ring", "fchunk",
             "fdoubles", "err_chunk", "final_groups")
DEVICE_MODES = ("one", "whole", "split")
QUEUE_MODES = ("serial", "overlapped", "fused")
KNOB_OVERLAP, KNOB_ITEM_CANCEL, KNOB_FUSED_BATCHES, KNOB_FUSED_PREVIEW = 1, 2, 4, 8
_plan_out = None


def render_plan(**kw):
    """The plan of a render (render_plan.h plan_render) for PLAN_IN's fields by name (PLAN_DEFAULTS otherwise; knobs:
    the KNOB_* bits, default the shipped ones).  A dict of PLAN_HEAD with devices / queue as DEVICE_MODES / QUEUE_MODES
    strings, plus chunk_hint and slot_bytes (per shard), asks (the fit questions in order: (kind, shard, amount), kind
    "slots" | "fused"), launches (per batch a list of (begin, end, shard, chunk, chunks)) and groups_after."""
    L = lib()
    L.ptc_render_plan.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.c_longlong]
    L.ptc_render_plan.restype = C.c_longlong
    v = dict(PLAN_DEFAULTS, **kw)
    assert set(v) == set(PLAN_IN), sorted(set(v) ^ set(PLAN_IN))
    global _plan_out
    if _plan_out is None:
        _plan_out = (C.c_longlong * (80 + 6 * 8 * 1024))()
    out, cap = _plan_out, len(_plan_out)
    n = L.ptc_render_plan((C.c_int * len(PLAN_IN))(*[int(v[k]) for k in PLAN_IN]), out, cap)
    assert n >= 80, n
    res = dict(zip(PLAN_HEAD, out[:15]))
    res["devices"], res["queue"] = DEVICE_MODES[res["devices"]], QUEUE_MODES[res["queue"]]
    res["chunk_hint"] = list(out[16:16 + v["shards"]])
    res["slot_bytes"] = list(out[24:24 + v["shards"]])
    res["asks"] = [(("slots", "fused")[out[32 + 3 * k]], out[33 + 3 * k], out[34 + 3 * k]) for k in range(min(out[15], 16))]
    rows = [tuple(out[k:k + 6]) for k in range(80, n, 6)]
    per = v["shards"] if res["devices"] == "split" else 1
    res["launches"] = [[r[:5] for r in rows[k * per:(k + 1) * per]] for k in range(res["nb"])]
    res["groups_after"] = [rows[k * per][5] for k in range(res["nb"])]
    return res


KNOBS = ("bvh_walk", "lean", "lds_grid", "lds_nodes", "lds_tri", "tri_lds_nodes")
FACTS = ("num_lights", "num_tex", "num_tri_nodes", "num_tri_wide", "num_sphere_wide", "num_grid_cells", "use_grid",
         "num_planes", "num_boxes", "background", "cam_ortho", "stack_entries", "num_mats", "grid_lds_bytes")


def kernel_choice(packed, precision, bvh, pool=True, aa_mode=0, **knobs):
    """The trace kernel a launch of this scene runs (kernel_select.h select_kernel): a dict with the choice
    (acc, lds, lds_bytes, tri_lds_nodes, walk = rt_scene_walk's answer), the scene's facts and the two node
    kernels' occupancy constants.  knobs: the SelectKnobs fields by name; bvh_walk takes RT_BVH_WALK's string."""
    L = lib()
    L.ptc_kernel_choice.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                    C.POINTER(C.c_longlong)]
    L.ptc_parse_bvh_walk.argtypes = [C.c_char_p]
    k = (C.c_int * len(KNOBS))()
    L.ptc_default_knobs(k)
    for name, value in knobs.items():
        k[KNOBS.index(name)] = L.ptc_parse_bvh_walk(value.encode()) if name == "bvh_walk" else value
    out = (C.c_longlong * 23)()
    assert L.ptc_kernel_choice(C.byref(packed.desc), precision, int(bvh), int(pool), aa_mode, k, out) == 0
    res = dict(zip(("acc", "lds", "lds_bytes", "tri_lds_nodes", "walk") + FACTS, out[:19]))
    res.update(zip(("sphere_lds_waves", "sphere_lds_occ", "tri_lds_waves", "tri_lds_occ"), out[19:]))
    return res
