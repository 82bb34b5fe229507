"""The device's hit records (rt_hit_records: the trace kernels' closest-hit query, then pt_core.h hit_record, the
function shade_segment calls) against tests/shade_ref.py, on the scenes, rays, comparisons and bounds of
tests/test_shade.py: binary64 bit for bit, binary32 within the bounds derived there, the box face wherever the face is
unambiguous.  DESIGN.md §4 "Shading stages against an independent reference" records the printed ratios."""
import ctypes as C

import numpy as np
import pytest

import shade_ref as sr
import test_shade as cpu
from blenderraytracer_amd import capi

pytestmark = pytest.mark.gpu

ACCELS = pytest.mark.parametrize("accel", [capi.RT_ACCEL_BVH, capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_AUTO], ids=["bvh", "brute", "auto"])


def _ptr(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def device_hit_records(lib, rt, rays, precision, accel, only=None):
    """rt_hit_records' outputs by name (the layout of hostcheck_binding.hit_records); only: the outputs asked for, the
    others passed as NULL"""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = len(rays)
    out = {"t": np.zeros(n), "kind": np.full(n, -2, dtype=np.int32), "idx": np.full(n, -2, dtype=np.int32),
           "point": np.zeros((n, 3)), "normal": np.zeros((n, 3)), "front": np.full(n, 2, dtype=np.uint8),
           "mat": np.full(n, -2, dtype=np.int32)}
    types = {"t": C.c_double, "kind": C.c_int32, "idx": C.c_int32, "point": C.c_double, "normal": C.c_double,
             "front": C.c_uint8, "mat": C.c_int32}
    args = [_ptr(out[k], types[k]) if only is None or k in only else None for k in ("t", "kind", "idx", "point", "normal", "front", "mat")]
    capi.check(lib.rt_hit_records(rt.scene_handle(), precision, accel, _ptr(rays, C.c_double), n, *args), lib)
    return out if only is None else {k: out[k] for k in only}


@ACCELS
@pytest.mark.parametrize("name", cpu.NAMES)
def test_device_hit_records_equal_the_reference(gpu, name, accel):
    """Binary64, World order, the tree and the walk a render of the scene takes: t, kind and index are world_hit's, and
    point, normal, front and the material are shade_ref.hit_record's, bit for bit; a row without a hit has NaN, 0, -1."""
    f = cpu.family(name)
    assert cpu.f64_mismatch(f, device_hit_records(gpu, f["rt"], f["rays"], cpu.F64, accel)) == {}


@ACCELS
@pytest.mark.parametrize("name", cpu.NAMES)
def test_device_hit_records_binary32_within_bounds(gpu, name, accel):
    """Binary32 on the device (its own reciprocal division in the sphere normal): the bounds of tests/test_shade.py,
    front and the box face where they are decided; the worst error over its bound is printed per ray class."""
    f = cpu.family(name)
    h = device_hit_records(gpu, f["rt"], f["rays"], cpu.F32, accel)
    bad, info = cpu.f32_check(f, h, f"device {name} {('auto', 'brute', 'bvh')[accel]}")
    assert bad == {}
    if name in sr.FAMILIES:
        assert info["hits"].sum() >= 0.9 * (f["kind"] >= 0).sum()
        assert info["clear"].sum() >= 0.5 * info["hits"].sum()
    if name == "boxes":
        far = info["hits"] & (np.abs(info["ref"]["point"]).max(axis=1) >= 16)
        assert (info["face_ok"] & far).sum() >= 0.5 * far.sum()
        cpu.box_t_check(f, h, "device boxes")


def test_rt_hit_records_arguments(gpu):
    """Every output is optional and an output asked for alone has the bits of the full call; a ragged count (one
    workgroup and a part) and no ray at all; a bad precision, accel or NULL rays is RT_ERR_INVALID."""
    f = cpu.family("boxes")
    rays = f["rays"][:77]
    full = device_hit_records(gpu, f["rt"], rays, cpu.F64, capi.RT_ACCEL_BRUTE)
    for k in full:
        alone = device_hit_records(gpu, f["rt"], rays, cpu.F64, capi.RT_ACCEL_BRUTE, only=(k,))
        assert np.array_equal(alone[k].view(np.uint8), full[k].view(np.uint8)), k
    h = f["rt"].scene_handle()
    none = [None] * 7
    assert gpu.rt_hit_records(h, cpu.F64, capi.RT_ACCEL_BRUTE, None, 0, *none) == 0
    assert gpu.rt_hit_records(h, cpu.F64, capi.RT_ACCEL_BRUTE, None, 1, *none) == -1
    assert gpu.rt_hit_records(h, 7, capi.RT_ACCEL_BRUTE, _ptr(rays, C.c_double), 1, *none) == -1
    assert gpu.rt_hit_records(h, cpu.F64, 9, _ptr(rays, C.c_double), 1, *none) == -1
    assert gpu.rt_hit_records(None, cpu.F64, capi.RT_ACCEL_BRUTE, _ptr(rays, C.c_double), 1, *none) == -1


# ---- shade_segment and start_sample on the device (rt_shade_segments, rt_camera_rays) ------------------------------
def device_shade_segments(lib, rt, precision, accel, rays, keys, depth, variant=0):
    """rt_shade_segments' outputs (out_f n x 12, out_i n x 4), or None where the variant refuses the scene"""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
    out_f, out_i = np.zeros((len(rays), 12)), np.full((len(rays), 4), -2, dtype=np.int32)
    rc = lib.rt_shade_segments(rt.scene_handle(), precision, accel, variant, _ptr(rays, C.c_double), _ptr(keys, C.c_uint32), depth,
                               len(rays), _ptr(out_f, C.c_double), _ptr(out_i, C.c_int32))
    if rc == -1 and b"leaves out" in lib.rt_last_error():
        return None
    capi.check(rc, lib)
    return out_f, out_i


def device_camera_rays(lib, rt, settings, pixels, variant):
    pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 3)
    out, draws = np.zeros((len(pixels), 6)), np.zeros(len(pixels), dtype=np.uint32)
    rc = lib.rt_camera_rays(rt.scene_handle(), C.byref(settings), variant, _ptr(pixels, C.c_int32), len(pixels),
                            _ptr(out, C.c_double), _ptr(draws, C.c_uint32))
    if rc == -1 and b"lean kernels" in lib.rt_last_error():
        return None
    capi.check(rc, lib)
    return out, draws


@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BVH, capi.RT_ACCEL_BRUTE], ids=["bvh", "brute"])
@pytest.mark.parametrize("depth", cpu.DEPTHS)
@pytest.mark.parametrize("name", sr.SCATTER_SCENES)
def test_device_shade_segments_equal_the_reference(gpu, name, depth, accel):
    """shade_segment on the device, binary64: done, the hit, the draw count, the next origin and direction, T and L are
    shade_ref's bit for bit on every material scene and ray class (tests/test_shade.py's)."""
    f = cpu.scatter_family(name)
    got = device_shade_segments(gpu, f["rt"], cpu.F64, accel, f["rays"], f["keys"], depth)
    assert cpu.segment_mismatch(f, depth, got) == {}


@pytest.mark.parametrize("precision", [cpu.F64, cpu.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sr.SCATTER_SCENES)
def test_device_lean_variants_equal_the_general_one(gpu, name, precision):
    """The lean feature sets (the triangle-tree kernel's with its out-of-line exact Schlick path, the grid kernel's) give
    F_ALL's bits on the device in both precisions; a scene with boxes is refused."""
    f = cpu.scatter_family(name)
    base = device_shade_segments(gpu, f["rt"], precision, capi.RT_ACCEL_BRUTE, f["rays"], f["keys"], 5)
    for variant in (1, 2):
        got = device_shade_segments(gpu, f["rt"], precision, capi.RT_ACCEL_BRUTE, f["rays"], f["keys"], 5, variant)
        assert cpu.same_bits(got[0], base[0]).all() and np.array_equal(got[1], base[1]), variant
    boxes = cpu.family("boxes")
    for variant in (1, 2):
        assert device_shade_segments(gpu, boxes["rt"], precision, capi.RT_ACCEL_BRUTE, boxes["rays"][:4], np.zeros((4, 2)), 5, variant) is None


def test_device_schlick_knife_edge_takes_the_exact_path(gpu):
    f = cpu.scatter_family("dielectric")
    cpu.knife_edge_check(lambda rays, keys, variant: device_shade_segments(gpu, f["rt"], cpu.F64, capi.RT_ACCEL_BRUTE, rays, keys, 5,
                                                                           variant), "device")


def test_device_backgrounds_equal_the_reference(gpu):
    """The four backgrounds at three intensities on an empty scene, every direction class of tests/test_shade.py."""
    cpu.background_check(lambda rt, rays, keys: device_shade_segments(gpu, rt, cpu.F64, capi.RT_ACCEL_BRUTE, rays, keys, 5), "device")


def test_device_camera_rays_equal_the_reference(gpu):
    """start_sample on the device, binary64: shade_ref's camera rays bit for bit; the reloading form (the camera read
    from the kernel-argument segment) and the lean form give the same bits."""
    cpu.camera_check(lambda rt, st, px, variant: device_camera_rays(gpu, rt, st, px, variant), "device")


def test_device_camera_rays_binary32_within_bounds(gpu):
    cpu.camera_check(lambda rt, st, px, variant: device_camera_rays(gpu, rt, st, px, variant), "device f32", precision=cpu.F32)


@pytest.mark.parametrize("name", sr.SCATTER_SCENES)
def test_device_shade_segments_binary32_within_bounds(gpu, name):
    """Binary32 on the device (its own reciprocal division in normalize, its pow5): tests/test_shade.py's counted bounds,
    decisions and draws on the rays whose margins are clear."""
    f = cpu.scatter_family(name)
    shares = cpu.segment_check32(name, lambda rays, keys, depth: device_shade_segments(gpu, f["rt"], cpu.F32, capi.RT_ACCEL_BRUTE, rays, keys, depth),
                                 lambda rays: device_hit_records(gpu, f["rt"], rays, cpu.F32, capi.RT_ACCEL_BRUTE), "device")
    for c in ("normal", "random", "inside", "length"):
        assert shares[c] >= 0.9, (name, c, shares)


def test_device_backgrounds_binary32_within_bounds(gpu):
    """The device's own powf, expf and normalize in the four backgrounds against tests/test_shade.py's binary32 bounds."""
    cpu.background_check32(lambda rt, rays, keys: device_shade_segments(gpu, rt, cpu.F32, capi.RT_ACCEL_BRUTE, rays, keys, 5), "device")


def test_device_camera_rays_equal_the_cpu_build(gpu):
    """The CPU twin fills its ImageParams itself: binary64 rays of the device and of the twin are the same bits (both are
    compared with shade_ref as well; this pins the twin's set-up to rt_camera_rays')."""
    import hostcheck_binding as hb
    for cname in ("lens", "ortho_lens"):
        for mode in (0, 1, 2):
            rt = cpu.camera_tracer(sr.CAMERA_SPECS[cname], 30, 300, mode, 4242)
            px = sr.camera_pixels(30, 300)
            a, b = device_camera_rays(gpu, rt, rt.settings(), px, 0), hb.camera_rays(rt.packed(), rt.settings(), px, 0)
            assert cpu.same_bits(a[0], b[0]).all() and np.array_equal(a[1], b[1]), (cname, mode)
            rt.close()


def test_rt_shade_segments_and_camera_rays_arguments(gpu):
    """Either output may be NULL and the other keeps its bits; a count that is no multiple of 64; no ray at all; a bad
    precision, accel, variant, NULL inputs and a pixel outside the image are RT_ERR_INVALID."""
    f = cpu.scatter_family("blend")
    rays, keys = np.ascontiguousarray(f["rays"][:77]), np.ascontiguousarray(f["keys"][:77])
    h = f["rt"].scene_handle()
    F, B = cpu.F64, capi.RT_ACCEL_BRUTE
    full = device_shade_segments(gpu, f["rt"], F, B, rays, keys, 5)
    out_f, out_i = np.zeros((77, 12)), np.zeros((77, 4), dtype=np.int32)
    rp, kp = _ptr(rays, C.c_double), _ptr(keys, C.c_uint32)
    assert gpu.rt_shade_segments(h, F, B, 0, rp, kp, 5, 77, _ptr(out_f, C.c_double), None) == 0
    assert gpu.rt_shade_segments(h, F, B, 0, rp, kp, 5, 77, None, _ptr(out_i, C.c_int32)) == 0
    assert cpu.same_bits(out_f, full[0]).all() and np.array_equal(out_i, full[1])
    assert gpu.rt_shade_segments(h, F, B, 0, rp, kp, 5, 77, None, None) == 0
    assert gpu.rt_shade_segments(h, F, B, 0, None, None, 5, 0, None, None) == 0
    assert gpu.rt_shade_segments(h, F, B, 0, None, kp, 5, 1, None, None) == -1
    assert gpu.rt_shade_segments(h, F, B, 0, rp, None, 5, 1, None, None) == -1
    assert gpu.rt_shade_segments(h, F, B, 3, rp, kp, 5, 1, None, None) == -1
    assert gpu.rt_shade_segments(h, F, B, -1, rp, kp, 5, 1, None, None) == -1
    assert gpu.rt_shade_segments(h, 7, B, 0, rp, kp, 5, 1, None, None) == -1
    assert gpu.rt_shade_segments(h, F, 9, 0, rp, kp, 5, 1, None, None) == -1
    assert gpu.rt_shade_segments(None, F, B, 0, rp, kp, 5, 1, None, None) == -1
    rt = cpu.camera_tracer(sr.CAMERA_SPECS["lens"], 64, 64, 0, 17)
    st = rt.settings()
    px = np.ascontiguousarray(np.array([(i % 64, (7 * i) % 64, i) for i in range(77)], dtype=np.int32))
    full = device_camera_rays(gpu, rt, st, px, 0)
    out, draws = np.zeros((77, 6)), np.zeros(77, dtype=np.uint32)
    ch, pp = rt.scene_handle(), _ptr(px, C.c_int32)
    assert gpu.rt_camera_rays(ch, C.byref(st), 0, pp, 77, _ptr(out, C.c_double), None) == 0
    assert gpu.rt_camera_rays(ch, C.byref(st), 0, pp, 77, None, _ptr(draws, C.c_uint32)) == 0
    assert cpu.same_bits(out, full[0]).all() and np.array_equal(draws, full[1])
    assert gpu.rt_camera_rays(ch, C.byref(st), 0, pp, 77, None, None) == 0
    assert gpu.rt_camera_rays(ch, C.byref(st), 0, None, 0, None, None) == 0
    assert gpu.rt_camera_rays(ch, C.byref(st), 0, None, 1, None, None) == -1
    assert gpu.rt_camera_rays(ch, None, 0, pp, 1, None, None) == -1
    assert gpu.rt_camera_rays(None, C.byref(st), 0, pp, 1, None, None) == -1
    assert gpu.rt_camera_rays(ch, C.byref(st), 4, pp, 1, None, None) == -1
    assert gpu.rt_camera_rays(ch, C.byref(st), -1, pp, 1, None, None) == -1
    for bad in ((64, 0, 0), (0, 64, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        one = np.array([bad], dtype=np.int32)
        assert gpu.rt_camera_rays(ch, C.byref(st), 0, _ptr(one, C.c_int32), 1, None, None) == -1, bad
    rt.close()
