"""Procedural textures on the GPU against the fixtures the real reference produced (tests/golden/textures/,
tests/js/texture_reference.mjs): bit-exact binary64 renders, the device's texture values, walk and kernel
routing, binary32 accuracy, lowering, and the Node drop-in.  The CPU side is tests/test_textures.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import texcheck_binding as tb
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = ("mean", "segments", "draws")


@pytest.mark.parametrize("case", tb.CASES)
def test_f64_sample_order_bit_exact_to_reference(gpu, case):
    """As tests/test_gpu_parity.py's test of the same name, for scenes the reference renders with its own
    TexturedLambertian / TexturedMetal: means, post-gamma values (float32 storage) and RGBA8 equal the
    fixtures exactly, with the reference's segment and draw counts."""
    rt, c = tb.tracer_for(case, precision=capi.RT_PREC_F64)
    rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
    r = rt.render(crop=c["crop"], want=WANT)
    lin = tb.load_array(case, "linear")
    assert not np.isnan(lin).any() and not np.isnan(r["mean"]).any()
    same = tb.bits(r["mean"]) == tb.bits(lin)
    print(f"{case}: {same.mean():.4f} of channels bit-identical")
    assert same.all()
    assert np.array_equal(r["segments"], tb.load_array(case, "segs"))
    assert np.array_equal(r["draws"], tb.load_array(case, "draws"))
    assert np.array_equal(r["rgba8"], tb.load_array(case, "rgba8"))
    assert np.array_equal(r["post"][..., :3], tb.load_array(case, "post").astype(np.float32))
    rt.close()


@pytest.mark.parametrize("case", tb.CASES)
def test_f64_pool_order(gpu, case):
    """The sample pool: the reference's segments, draws and RGBA8; means within the summation-order bound
    (1e-12 relative, tests/test_gpu_parity.py)."""
    rt, c = tb.tracer_for(case, precision=capi.RT_PREC_F64)
    r = rt.render(crop=c["crop"], want=WANT)
    lin = tb.load_array(case, "linear")
    assert np.array_equal(r["segments"], tb.load_array(case, "segs"))
    assert np.array_equal(r["draws"], tb.load_array(case, "draws"))
    assert np.array_equal(r["rgba8"], tb.load_array(case, "rgba8"))
    rel = float(np.max(np.abs(r["mean"] - lin) / np.maximum(np.abs(lin), 1e-300)))
    print(f"{case}: pool-order max relative difference {rel:.2e}")
    assert rel <= 1e-12
    rt.close()


def test_device_texture_values_equal_the_kats(gpu):
    """rt_texture_values (the trace kernels' texture_value, on the device) == the reference's Texture.value at
    every KAT point, bit for bit in binary64; binary32 agrees loosely away from checker edges (smoke)."""
    k = tb.kats()
    ks = tb.KatScene()
    h = C.c_void_p()
    capi.check(gpu.rt_scene_create(C.byref(ks.desc), 0, C.byref(h)), gpu)
    dp = C.POINTER(C.c_double)
    try:
        for i, t in enumerate(k["textures"]):
            pts, want = np.array(t["points"], dtype=np.float64), np.array(t["values"], dtype=np.float64)
            got = np.full_like(pts, np.nan)
            capi.check(gpu.rt_texture_values(h, capi.RT_PREC_F64, i, pts.ctypes.data_as(dp), len(pts), got.ctypes.data_as(dp)), gpu)
            bad = np.flatnonzero((tb.bits(got) != tb.bits(want)).any(axis=1))
            assert bad.size == 0, (t["type"], t["scale"], pts[bad[:3]], got[bad[:3]], want[bad[:3]])
        # binary32: the first 60 points (|p| <= 3) of the smooth textures
        for i, t in enumerate(k["textures"]):
            if t["type"] == "checker":
                continue
            pts, want = np.array(t["points"][:60], dtype=np.float64), np.array(t["values"][:60], dtype=np.float64)
            got = np.full_like(pts, np.nan)
            capi.check(gpu.rt_texture_values(h, capi.RT_PREC_F32, i, pts.ctypes.data_as(dp), len(pts), got.ctypes.data_as(dp)), gpu)
            assert np.max(np.abs(got - want)) <= 1e-3, (t["type"], t["scale"])
        got = np.zeros((1, 3))
        assert gpu.rt_texture_values(h, capi.RT_PREC_F64, len(k["textures"]), got.ctypes.data_as(dp), 1, got.ctypes.data_as(dp)) == -1
        assert gpu.rt_texture_values(h, capi.RT_PREC_F64, -1, got.ctypes.data_as(dp), 1, got.ctypes.data_as(dp)) == -1
    finally:
        gpu.rt_scene_destroy(h)


@pytest.mark.parametrize("case", tb.CASES)
def test_brute_and_bvh_are_bit_identical(gpu, case):
    """RT_ACCEL_BRUTE and RT_ACCEL_BVH renders of a textured scene: the same bits, in both summation orders
    and with counting off; rt_scene_walk reports the walk that ran (never the grid)."""
    out = {}
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt, c = tb.tracer_for(case, precision=capi.RT_PREC_F64, accel=accel)
        assert gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, accel) == (0 if accel == capi.RT_ACCEL_BRUTE else 1)
        assert gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F32, capi.RT_ACCEL_AUTO) in (0, 1)
        pool = rt.render(crop=c["crop"], want=WANT)
        plain = rt.render(crop=c["crop"], want=("mean",))                  # the kernels without counting
        assert np.array_equal(tb.bits(pool["mean"]), tb.bits(plain["mean"]))
        rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
        out[accel] = (pool, rt.render(crop=c["crop"], want=WANT))
        rt.close()
    for a, b in zip(out[capi.RT_ACCEL_BRUTE], out[capi.RT_ACCEL_BVH]):
        assert np.array_equal(tb.bits(a["mean"]), tb.bits(b["mean"]))
        assert np.array_equal(a["segments"], b["segments"]) and np.array_equal(a["draws"], b["draws"])
        assert np.array_equal(a["rgba8"], b["rgba8"])


def test_textured_sphere_scene_leaves_the_grid(gpu):
    """A sphere-only scene that walks the grid (RTOW) walks the tree once its ground is textured, and the
    progressive (batched, cancellable) render of the textured scene equals its one-batch render."""
    data = load_scene_json("rtow.json")
    rt = GpuRayTracer(96, 54, seed=5)
    assert rt.load_from_json(data)
    assert gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, capi.RT_ACCEL_AUTO) == 2
    rt.close()
    ground = max((o for o in data["objects"] if o["type"] == "sphere"), key=lambda o: o["radius"])
    assert ground["material"]["type"] == "lambertian"
    ground["material"]["texture"] = {"type": "checkerboard"}
    rt = GpuRayTracer(96, 54, seed=5)
    assert rt.load_from_json(data)
    rt.update_render_settings({"maxBounces": 5, "samples": 16})
    assert rt.packed().num_textures == 1
    for prec in (capi.RT_PREC_F64, capi.RT_PREC_F32):
        assert gpu.rt_scene_walk(rt.scene_handle(), prec, capi.RT_ACCEL_AUTO) == 1
    one = rt.render(want=WANT)
    seen = []
    batched = rt.render(want=WANT, batch_samples=4, on_progress=lambda f: seen.append(f) and False)
    assert len(seen) >= 4
    assert np.array_equal(one["segments"], batched["segments"]) and np.array_equal(one["draws"], batched["draws"])
    assert np.array_equal(one["rgba8"], batched["rgba8"])
    assert np.max(np.abs(one["mean"] - batched["mean"]) / np.maximum(np.abs(one["mean"]), 1e-300)) <= 1e-12
    rt.close()


@pytest.mark.parametrize("case", tb.CASES)
def test_f32_nan_pattern_and_rms(gpu, case):
    """Binary32 mode (textures in float with the device's own sin): the reference's NaN pattern and a post-gamma
    RMS within 3e-2, the bound tests/test_gpu_parity.py::test_f32_rms uses for low-spp fixtures."""
    rt, c = tb.tracer_for(case, precision=capi.RT_PREC_F32)
    r = rt.render(crop=c["crop"])
    post = tb.load_array(case, "post")
    ok = ~np.isnan(post)
    assert np.array_equal(np.isnan(r["post"][..., :3]), ~ok)
    rms = float(np.sqrt(np.mean((r["post"][..., :3][ok] - post[ok]) ** 2))) if ok.any() else 0.0
    print(f"{case}: f32 post-gamma RMS {rms:.2e}")
    assert rms <= 3e-2
    rt.close()


@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH], ids=["brute", "bvh"])
def test_f32_sample_order_matches_pool(gpu, accel):
    """The binary32 lane-per-pixel textured kernels against the binary32 pool kernels: the same samples (same
    segments and draws per pixel), added in another order (the summation-order bound of test_f64_pool_order)."""
    rt, c = tb.tracer_for("tex_kitchen_sink", precision=capi.RT_PREC_F32, accel=accel)
    pool = rt.render(crop=c["crop"], want=WANT)
    rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
    order = rt.render(crop=c["crop"], want=WANT)
    rt.close()
    assert np.array_equal(pool["segments"], order["segments"]) and np.array_equal(pool["draws"], order["draws"])
    assert not np.isnan(order["mean"]).any() and order["mean"].max() > 0
    assert np.max(np.abs(pool["mean"] - order["mean"]) / np.maximum(np.abs(order["mean"]), 1e-300)) <= 1e-12


def test_solid_lowered_scene_renders_like_its_plain_twin(gpu):
    """The JSON extension's solid branch (an unknown texture type) is the plain material: same packed bytes, same
    walk (the plain scene's own kernels) and the same render, bit for bit."""
    import copy
    plain = load_scene_json("sample_scene.json")
    lowered = copy.deepcopy(plain)
    n = 0
    for o in lowered["objects"]:
        if o.get("material", {}).get("type") in ("lambertian", "metal"):
            o["material"]["texture"] = {"type": "solid", "scale": 3}
            n += 1
    assert n >= 2
    res = []
    for data in (plain, lowered):
        rt = GpuRayTracer(64, 48, seed=9)
        assert rt.load_from_json(data)
        rt.update_render_settings({"maxBounces": 5, "samples": 8})
        p = rt.packed()
        assert p.num_textures == 0
        res.append((bytes(C.string_at(p.materials, 72 * p.num_materials)), bytes(C.string_at(p.objects, 64 * p.num_objects)),
                    gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, capi.RT_ACCEL_AUTO), rt.render(want=WANT)))
        rt.close()
    assert res[0][:3] == res[1][:3]
    for k in ("mean", "segments", "draws", "rgba8", "post"):
        assert np.array_equal(res[0][3][k], res[1][3][k]), k


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_drop_in_with_the_twin_classes_matches_the_fixture(gpu, tmp_path):
    """GpuRayTracer (Node, N-API) with TexturedLambertian / TexturedMetal twins on case 1: the fixture's RGBA8."""
    assert os.path.exists(os.path.join(ROOT, "blenderraytracer_amd", "lib", "rt_napi.node")), "rt_napi.node missing on the GPU box"
    out = tmp_path / "rgba8.bin"
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "texture_host_tool.mjs"), "render",
                        "tex_checker_spheres", str(out)], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    want = tb.load_array("tex_checker_spheres", "rgba8")
    got = np.frombuffer(out.read_bytes(), dtype=np.uint8).reshape(want.shape)
    assert np.array_equal(got, want)


def test_cli_renders_a_textured_scene_file(gpu, tmp_path):
    """rt_render_cli (the C++ JSON loader) on a scene file with "texture" entries, no new flag: the reference's
    RGBA8 frame (the pool-order frame test_f64_pool_order pins for the Python host)."""
    cli = os.path.join(ROOT, "blenderraytracer_amd", "lib", "rt_render_cli")
    assert os.path.exists(cli), "rt_render_cli missing on the GPU box"
    c = tb.manifest()["cases"]["tex_kitchen_sink"]
    out = tmp_path / "img.pam"
    r = subprocess.run([cli, os.path.join(ROOT, "scenes", c["scene"]), "--width", str(c["width"]), "--height", str(c["height"]),
                        "--spp", "8", "--depth", "5", "--seed", str(c["seed"]), "--aa", "stochastic", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    head, _, body = out.read_bytes().partition(b"ENDHDR\n")
    img = np.frombuffer(body, dtype=np.uint8).reshape(c["height"], c["width"], 4)
    assert np.array_equal(img, tb.load_array("tex_kitchen_sink", "rgba8"))
