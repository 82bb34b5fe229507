"""Direct lighting from scene lights on the GPU against the fixtures the real reference produced
(tests/golden/lights/, tests/js/lights_reference.mjs): bit-exact binary64 renders, the device's occlusion query,
kernel routing, binary32 accuracy, progressive renders, the Node drop-in and the CLI.  The CPU side is
tests/test_lights.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lightcheck_binding as lb
from blenderraytracer_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = ("mean", "segments", "draws")
ACCELS = pytest.mark.parametrize("accel", [capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH], ids=["brute", "bvh"])


@pytest.mark.parametrize("case", lb.CASES)
def test_f64_sample_order_bit_exact_to_reference(gpu, case):
    """Binary64 in sample order: means, post-gamma values (float32 storage) and RGBA8 equal the fixtures of the
    reference's lit rayColor exactly, with its segment and draw counts (shadow rays are not segments)."""
    rt, c = lb.tracer_for(case, precision=capi.RT_PREC_F64)
    rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
    r = rt.render(crop=lb.crop_of(c), want=WANT)
    lin = lb.load_array(case, "linear")
    assert not np.isnan(lin).any() and not np.isnan(r["mean"]).any()
    same = lb.bits(r["mean"]) == lb.bits(lin)
    print(f"{case}: {same.mean():.4f} of channels bit-identical")
    assert same.all()
    assert np.array_equal(r["segments"], lb.load_array(case, "segs"))
    assert np.array_equal(r["draws"], lb.load_array(case, "draws"))
    assert np.array_equal(r["rgba8"], lb.load_array(case, "rgba8"))
    assert np.array_equal(r["post"][..., :3], lb.load_array(case, "post").astype(np.float32))
    rt.close()


@pytest.mark.parametrize("case", lb.CASES)
def test_f64_pool_order(gpu, case):
    """The sample pool (Lacc += T (.) direct): the reference's segments, draws and RGBA8; means within the
    summation-order bound (1e-12 relative, tests/test_gpu_parity.py)."""
    rt, c = lb.tracer_for(case, precision=capi.RT_PREC_F64)
    r = rt.render(crop=lb.crop_of(c), want=WANT)
    lin = lb.load_array(case, "linear")
    assert np.array_equal(r["segments"], lb.load_array(case, "segs"))
    assert np.array_equal(r["draws"], lb.load_array(case, "draws"))
    assert np.array_equal(r["rgba8"], lb.load_array(case, "rgba8"))
    rel = float(np.max(np.abs(r["mean"] - lin) / np.maximum(np.abs(lin), 1e-300)))
    print(f"{case}: pool-order max relative difference {rel:.2e}")
    assert rel <= 1e-12
    rt.close()


@pytest.mark.parametrize("case", lb.CASES)
def test_brute_and_bvh_are_bit_identical(gpu, case):
    """RT_ACCEL_BRUTE and RT_ACCEL_BVH renders of a lit scene: the same bits in both summation orders and with
    counting off; rt_scene_walk reports the walk that ran (never the grid)."""
    out = {}
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt, c = lb.tracer_for(case, precision=capi.RT_PREC_F64, accel=accel)
        assert gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, accel) == (0 if accel == capi.RT_ACCEL_BRUTE else 1)
        pool = rt.render(crop=lb.crop_of(c), want=WANT)
        plain = rt.render(crop=lb.crop_of(c), want=("mean",))              # the kernels without counting
        assert np.array_equal(lb.bits(pool["mean"]), lb.bits(plain["mean"]))
        rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
        out[accel] = (pool, rt.render(crop=lb.crop_of(c), want=WANT))
        rt.close()
    for a, b in zip(out[capi.RT_ACCEL_BRUTE], out[capi.RT_ACCEL_BVH]):
        assert np.array_equal(lb.bits(a["mean"]), lb.bits(b["mean"]))
        assert np.array_equal(a["segments"], b["segments"]) and np.array_equal(a["draws"], b["draws"])
        assert np.array_equal(a["rgba8"], b["rgba8"])


@pytest.mark.parametrize("case", ["lit_sample_scene", "lit_rtow_crop", "lit_cornell_crop"])
def test_lit_and_unlit_renders_share_segments_and_draws(gpu, case):
    """Per-pixel segments and draws of the lit render equal the unlit render's of the same scene (the default:
    direct lighting off, the scene's lights ignored, the kernels the scene always ran), while the means differ."""
    lit_rt, c = lb.tracer_for(case, precision=capi.RT_PREC_F64)
    lit = lit_rt.render(crop=lb.crop_of(c), want=WANT)
    lit_rt.close()
    rt, _ = lb.tracer_for(case, direct_lighting=False, precision=capi.RT_PREC_F64)
    assert rt.packed().num_lights == 0
    unlit = rt.render(crop=lb.crop_of(c), want=WANT)
    assert np.array_equal(lit["segments"], unlit["segments"]) and np.array_equal(lit["draws"], unlit["draws"])
    assert (unlit["mean"] <= lit["mean"] * (1 + 1e-12)).all() and (unlit["mean"] < lit["mean"]).mean() > 0.3
    # turning the setting on marks the scene dirty and renders the lit frame
    rt.update_render_settings({**c["settings_in"], "directLighting": True})
    again = rt.render(crop=lb.crop_of(c), want=WANT)
    assert np.array_equal(lb.bits(again["mean"]), lb.bits(lit["mean"]))
    rt.close()


def _occluded(lib, rt, rays, tmax, precision, accel):
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    tmax = np.ascontiguousarray(tmax, dtype=np.float64)
    out = np.full(len(rays), 7, dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    capi.check(lib.rt_occluded(rt.scene_handle(), precision, accel, rays.ctypes.data_as(dp), tmax.ctypes.data_as(dp),
                               len(rays), out.ctypes.data_as(C.POINTER(C.c_uint8))), lib)
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def _closest_t(lib, rt, rays, accel, precision=capi.RT_PREC_F64):
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    t = np.full(len(rays), np.nan)
    kind = np.full(len(rays), -2, dtype=np.int32)
    capi.check(lib.rt_closest_hits(rt.scene_handle(), precision, accel, rays.ctypes.data_as(C.POINTER(C.c_double)),
                                   len(rays), t.ctypes.data_as(C.POINTER(C.c_double)),
                                   kind.ctypes.data_as(C.POINTER(C.c_int32)), None), lib)
    return t, kind


@pytest.mark.parametrize("case", lb.CASES)
def test_rt_occluded_equals_kats_and_closest_hits(gpu, case):
    """rt_occluded (the lit kernels' any-hit query on the device), binary64, both accels: every occlusion KAT
    verdict of the reference's World.hit; and on 20,000 stress rays of the scene (the BVH tests' generator:
    near-tangent spheres, triangle edges and vertices) the verdict of rt_closest_hits' own t < tmax, for tmax at
    the hit's t exactly (never occluded), one ulp above (occluded), half and twice t, and +inf."""
    import hostcheck_binding as hb
    rt, c = lb.tracer_for(case, precision=capi.RT_PREC_F64)
    rays, tmax, want = lb.occlusion_queries(case)
    r, _, _, _ = hb.bvh_rays(rt.packed(), 20_000, 77, 0)
    assert len(r) > 18_000
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        got = _occluded(gpu, rt, rays, tmax, capi.RT_PREC_F64, accel)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (case, accel, bad[:5], rays[bad[:5]], tmax[bad[:5]])
        t, kind = _closest_t(gpu, rt, r, accel)
        hit = kind >= 0
        assert hit.sum() > len(r) // 10 and np.isinf(t[~hit]).all()
        for name, lim in (("t", t), ("t+", np.nextafter(t, np.inf)), ("t/2", t * 0.5), ("2t", t * 2.0),
                          ("inf", np.full(len(r), np.inf))):
            occ = _occluded(gpu, rt, r, lim, capi.RT_PREC_F64, accel)
            expect = hit & (t < lim)
            bad = np.flatnonzero(occ != expect)
            assert bad.size == 0, (case, accel, name, bad[:5], r[bad[:5]], t[bad[:5]])
        assert not _occluded(gpu, rt, r, t, capi.RT_PREC_F64, accel).any()
    # binary32 against rt_closest_hits in RT_PREC_F32 (the same per-primitive arithmetic), limits in binary32: the
    # hit's own t, the next float above, half, twice, +inf.  World order tests every primitive in both queries, so
    # the verdict equals t < tmax for every limit.  In the tree walk the nodes a query enters depend on its limit,
    # and a binary32 candidate t of a stress ray (|o| ~ 1e3, |d| ~ 1e4: cancellation in the discriminant) can lie
    # before its own box's entry, so a hit the closest-hit walk reached under a larger limit may be culled under
    # a limit just above it.  What holds there: the any-hit walk's limit never exceeds the closest-hit walk's, so
    # it enters a subset of its nodes and sees a subset of its candidates, all >= the closest t — no verdict is
    # true where t < tmax is false (every limit), none is true at t and t/2; and with tmax = +inf both walks start
    # unlimited and find a first candidate in the same nodes, so the verdict equals "hit".
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        t, kind = _closest_t(gpu, rt, r, accel, capi.RT_PREC_F32)
        hit = kind >= 0
        t32 = t.astype(np.float32)
        assert np.array_equal(t32.astype(np.float64), t)                # the device's t is a float
        assert hit.sum() > len(r) // 10 and np.isinf(t[~hit]).all()
        for name, lim in (("t", t32), ("t+", np.nextafter(t32, np.float32(np.inf))), ("t/2", t32 * np.float32(0.5)),
                          ("2t", t32 * np.float32(2)), ("inf", np.full(len(r), np.inf, dtype=np.float32))):
            occ = _occluded(gpu, rt, r, lim.astype(np.float64), capi.RT_PREC_F32, accel)
            expect = hit & (t32 < lim)
            print(f"{case} f32 accel {accel} tmax {name}: {(occ == expect).mean():.4f} agree")
            exact = accel == capi.RT_ACCEL_BRUTE or name in ("t", "t/2", "inf")
            bad = np.flatnonzero(occ != expect if exact else occ & ~expect)
            assert bad.size == 0, (case, accel, "f32", name, bad[:5], r[bad[:5]], t[bad[:5]])
    rt.close()


def test_lit_rtow_leaves_the_grid_and_the_lean_kernels(gpu):
    """RTOW walks the grid (rt_scene_walk 2); with direct lighting it walks the trees (1) in both precisions, and
    World order when asked to."""
    rt, c = lb.tracer_for("lit_rtow_crop", direct_lighting=False)
    assert gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, capi.RT_ACCEL_AUTO) == 2
    rt.update_render_settings({**c["settings_in"], "directLighting": True})
    for prec in (capi.RT_PREC_F64, capi.RT_PREC_F32):
        assert gpu.rt_scene_walk(rt.scene_handle(), prec, capi.RT_ACCEL_AUTO) == 1
        assert gpu.rt_scene_walk(rt.scene_handle(), prec, capi.RT_ACCEL_BVH) == 1
        assert gpu.rt_scene_walk(rt.scene_handle(), prec, capi.RT_ACCEL_BRUTE) == 0
    rt.close()


@pytest.mark.parametrize("case", lb.CASES)
def test_f32_nan_pattern_and_rms(gpu, case):
    """Binary32 mode: the reference's NaN pattern and a post-gamma RMS within 3e-2, the project's bound for
    low-spp fixtures (tests/test_gpu_parity.py::test_f32_rms)."""
    rt, c = lb.tracer_for(case, precision=capi.RT_PREC_F32)
    r = rt.render(crop=lb.crop_of(c))
    post = lb.load_array(case, "post")
    ok = ~np.isnan(post)
    assert np.array_equal(np.isnan(r["post"][..., :3]), ~ok)
    rms = float(np.sqrt(np.mean((r["post"][..., :3][ok] - post[ok]) ** 2))) if ok.any() else 0.0
    print(f"{case}: f32 post-gamma RMS {rms:.2e}")
    assert rms <= 3e-2
    rt.close()


@ACCELS
def test_f32_sample_order_matches_pool(gpu, accel):
    """The binary32 lane-per-pixel lit kernels against the binary32 pool kernels: the same samples (same
    segments and draws per pixel), added in another order (the summation-order bound of test_f64_pool_order)."""
    rt, c = lb.tracer_for("lit_kitchen_sink", precision=capi.RT_PREC_F32, accel=accel)
    pool = rt.render(crop=lb.crop_of(c), want=WANT)
    rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
    order = rt.render(crop=lb.crop_of(c), want=WANT)
    rt.close()
    assert np.array_equal(pool["segments"], order["segments"]) and np.array_equal(pool["draws"], order["draws"])
    assert not np.isnan(order["mean"]).any() and order["mean"].max() > 0
    assert np.max(np.abs(pool["mean"] - order["mean"]) / np.maximum(np.abs(order["mean"]), 1e-300)) <= 1e-12


def test_progressive_and_resumed_renders_equal_the_one_batch_render(gpu):
    """A lit render in batches equals the one-batch render: bit for bit in sample order, also across a cancel,
    checkpoint and resume; the sample pool's batched render keeps segments, draws and RGBA8 and stays within the
    summation-order bound."""
    case = "lit_rtow_crop"
    rt, c = lb.tracer_for(case, precision=capi.RT_PREC_F64)
    crop = lb.crop_of(c)
    one = rt.render(crop=crop, want=WANT)
    seen = []
    batched = rt.render(crop=crop, want=WANT, batch_samples=4, on_progress=lambda f: seen.append(f) and False)
    assert len(seen) >= 4
    assert np.array_equal(one["segments"], batched["segments"]) and np.array_equal(one["draws"], batched["draws"])
    assert np.array_equal(one["rgba8"], batched["rgba8"])
    assert np.max(np.abs(one["mean"] - batched["mean"]) / np.maximum(np.abs(one["mean"]), 1e-300)) <= 1e-12
    rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
    full = rt.render(crop=crop, want=("mean",))
    assert np.array_equal(lb.bits(full["mean"]), lb.bits(lb.load_array(case, "linear")))
    four = rt.render(crop=crop, want=("mean",), batch_samples=4)
    assert np.array_equal(lb.bits(four["mean"]), lb.bits(full["mean"]))
    with pytest.raises(RuntimeError, match="CANCELLED"):
        rt.render(crop=crop, batch_samples=1, on_progress=lambda f: True)
    sums, done = rt.checkpoint(crop=crop)
    rt.close()
    assert 0 < done < 16
    rt2, _ = lb.tracer_for(case, precision=capi.RT_PREC_F64)
    rt2.sum_order = capi.RT_SUM_SAMPLE_ORDER
    res = rt2.render(crop=crop, want=("mean",), resume=(sums, done), batch_samples=4)
    assert np.array_equal(lb.bits(res["mean"]), lb.bits(full["mean"]))
    rt2.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_drop_in_with_direct_lighting_matches_the_fixture(gpu, tmp_path):
    """GpuRayTracer (Node, N-API) with updateRenderSettings({directLighting: true}): lit_sample_scene's RGBA8."""
    assert os.path.exists(os.path.join(ROOT, "blenderraytracer_amd", "lib", "rt_napi.node")), "rt_napi.node missing on the GPU box"
    out = tmp_path / "rgba8.bin"
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "lights_host_tool.mjs"), "render",
                        "lit_sample_scene", str(out)], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    want = lb.load_array("lit_sample_scene", "rgba8")
    got = np.frombuffer(out.read_bytes(), dtype=np.uint8).reshape(want.shape)
    assert np.array_equal(got, want)


def test_cli_lights_flag_reproduces_the_fixture(gpu, tmp_path):
    """rt_render_cli --lights (the C++ JSON loader's rt_json_scene_desc_lit) on sample_scene.json: the reference's
    lit RGBA8 frame; without the flag, the unlit frame the CLI always rendered."""
    cli = os.path.join(ROOT, "blenderraytracer_amd", "lib", "rt_render_cli")
    assert os.path.exists(cli), "rt_render_cli missing on the GPU box"
    c = lb.manifest()["cases"]["lit_sample_scene"]
    args = [cli, os.path.join(ROOT, "scenes", c["scene"]), "--width", str(c["width"]), "--height", str(c["height"]),
            "--spp", str(c["settings_in"]["samples"]), "--depth", str(c["settings_in"]["maxBounces"]), "--seed", str(c["seed"])]
    imgs = []
    for extra in (["--lights"], []):
        out = tmp_path / f"img{len(extra)}.pam"
        r = subprocess.run(args + ["--out", str(out)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        _, _, body = out.read_bytes().partition(b"ENDHDR\n")
        imgs.append(np.frombuffer(body, dtype=np.uint8).reshape(c["height"], c["width"], 4))
    assert np.array_equal(imgs[0], lb.load_array("lit_sample_scene", "rgba8"))
    rt, _ = lb.tracer_for("lit_sample_scene", direct_lighting=False)
    assert np.array_equal(imgs[1], rt.render()["rgba8"])
    rt.close()
