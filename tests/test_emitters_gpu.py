"""Emitter sampling (next-event estimation with MIS) on the GPU: the device against the CPU
build of the same code bit for bit (renders and rt_emitter_samples), the estimator's expectation against the
plain render's in both precisions, toggling, progressive renders and resume, the Node drop-in and the CLI.
Every render is 32 x 32.  The CPU side is tests/test_emitters.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import neecheck_binding as nb
from blenderraytracer_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = ("mean", "segments", "draws")


# ---- 1: bit-identity with the CPU build ----------------------------------------------------------------------------
@pytest.mark.parametrize("scene,direct", [("cornell", False), ("nee_mixed", False), ("nee_mixed", True)],
                         ids=["cornell", "nee_mixed", "nee_mixed_lit"])
def test_f64_renders_equal_the_cpu_build(gpu, scene, direct):
    """Binary64 at 16 spp: in sample order the means, segments and draws are the CPU build's bits in World order
    and through the trees; the two walks agree bit for bit in both summation orders, counting on and off; pool
    order stays within the summation-order bound (1e-12 relative) of sample order; rt_scene_walk reports the walk."""
    out = {}
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt = nb.tracer(scene, accel=accel, emitter_sampling=True, direct_lighting=direct)
        assert rt.emitter_count() == len(nb.emitters(rt.packed())) > 0
        assert gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, accel) == (0 if accel == capi.RT_ACCEL_BRUTE else 1)
        pool = rt.render(want=WANT)
        uncounted = rt.render(want=("mean",))
        assert np.array_equal(nb.bits(pool["mean"]), nb.bits(uncounted["mean"]))
        rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
        order = rt.render(want=WANT)
        assert np.array_equal(nb.bits(order["mean"]), nb.bits(rt.render(want=("mean",))["mean"]))
        host = nb.host_render(rt.packed(), rt.settings(), True)
        same = nb.bits(order["mean"]) == nb.bits(host["mean"])
        print(f"{scene} accel {accel}: {same.mean():.4f} of channels bit-identical to the CPU build")
        assert same.all()
        assert np.array_equal(order["segments"], host["segments"]) and np.array_equal(order["draws"], host["draws"])
        assert np.array_equal(pool["segments"], host["segments"]) and np.array_equal(pool["draws"], host["draws"])
        rel = float(np.max(np.abs(pool["mean"] - order["mean"]) / np.maximum(np.abs(order["mean"]), 1e-300)))
        print(f"{scene} accel {accel}: pool order against sample order, max relative difference {rel:.2e}")
        assert rel <= 1e-12
        out[accel] = (pool, order)
        rt.close()
    for a, b in zip(out[capi.RT_ACCEL_BRUTE], out[capi.RT_ACCEL_BVH]):
        assert np.array_equal(nb.bits(a["mean"]), nb.bits(b["mean"]))
        assert np.array_equal(a["rgba8"], b["rgba8"])


# ---- 2: the device query ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", nb.SCENES)
def test_rt_emitter_samples_equals_the_cpu_build(gpu, scene):
    """rt_emitter_samples in binary64, both walks, on the CPU test's 10,000 queries: the emitter, omega, p_l, t_e and
    the verdict are the CPU build's, bit for bit.  Binary32 runs the same query and chooses the same emitters."""
    pts, keys = nb.query_set(scene)
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt = nb.tracer(scene, accel=accel, emitter_sampling=True)
        got = rt.emitter_samples(pts, keys)
        want = nb.host_samples(rt.packed(), accel, pts, keys)
        assert np.array_equal(got["emitter"], want["emitter"]) and np.array_equal(got["visible"], want["visible"])
        for k in ("omega", "p_l", "t_e"):
            same = nb.bits(got[k]) == nb.bits(want[k])
            assert same.all(), (scene, accel, k, float(same.mean()))
        assert got["visible"].sum() > 500
        rt.close()
    rt = nb.tracer(scene, precision=capi.RT_PREC_F32, emitter_sampling=True)
    g32 = rt.emitter_samples(pts, keys)
    assert np.array_equal(g32["emitter"], want["emitter"])
    both = (g32["p_l"] > 0) & (want["p_l"] > 0)
    assert both.mean() > 0.9 and np.abs(g32["omega"][both] - want["omega"][both]).max() < 1e-3
    rt.close()
    off = nb.tracer(scene)
    assert off.emitter_count() == 0
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID"):
        off.emitter_samples(pts[:4], keys[:4])
    off.close()


# ---- 3: same expectation as the plain render -------------------------------------------------------------------------
SEEDS = 16
SPP = 1024
_renders = {}


def _blocks(scene, on, first_seed, precision):
    key = (scene, on, first_seed, precision)
    if key not in _renders:
        out = []
        for s in range(SEEDS):
            rt = nb.tracer(scene, seed=first_seed + s, samples=SPP, precision=precision, emitter_sampling=on)
            out.append(nb.block_means(rt.render(want=("mean",))["mean"]))
            rt.close()
        _renders[key] = np.array(out)
    return _renders[key]


@pytest.mark.parametrize("precision", [capi.RT_PREC_F64, capi.RT_PREC_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("scene", nb.SCENES)
def test_same_expectation_as_the_plain_render(gpu, scene, precision):
    """The CPU test's conditions with 16 seeds x 1024 spp a side: emitter sampling in binary64 and in binary32, each
    against the binary64 plain render"""
    t, blocks = nb.welch(_blocks(scene, True, 101, precision), _blocks(scene, False, 1, capi.RT_PREC_F64))
    mx, share, mt, bound = nb.expectation_conditions(t, blocks)
    print(f"{scene} precision {precision}: max |t| {mx:.2f}, |t| > 3 in {100 * share:.2f} %, |mean t| {mt:.3f} (bound {bound:.3f})")
    assert mx < 6
    assert share <= 0.02
    assert mt <= bound


# ---- 4: toggling, progressive renders and resume ---------------------------------------------------------------------
def test_toggling_rerenders_and_off_is_the_plain_render(gpu):
    plain_rt = nb.tracer("nee_mixed")
    plain = plain_rt.render(want=WANT)
    plain_rt.close()
    rt = nb.tracer("nee_mixed")
    first = rt.render(want=WANT)
    assert np.array_equal(nb.bits(first["mean"]), nb.bits(plain["mean"]))
    rt.update_render_settings({"samples": 16, "maxBounces": 5, "emitterSampling": True})
    on = rt.render(want=WANT)
    assert rt.emitter_count() == 7
    assert not np.array_equal(on["mean"], plain["mean"])
    assert np.array_equal(on["segments"], plain["segments"]) and np.array_equal(on["draws"], plain["draws"])
    rt.update_render_settings({"samples": 16, "maxBounces": 5, "emitterSampling": False})
    off = rt.render(want=WANT)
    assert rt.emitter_count() == 0
    assert np.array_equal(nb.bits(off["mean"]), nb.bits(plain["mean"])) and np.array_equal(off["rgba8"], plain["rgba8"])
    # the setter itself, on a live scene: on, then off again — the plain bits once more
    h = rt.scene_handle()
    capi.check(gpu.rt_scene_set_emitter_sampling(h, 1), gpu)
    assert rt.emitter_count() == 7
    assert np.array_equal(nb.bits(rt.render(want=WANT)["mean"]), nb.bits(on["mean"]))
    capi.check(gpu.rt_scene_set_emitter_sampling(h, 0), gpu)
    assert np.array_equal(nb.bits(rt.render(want=WANT)["mean"]), nb.bits(plain["mean"]))
    rt.close()


def test_scene_without_emitters_keeps_its_kernels(gpu):
    """RTOW lists nothing: with the setting on it still walks the grid and renders the same bits"""
    import golden_cases as gc
    rt, c = gc.tracer_for("cfg3_rtow_crop")
    a = rt.render(crop=c["crop"], want=WANT)
    rt.update_render_settings({**c["settings_in"], "emitterSampling": True})
    assert rt.emitter_count() == 0
    assert gpu.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, capi.RT_ACCEL_AUTO) == 2
    b = rt.render(crop=c["crop"], want=WANT)
    assert np.array_equal(nb.bits(a["mean"]), nb.bits(b["mean"]))
    rt.close()


def test_progressive_and_resumed_renders_equal_the_one_batch_render(gpu):
    """With emitter sampling on: a render in batches equals the one-batch render bit for bit in sample order, also
    across a cancel, checkpoint and resume; the pool's batched and fused renders keep segments, draws and RGBA8
    within the summation-order bound; the guided filter runs on top."""
    rt = nb.tracer("nee_mixed", emitter_sampling=True)
    one = rt.render(want=WANT)
    seen = []
    batched = rt.render(want=WANT, batch_samples=4, on_progress=lambda f: seen.append(f) and False)
    assert len(seen) >= 4
    assert np.array_equal(one["segments"], batched["segments"]) and np.array_equal(one["draws"], batched["draws"])
    assert np.array_equal(one["rgba8"], batched["rgba8"])
    assert np.max(np.abs(one["mean"] - batched["mean"]) / np.maximum(np.abs(one["mean"]), 1e-300)) <= 1e-12
    fused = rt.render(want=WANT, batch_samples=4)            # no progress callback: the batches of one launch
    assert np.array_equal(one["rgba8"], fused["rgba8"])
    assert np.max(np.abs(one["mean"] - fused["mean"]) / np.maximum(np.abs(one["mean"]), 1e-300)) <= 1e-12
    rt.update_render_settings({"samples": 16, "maxBounces": 5, "guidedDenoise": True})
    filtered = rt.render(want=("mean",))
    assert np.isfinite(filtered["mean"]).all() and not np.array_equal(filtered["mean"], one["mean"])
    rt.update_render_settings({"samples": 16, "maxBounces": 5, "guidedDenoise": False})
    rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
    full = rt.render(want=("mean",))
    four = rt.render(want=("mean",), batch_samples=4)
    assert np.array_equal(nb.bits(four["mean"]), nb.bits(full["mean"]))
    with pytest.raises(RuntimeError, match="CANCELLED"):
        rt.render(batch_samples=1, on_progress=lambda f: True)
    sums, done = rt.checkpoint()
    rt.close()
    assert 0 < done < 16
    rt2 = nb.tracer("nee_mixed", emitter_sampling=True)
    rt2.sum_order = capi.RT_SUM_SAMPLE_ORDER
    res = rt2.render(want=("mean",), resume=(sums, done), batch_samples=4)
    assert np.array_equal(nb.bits(res["mean"]), nb.bits(full["mean"]))
    rt2.close()


def test_two_shards_on_one_device_equal_the_single_render(gpu):
    """The multi-device split with emitter sampling on (both shards on device 0: a replica with its own records)"""
    rt = nb.tracer("nee_mixed", emitter_sampling=True)
    one = rt.render(want=WANT, batch_samples=4)
    two = rt.render(want=WANT, batch_samples=4, devices=[0, 0])
    assert np.array_equal(one["segments"], two["segments"]) and np.array_equal(one["draws"], two["draws"])
    assert np.max(np.abs(one["mean"] - two["mean"]) / np.maximum(np.abs(one["mean"]), 1e-300)) <= 1e-12
    rt.close()


# ---- 5: Node and the CLI ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_drop_in_matches_the_python_host(gpu, tmp_path):
    """GpuRayTracer (Node, N-API) with updateRenderSettings({emitterSampling: true}): the Python host's RGBA8"""
    assert os.path.exists(os.path.join(ROOT, "blenderraytracer_amd", "lib", "rt_napi.node")), "rt_napi.node missing on the GPU box"
    out = tmp_path / "rgba8.bin"
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "nee_host_tool.mjs"), "render",
                        "nee_mixed", "32", "32", "1", "16", "5", str(out)], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    rt = nb.tracer("nee_mixed", emitter_sampling=True, sum_order=capi.RT_SUM_SAMPLE_ORDER)
    want = rt.render()["rgba8"]
    plain_rt = nb.tracer("nee_mixed", sum_order=capi.RT_SUM_SAMPLE_ORDER)
    assert not np.array_equal(want, plain_rt.render()["rgba8"])
    got = np.frombuffer(out.read_bytes(), dtype=np.uint8).reshape(want.shape)
    assert np.array_equal(got, want)
    rt.close()
    plain_rt.close()


def test_cli_nee_flag_matches_the_python_host(gpu, tmp_path):
    """rt_render_cli --nee on nee_mixed.json: the Python host's RGBA8 with emitter sampling; without the flag, the
    plain frame; with --lights too, the Python host's frame with both."""
    cli = os.path.join(ROOT, "blenderraytracer_amd", "lib", "rt_render_cli")
    assert os.path.exists(cli), "rt_render_cli missing on the GPU box"
    args = [cli, os.path.join(ROOT, "scenes", "nee_mixed.json"), "--width", "32", "--height", "32", "--spp", "16",
            "--depth", "5", "--seed", "1"]
    imgs = {}
    for name, extra in (("nee", ["--nee"]), ("plain", []), ("both", ["--nee", "--lights"])):
        out = tmp_path / f"{name}.pam"
        r = subprocess.run(args + ["--out", str(out)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        _, _, body = out.read_bytes().partition(b"ENDHDR\n")
        imgs[name] = np.frombuffer(body, dtype=np.uint8).reshape(32, 32, 4)
    for name, kw in (("nee", {"emitter_sampling": True}), ("plain", {}),
                     ("both", {"emitter_sampling": True, "direct_lighting": True})):
        rt = nb.tracer("nee_mixed", **kw)
        assert np.array_equal(imgs[name], rt.render()["rgba8"]), name
        rt.close()
    assert not np.array_equal(imgs["nee"], imgs["plain"]) and not np.array_equal(imgs["nee"], imgs["both"])
