"""The epilogue kernels (finalize_kernel, preview_kernel, reduce_preview_kernel, the gamma-table kernels
and denoise_kernel, csrc/pt_trace.hip) and epilogue() / gamma_table() (csrc/rt_capi.cpp) against the
independent reference of tests/epilogue_ref.py and the CPU oracle, through rt_finalize_device on synthetic
device sums.  Only test_running_frames_under_a_non_default_epilogue traces rays.  The oracle and the
reference themselves are compared in tests/test_epilogue.py, which needs no GPU."""
import numpy as np
import pytest

import epilogue_ref as er
from blenderraytracer_amd.renderer import GpuRayTracer
from oracle import binding
from test_gpu_parity import _render_in_child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(gpu):
    """Any scene: rt_finalize_device takes the frame size and the epilogue from the settings."""
    rt = GpuRayTracer(8, 8, seed=1)
    yield rt.scene_handle()
    rt.close()


def _oracle(sums, st):
    mean, post, rgba = binding.finalize(sums, st)
    with np.errstate(over="ignore"):
        return mean, post.astype(np.float32), rgba


def _assert_device_equals_oracle(dev, mean, post32, rgba, label):
    assert er.same_bits(dev["mean"], mean).all(), label
    assert er.same_bits(dev["post"][:, :3], post32).all(), label            # the NaNs in the same places
    assert (dev["post"][:, 3] == 1.0).all(), label
    assert np.array_equal(dev["rgba8"], rgba), label                         # alpha 255 included


@pytest.mark.parametrize("tone", er.TONE_MAPS)
@pytest.mark.parametrize("exposure,gamma,samples", er.GRID, ids=er.GRID_IDS)
def test_finalize_kernel_against_numpy_oracle_and_mpmath(scene, tone, exposure, gamma, samples):
    """finalize_kernel's mean equals numpy's bit for bit; its Float32 frame and bytes equal orc_finalize's
    exactly and meet the mpmath criteria of tests/test_epilogue.py on their own (independent of the oracle's
    pow).  Then frames of 1, 63, 64 and 65 pixels (the last partial wave), cut from the end of the same
    sums, where the special values are."""
    sums, n_near = er.input_sums(tone, exposure, gamma, samples)
    n = sums.size // 3
    st = er.settings(n, tone, exposure, gamma, samples)
    dev = er.finalize_device(scene, st, sums, mean=True, post=True)
    ref_mean, ref_tm = er.stage_a(tone, exposure, samples, sums)
    assert er.same_bits(dev["mean"].ravel(), ref_mean).all()
    mean, post32, rgba = _oracle(sums, st)
    _assert_device_equals_oracle(dev, mean, post32, rgba, "full")
    er.check_post_and_bytes(f"device {tone} {exposure:g} {gamma:g} {samples}", gamma, ref_tm, n_near,
                            dev["post"][:, :3].ravel(), dev["rgba8"][:, :3].ravel())
    for m in (1, 63, 64, 65):
        part = er.finalize_device(scene, er.settings(m, tone, exposure, gamma, samples), sums[-3 * m:], mean=True, post=True)
        _assert_device_equals_oracle(part, mean[-m:], post32[-m:], rgba[-m:], m)


@pytest.mark.parametrize("tone", er.TONE_MAPS)
@pytest.mark.parametrize("exposure,gamma,samples", er.GRID, ids=er.GRID_IDS)
def test_preview_kernel_bytes_equal_finalize_kernel(scene, tone, exposure, gamma, samples):
    """An RGBA8-only call (preview_kernel: its own copy of the tone maps, then the count of gamma thresholds)
    against a call that also asks for the Float32 frame (finalize_kernel): identical bytes on every one of
    the +-3000 ulps around every threshold, mapped back through the inverse tone map, exposure and sample
    count, plus the random and special values."""
    sums, n_near = er.input_sums(tone, exposure, gamma, samples, steps=er.DENSE_STEPS)
    st = er.settings(sums.size // 3, tone, exposure, gamma, samples)
    fast = er.finalize_device(scene, st, sums)["rgba8"]
    exact = er.finalize_device(scene, st, sums, post=True)["rgba8"]
    assert np.array_equal(fast, exact), int(np.count_nonzero(fast != exact))
    if exposure != 0:
        assert len(np.unique(exact[:, :3].ravel()[:n_near])) == 256          # every byte value occurs
    else:
        assert not exact[:, :3].any()


def _stride_sums(tone, exposure, gamma, samples):
    """3000 values (1000 pixels) of the tier-1 set: every 24th value and the last 100 (the specials)."""
    sums, _ = er.input_sums(tone, exposure, gamma, samples)
    return np.concatenate([sums[:-100:24][:2900], sums[-100:]])


_STRIDE_SCRIPT = r'''
import os, sys, numpy as np
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import torch  # noqa: F401  (HIP runtime first)
import epilogue_ref as er
from blenderraytracer_amd.renderer import GpuRayTracer
from test_epilogue_gpu import _stride_sums
rt = GpuRayTracer(8, 8, seed=1)
scene = rt.scene_handle()
out = {}
for tone in er.TONE_MAPS:
    for k, (exposure, gamma, samples) in enumerate(er.GRID):
        sums = _stride_sums(tone, exposure, gamma, samples)
        st = er.settings(1000, tone, exposure, gamma, samples)
        out[f"{tone}.{k}.fast"] = er.finalize_device(scene, st, sums)["rgba8"]
        out[f"{tone}.{k}.exact"] = er.finalize_device(scene, st, sums, post=True)["rgba8"]
rt.close()
np.savez(sys.argv[2], **out)
'''


def test_preview_kernel_grid_stride(gpu, tmp_path):
    """RT_PREVIEW_WGS=3 (read once per process, hence the child): 1000 pixels on 3 workgroups of 64 threads,
    which is 5 full strides of 192 and a partial one.  The bytes equal finalize_kernel's and the oracle's."""
    got = _render_in_child(_STRIDE_SCRIPT, tmp_path / "stride.npz", RT_PREVIEW_WGS="3")
    for tone in er.TONE_MAPS:
        for k, (exposure, gamma, samples) in enumerate(er.GRID):
            rgba = binding.finalize(_stride_sums(tone, exposure, gamma, samples),
                                    er.settings(1000, tone, exposure, gamma, samples))[2]
            assert np.array_equal(got[f"{tone}.{k}.exact"], rgba), (tone, k)
            assert np.array_equal(got[f"{tone}.{k}.fast"], rgba), (tone, k)


def test_gamma_table_eviction(gpu):
    """A scene keeps 8 gamma tables (kGammaSlots, rt_capi.cpp).  Ten distinct gammas one after the other evict
    the first two, which are then built again (evicting the third and fourth); the last call uses a table
    that stayed resident.  Every RGBA8-only call gives the exact path's bytes for its own gamma."""
    rt = GpuRayTracer(8, 8, seed=2)
    scene = rt.scene_handle()
    gammas = [float(g) for g in np.linspace(0.25, 4.0, 10)]
    for call, gamma in enumerate(gammas + gammas[:2] + gammas[-1:]):
        sums, _ = er.input_sums("linear", 1.0, gamma, 1)
        st = er.settings(sums.size // 3, "linear", 1.0, gamma, 1)
        fast = er.finalize_device(scene, st, sums)["rgba8"]
        exact = er.finalize_device(scene, st, sums, post=True)["rgba8"]       # finalize_kernel: touches no table
        assert np.array_equal(fast, exact), (call, gamma)
        assert len(np.unique(exact[:, :3])) == 256, (call, gamma)
    rt.close()


_RUNNING_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401  (HIP runtime first)
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
def tracer(spp, tone, exposure, gamma):
    rt = GpuRayTracer(128, 72, seed=6)
    assert rt.load_from_json(load_scene_json("rtow.json"))
    rt.update_render_settings({"maxBounces": 5, "samples": spp, "toneMapping": tone, "exposure": exposure, "gamma": gamma})
    return rt
out = {}
for tone, exposure, gamma in (("aces", 1.7, 2.4), ("reinhard", 0.6, 2.2)):
    rt = tracer(8, tone, exposure, gamma)
    fr = []
    res = rt.render(want=("preview",), batch_samples=2, on_progress=lambda f: fr.append(f) and False)
    assert len(fr) >= 4 and fr[-1] == 1.0, fr
    out[f"{tone}.preview"], out[f"{tone}.final"] = res["preview"], res["rgba8"]
    rt.close()
    rt = tracer(6, tone, exposure, gamma)
    out[f"{tone}.six"] = rt.render(batch_samples=2)["rgba8"]
    rt.close()
np.savez(sys.argv[2], **out)
'''


def test_running_frames_under_a_non_default_epilogue(gpu, tmp_path):
    """Progressive renders of RTOW, 128x72, 8 samples in batches of 2, under (ACES, exposure 1.7, gamma 2.4)
    and (Reinhard, 0.6, 2.2): the running frame at the last progress call (6 of 8 samples, divided by 6)
    equals the RGBA8 frame of a render of exactly those 6 samples in the same batches, as
    test_progressive_preview_and_cancel asserts for the default epilogue.  Run with the default kernels,
    with RT_FUSED_PREVIEW=1 (reduce_preview_kernel, which no other test runs) and with RT_FUSED_BATCHES=0
    (a launch per batch): the three running frames are equal."""
    runs = {name: _render_in_child(_RUNNING_SCRIPT, tmp_path / f"{name}.npz", **env)
            for name, env in (("default", {}), ("fused_preview", {"RT_FUSED_PREVIEW": "1"}),
                              ("unfused_batches", {"RT_FUSED_BATCHES": "0"}))}
    for tone in ("aces", "reinhard"):
        for name, r in runs.items():
            assert np.array_equal(r[f"{tone}.preview"], r[f"{tone}.six"]), (tone, name)
            assert not np.array_equal(r[f"{tone}.preview"], r[f"{tone}.final"]), (tone, name)
            assert np.array_equal(r[f"{tone}.preview"], runs["default"][f"{tone}.preview"]), (tone, name)
    assert not np.array_equal(runs["default"]["aces.six"], runs["default"]["reinhard.six"])


@pytest.mark.parametrize("w,h", er.DENOISE_SHAPES)
def test_denoise_kernel_against_oracle_and_numpy(scene, w, h):
    """denoise_kernel on frames of width or height 1 to 3 (clamp-to-edge reads one pixel several times), on
    frames that end inside a 256-thread block (19x27 = 513: one thread in the last block) and on a row
    longer than a block, at strengths whose weights reach 1e-174, on random values, a checkerboard and a
    frame with a NaN, a +Inf and a negative-sum pixel.  The Float32 input is the frame of a first call
    without denoise (linear tone map, gamma 1); the denoised floats and bytes equal orc_denoise's and the
    numpy reference's of that frame bit for bit."""
    for name, frame in er.denoise_frames(w, h).items():
        first = er.finalize_device(scene, er.settings((w, h), "linear", 1.0, 1.0, 1), frame, post=True)["post"]
        first = first.reshape(h, w, 4)
        with np.errstate(invalid="ignore"):
            assert er.same_bits(first[..., :3], (np.maximum(0.0, frame) + 0.0).astype(np.float32)).all(), name
        for strength in er.DENOISE_STRENGTHS:
            st = er.settings((w, h), "linear", 1.0, 1.0, 1, denoise_strength=strength)
            dev = er.finalize_device(scene, st, frame, post=True)
            got, rgba = dev["post"].reshape(h, w, 4), dev["rgba8"].reshape(h, w, 4)
            ref = er.denoise_ref(first, np.array(list(st.denoise_weights)))
            o_post, o_rgba = binding.denoise(first[..., :3], st)
            assert er.same_bits(got, ref).all(), (name, strength)
            assert er.same_bits(got, o_post).all(), (name, strength)
            assert (got[..., 3] == 1.0).all() and (rgba[..., 3] == 255).all()                 # alpha is preserved
            assert np.array_equal(rgba[..., :3], er.bytes_of(ref[..., :3])), (name, strength)
            assert np.array_equal(rgba, o_rgba), (name, strength)
            if name == "nan_inf_negative":      # the NaN spreads to exactly its 3x3 neighbourhood: bytes 0 there
                spread = er.nan_neighbourhood(first)
                assert np.array_equal(np.isnan(got[..., :3]).all(axis=2), spread), strength
                assert np.array_equal(np.isnan(got[..., :3]).any(axis=2), spread), strength
                assert not rgba[..., :3][spread].any()
                assert spread.sum() == min(w, 3) * min(h, 3)                # the NaN is not on an edge of a larger frame
