"""The per-pixel error estimate and the noise-threshold stop on the GPU (include/rt_hip.h rt_scene_set_error_estimate
.. rt_error_estimate_device): the device's arithmetic against the rational reference of tests/error_ref.py over
exactly the samples the render committed, and everything else a render produces unchanged."""
import ctypes as C
import math

import numpy as np
import pytest

import error_ref as ref
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json

pytestmark = pytest.mark.gpu

W, H = 24, 20            # 3 x 3 tiles, the right column and the bottom row ragged
SPP, BATCH = 22, 8       # batches of 8, 8 and 6 samples


def tracer(scene, precision=capi.RT_PREC_F64, spp=SPP, estimate=True, seed=77):
    rt = GpuRayTracer(W, H, seed=seed, precision=precision, error_estimate=estimate)
    assert rt.load_from_json(load_scene_json(scene))
    rt.update_render_settings({"maxBounces": 5, "samples": spp})
    return rt


_samples = {}


def sample_radiance(scene, precision, spp=SPP):
    """Every sample's radiance (spp, H, W, 3), exactly: sample i rendered alone as [i, i + 1) (one batch, the estimate
    off), its value read back as the checkpoint's sums (0 + x is x).  Computed once per scene and precision."""
    key = (scene, precision, spp)
    if key not in _samples:
        rt = tracer(scene, precision, spp, estimate=False)
        lib, h = capi.load_library(), rt.scene_handle()
        out = np.zeros((spp, H, W, 3))
        done = C.c_int32()
        for i in range(spp):
            st = rt.settings(sample_range=(i, i + 1))
            capi.check(lib.rt_render(h, C.byref(st), None, capi.PROGRESS_FN(0), None, None))
            capi.check(lib.rt_render_checkpoint(h, out[i].ctypes.data_as(C.POINTER(C.c_double)), out[i].size, C.byref(done)))
            assert done.value == i + 1
        rt.close()
        assert np.all(out >= 0.0)                      # the bound's chunk term assumes non-negative samples
        _samples[key] = out
    return _samples[key]


def group_sizes(done, batch, chunk):
    """The chunk partials of `done` samples in batches of `batch`, each batch in chunks of `chunk` (its last short)."""
    sizes = []
    for b in range(0, done, batch):
        ns = min(batch, done - b)
        sizes += [min(chunk, ns - c) for c in range(0, ns, chunk)]
    return sizes


def check_against_reference(rt, samples, done, batch=BATCH):
    """var_mean, rel_error and the frame's figures of rt's last render against the reference over samples [0, done)."""
    st = rt.error_stats()
    sums, ck = rt.checkpoint()
    assert ck == done and st["samples"] == done and st["pixels"] == W * H
    sizes = group_sizes(done, batch, st["chunk_samples"])
    assert len(sizes) == st["groups"], (sizes, st)
    var, rel = rt.error_estimate()
    n_max = max(sizes)
    # the device's sum is the samples' sum up to the additions' rounding (it is taken as given below)
    assert np.all(np.abs(sums - samples[:done].sum(axis=0)) <= 2 * done * ref.U * np.abs(sums))
    rvar, scale, vp, mp, bad = ref.reference(samples[:done], sizes, sums, per_sample=True)
    assert not bad.any() and st["nonfinite_pixels"] == 0
    tol = ref.var_tolerance(scale, len(sizes), n_max)
    ratio = np.max(np.abs(var - rvar) / np.where(tol > 0, tol, 1.0))
    print(f"groups {sizes}: max |var - ref| / bound {ratio:.3f}")
    assert np.all(np.abs(var - rvar) <= tol)
    assert np.all(var >= 0.0)
    e, etol = ref.rel_reference(vp, mp, tol, bad)
    assert np.all(np.abs(rel.astype(np.float64) - e) <= etol + 2.0 ** -24 * e)
    fe, ftol = ref.frame_reference(e, etol, bad)
    print(f"frame_error {st['frame_error']:.6g} (reference {fe:.6g}, bound {ftol:.3g}), max_error {st['max_error']:.6g}")
    assert abs(st["frame_error"] - fe) <= ftol
    # max_error is the e_p of the pixel with the largest one: the same value rel_error holds there, rounded once
    y, x = np.unravel_index(np.argmax(rel), rel.shape)
    assert np.float32(st["max_error"]) == rel[y, x]
    assert abs(st["max_error"] - e[y, x]) <= etol[y, x]
    return var, rel, st


@pytest.mark.parametrize("precision", [capi.RT_PREC_F64, capi.RT_PREC_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("scene", ["cornell.json", "rtow.json"])
def test_device_arithmetic_matches_rational_reference(gpu, scene, precision):
    samples = sample_radiance(scene, precision)
    rt = tracer(scene, precision)
    if scene == "rtow.json":
        assert gpu.rt_scene_walk(rt.scene_handle(), precision, capi.RT_ACCEL_AUTO) == 2      # the grid / LDS kernel
    rt.render(batch_samples=BATCH)
    check_against_reference(rt, samples, SPP)
    # one batch: the pool's own reduce is followed by the moments, too
    rt.render()
    st = rt.error_stats()
    assert st["samples"] == SPP and st["groups"] == math.ceil(SPP / st["chunk_samples"]) >= 2
    check_against_reference(rt, samples, SPP, batch=SPP)
    rt.close()


@pytest.mark.parametrize("kw", [dict(), dict(batch_samples=BATCH), dict(batch_samples=BATCH, preview=True),
                                dict(batch_samples=BATCH, devices=[0, 0]), dict(spp=4)],
                         ids=["one_batch", "three_batches", "preview", "two_device_states", "one_chunk"])
def test_nothing_else_moves(gpu, kw):
    kw = dict(kw)
    want = ("mean", "segments", "draws") + (("preview",) if kw.pop("preview", False) else ())
    spp = kw.pop("spp", SPP)
    res = []
    for on in (False, True):
        rt = tracer("cornell.json", spp=spp, estimate=on)
        res.append(rt.render(want=want, **kw))
        if on and spp == 4:
            # one batch of one chunk: the chunk goes through the partials while the estimate is on (one group: its
            # moment is kept, an estimate needs two)
            st = rt.error_stats()
            assert (st["groups"], st["samples"], st["chunk_samples"]) == (1, 4, 4) and math.isnan(st["frame_error"])
            with pytest.raises(RuntimeError, match="no estimate"):
                rt.error_estimate()
        elif on:
            assert rt.error_stats()["groups"] >= 2
            rt.error_estimate()
        else:
            assert rt.error_stats()["groups"] == 0
            with pytest.raises(RuntimeError, match="no estimate"):
                rt.error_estimate()
        rt.close()
    for k in ("mean", "post", "rgba8", "segments", "draws"):
        assert np.array_equal(res[0][k], res[1][k]), k


def test_cancel_covers_the_committed_batches(gpu):
    samples = sample_radiance("cornell.json", capi.RT_PREC_F64)
    rt = tracer("cornell.json")
    calls = []
    with pytest.raises(RuntimeError, match="CANCELLED"):
        rt.render(batch_samples=BATCH, on_progress=lambda f: calls.append(f) or len(calls) >= 2)
    done = rt.checkpoint()[1]
    assert done == 2 * BATCH
    assert rt.error_stats()["samples"] == done
    check_against_reference(rt, samples, done)
    rt.close()


def test_resume(gpu):
    rt = tracer("cornell.json")
    full_mean = rt.render(want=("mean",), batch_samples=BATCH)["mean"]
    full_var, full_rel = rt.error_estimate()
    full_stats = rt.error_stats()
    calls = []
    with pytest.raises(RuntimeError, match="CANCELLED"):
        rt.render(batch_samples=BATCH, on_progress=lambda f: calls.append(f) or True)
    sums, done = rt.checkpoint()
    assert 0 < done < SPP
    # from the sums on the device: the moments continue
    res = rt.render(want=("mean",), batch_samples=BATCH, resume=(None, done))
    assert np.array_equal(res["mean"], full_mean)
    var, rel = rt.error_estimate()
    assert np.array_equal(var, full_var) and np.array_equal(rel, full_rel)
    assert rt.error_stats() == full_stats
    # from host sums: the moments of those samples are not there
    res = rt.render(want=("mean",), batch_samples=BATCH, resume=(sums, done))
    assert np.array_equal(res["mean"], full_mean)
    assert rt.error_stats()["groups"] == 0
    lib = capi.load_library()
    out = capi.ErrorOutput()
    assert lib.rt_error_estimate(rt.scene_handle(), C.byref(out)) == -1 and "no estimate" in lib.rt_last_error().decode()
    rt.close()


def test_threshold_stops_at_the_first_batch_under_it(gpu):
    spp, batch, nb = 32, 4, 8
    rt = tracer("cornell.json", spp=spp)
    errs = []
    full = rt.render(want=("mean",), batch_samples=batch, on_progress=lambda f: errs.append(rt.error_stats()["frame_error"]) and False)
    errs = errs[:nb - 1] + [rt.error_stats()["frame_error"]]          # (the last call, at 1.0, is the host's own)
    assert len(errs) == nb and rt.error_stats()["converged"] == 0
    print("frame_error after every batch:", " ".join(f"{e:.5f}" for e in errs))
    assert all(math.isfinite(e) and e > 0 for e in errs[1:])           # one chunk partial after batch 1: no estimate yet

    def first_under(thr, min_samples=0):
        return next((k + 1 for k, e in enumerate(errs) if e <= thr and (k + 1) * batch >= min_samples), None)
    thr = errs[nb // 2 - 1]
    k = first_under(thr)
    assert k is not None and k < nb

    # the checkpoint of a render cancelled after batch k, with its frame
    calls = []
    with pytest.raises(RuntimeError, match="CANCELLED"):
        rt.render(want=("preview",), batch_samples=batch, on_progress=lambda f: calls.append(f) or len(calls) >= k)
    ck_frame = rt.image_data.copy()
    ck_sums, ck_done = rt.checkpoint()
    assert ck_done == k * batch

    def stopped(thr, min_samples=0):
        res = rt.render(want=("mean",), batch_samples=batch, noise_threshold=thr, min_samples=min_samples)
        return res, rt.error_stats(), rt.checkpoint()[1]
    res, st, done = stopped(thr)
    assert st["converged"] == 1 and st["samples"] == k * batch == done
    assert st["frame_error"] == errs[k - 1]
    assert rt.last_stats.samples == W * H * k * batch
    assert np.array_equal(res["mean"], ck_sums / float(k * batch))
    assert np.array_equal(res["rgba8"], ck_frame)
    # the same batch again
    res2, st2, done2 = stopped(thr)
    assert done2 == done and st2 == st and np.array_equal(res2["mean"], res["mean"])
    # a host may resume the stopped render to the full count
    assert np.array_equal(rt.render(want=("mean",), batch_samples=batch, resume=(None, done))["mean"], full["mean"])
    # min_samples beyond that batch: the first qualifying batch after it (or the whole render)
    k2 = first_under(thr, k * batch + 1)
    _, st, done = stopped(thr, k * batch + 1)
    assert done == (k2 or nb) * batch == st["samples"]
    assert st["converged"] == (1 if k2 else 0)
    # no threshold: the plain render
    res, st, done = stopped(0.0)
    assert done == spp and st["converged"] == 0 and np.array_equal(res["mean"], full["mean"])
    rt.close()


def test_unsupported_modes(gpu):
    plain = tracer("cornell.json", estimate=False)
    plain.sum_order = capi.RT_SUM_SAMPLE_ORDER
    want = plain.render(want=("mean",))["mean"]
    plain.close()
    rt = tracer("cornell.json")
    rt.sum_order = capi.RT_SUM_SAMPLE_ORDER
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID.*RT_SUM_SAMPLE_ORDER"):
        rt.render(want=("mean",))
    rt.error_estimate_on = False
    assert np.array_equal(rt.render(want=("mean",))["mean"], want)
    # a threshold needs the estimate
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID"):
        rt.render(noise_threshold=0.1)
    rt.sum_order = capi.RT_SUM_POOL
    rt.error_estimate_on = True
    rt.max_bounces = -1                                                # max_depth <= 0: nothing is traced
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID.*max_depth"):
        rt.render()
    rt.close()
