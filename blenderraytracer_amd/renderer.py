"""GpuRayTracer — Python mirror of the reference's RayTracer surface (js/ray-tracer.js), rendering
through librt_hip.so.  The JS twin for Node lives in blenderraytracer_amd/js/gpu-ray-tracer.mjs.

Mirrored members: width/height, maxBounces/samples/gamma/exposure/toneMapping/antiAliasing/denoising
(defaults ray-tracer.js:23-33), load_from_json (:305-334), update_render_settings (:554-566),
update_background (:568-585), resize_canvas (:598-614), render(on_progress) (:166-281) -> image_data.
Randomness: Math.random is replaced by the keyed RNG; `seed` selects the stream.
"""
import ctypes as C

import numpy as np

from . import capi
from .jsmath import js_exp
from .scene import (PackedScene, default_scene, load_from_json, setup_camera, keyed_permutation,
                    keyed_texture_permutation, js_or, truthy)


def settings_struct(width, height, samples, max_bounces, anti_aliasing, tone_mapping, exposure, gamma, seed,
                    crop=None, precision=capi.RT_PREC_F64, sample_range=None, batch_samples=0, denoising=False,
                    denoise_strength=0.5, accel=capi.RT_ACCEL_AUTO, devices=None, sum_order=capi.RT_SUM_POOL):
    """rt_settings from RayTracer fields, resolving sampleCount (ray-tracer.js:201) and the string
    switches of getAntiAliasSample (:125-149) and toneMap (:151-161)."""
    s = capi.Settings()
    s.width, s.height = int(width), int(height)
    s.samples = 1 if anti_aliasing == "none" else int(samples)
    s.max_depth = int(max_bounces)
    s.aa_mode = {"stochastic": capi.RT_AA_STOCHASTIC, "supersampling": capi.RT_AA_SUPERSAMPLING}.get(
        anti_aliasing, capi.RT_AA_CENTER)
    s.tone_map = {"aces": capi.RT_TM_ACES, "linear": capi.RT_TM_LINEAR}.get(tone_mapping, capi.RT_TM_REINHARD)
    s.exposure, s.gamma = float(exposure), float(gamma)
    s.seed = int(seed) & 0xFFFFFFFF
    if sample_range is not None:
        s.sample_begin, s.sample_end = int(sample_range[0]), int(sample_range[1])
    if crop is not None:
        s.crop_x0, s.crop_y0, s.crop_w, s.crop_h = (int(v) for v in crop)
    s.precision = int(precision)
    s.batch_samples = int(batch_samples)
    s.accel = int(accel)
    s.sum_order = int(sum_order)
    if devices:                 # multi-GPU sample split (rt_settings.devices)
        if len(devices) > capi.RT_MAX_DEVICES:
            raise ValueError(f"at most {capi.RT_MAX_DEVICES} devices")
        s.device_count = len(devices)
        for k, d in enumerate(devices):
            s.devices[k] = int(d)
    if truthy(denoising):
        # post-processor.js:55: Math.exp(-(kx*kx + ky*ky) / (2 * strength * strength)) for kx^2+ky^2 = 1, 2
        st = float(denoise_strength)
        s.denoise = 1
        s.denoise_weights[:] = (js_exp(-1 / (2 * st * st)), js_exp(-2 / (2 * st * st)))   # V8's Math.exp (jsmath.py)
    return s


# the guided filter's defaults (DESIGN.md §4 "Guided filter": the sweep that chose the sigmas)
GUIDED_LEVELS = capi.RT_GUIDED_DEFAULT_LEVELS
GUIDED_SIGMAS = dict(capi.RT_GUIDED_DEFAULT_SIGMAS)
GUIDED_SIGMA_VARIANCE = capi.RT_GUIDED_DEFAULT_SIGMA_VARIANCE   # "Variance-guided filter": its own sweep


class GpuRayTracer:
    def __init__(self, width, height, seed=0, device=0, precision=capi.RT_PREC_F64, accel=capi.RT_ACCEL_AUTO,
                 sum_order=capi.RT_SUM_POOL, direct_lighting=False, emitter_sampling=False, error_estimate=False):
        self.width, self.height = int(width), int(height)
        self.direct_lighting = bool(direct_lighting)   # opt-in: render World.lights
        self.emitter_sampling = bool(emitter_sampling)  # opt-in: sample emissive geometry with MIS
        # opt-in: the per-pixel error estimate from the sample pool's chunk partials
        self.error_estimate_on = bool(error_estimate)
        self.seed = seed
        self.device = device
        self.precision = precision
        self.accel = accel
        self.sum_order = sum_order
        self.max_bounces, self.samples, self.gamma, self.exposure = 5, 4, 2.2, 1.0
        self.tone_mapping, self.anti_aliasing = "reinhard", "supersampling"
        self.denoising, self.denoise_strength = False, 0.5
        # the edge-aware guided filter over the linear mean (opt-in)
        self.guided_denoise, self.guided_levels = False, GUIDED_LEVELS
        self.guided_sigma_color, self.guided_sigma_albedo = GUIDED_SIGMAS["color"], GUIDED_SIGMAS["albedo"]
        self.guided_sigma_normal, self.guided_sigma_depth = GUIDED_SIGMAS["normal"], GUIDED_SIGMAS["depth"]
        # its variance-guided form (opt-in; needs guided_denoise and error_estimate=True)
        self.guided_variance, self.guided_sigma_variance = False, GUIDED_SIGMA_VARIANCE
        self.world, self.camera = default_scene(self.width, self.height, keyed_permutation(seed))
        self.image_data = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self.float_data = None
        self.last_stats = None
        self._scene = None
        self._packed = None
        self._dirty = True

    # ---- RayTracer API --------------------------------------------------------------------------
    def load_from_json(self, data):
        try:
            world, camera, dims = load_from_json(data, self.width, self.height, keyed_permutation(self.seed),
                                                 keyed_texture_permutation(self.seed))
        except Exception:   # ray-tracer.js:330-333: errors -> false
            return False
        self.world = world
        if camera is not None:
            self.camera = camera
        if dims is not None:
            self.resize_canvas(*dims)
        self._dirty = True
        return True

    def resize_canvas(self, width, height):
        self.width, self.height = int(width), int(height)
        self.image_data = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        if self.camera is not None:
            self.camera = setup_camera(self.camera, self.width, self.height)
        self._dirty = True

    def update_render_settings(self, params):
        g = params.get
        self.max_bounces = js_or(g("maxBounces"), 5)
        self.samples = js_or(g("samples"), 4)
        self.gamma = js_or(g("gamma"), 2.2)
        self.exposure = js_or(g("exposure"), 1.0)
        self.tone_mapping = js_or(g("toneMapping"), "reinhard")
        self.anti_aliasing = js_or(g("antiAliasing"), "supersampling")
        self.denoising = js_or(g("denoising"), False)
        self.denoise_strength = js_or(g("denoiseStrength"), 0.5)
        if "directLighting" in params and bool(truthy(g("directLighting"))) != self.direct_lighting:
            self.direct_lighting = not self.direct_lighting
            self._dirty = True                      # the lights are part of the scene on the device
        if "emitterSampling" in params and bool(truthy(g("emitterSampling"))) != self.emitter_sampling:
            self.emitter_sampling = not self.emitter_sampling
            self._dirty = True                      # ... and so is the emitter list
        # the guided filter's keys, read only when present: a dict without them leaves the filter as it was
        if "guidedDenoise" in params:
            self.guided_denoise = bool(truthy(g("guidedDenoise")))
        if "guidedLevels" in params:
            self.guided_levels = int(g("guidedLevels"))
        for key, attr in (("guidedSigmaColor", "guided_sigma_color"), ("guidedSigmaAlbedo", "guided_sigma_albedo"),
                          ("guidedSigmaNormal", "guided_sigma_normal"), ("guidedSigmaDepth", "guided_sigma_depth")):
            if key in params:
                setattr(self, attr, float(g(key)))
        if "guidedVariance" in params:
            self.guided_variance = bool(truthy(g("guidedVariance")))
        if "guidedSigmaVariance" in params:
            self.guided_sigma_variance = float(g("guidedSigmaVariance"))

    def update_background(self, type, intensity=1.0):
        self.world.sky_intensity = intensity
        self.world.background = {"solid": capi.RT_BG_SOLID, "hdri": capi.RT_BG_HDRI,
                                 "procedural_sky": capi.RT_BG_PROCEDURAL_SKY}.get(type, capi.RT_BG_GRADIENT)
        self.world.solid_color = (0.1, 0.1, 0.1)
        self._dirty = True

    # ---- packing / rendering --------------------------------------------------------------------
    def packed(self):
        if self._dirty or self._packed is None:
            self._packed = PackedScene(self.world, self.camera, lights=self.direct_lighting)
        return self._packed

    def settings(self, crop=None, sample_range=None, batch_samples=0, devices=None):
        return settings_struct(self.width, self.height, self.samples, self.max_bounces, self.anti_aliasing,
                               self.tone_mapping, self.exposure, self.gamma, self.seed, crop=crop,
                               precision=self.precision, sample_range=sample_range, batch_samples=batch_samples,
                               denoising=self.denoising, denoise_strength=self.denoise_strength, accel=self.accel,
                               devices=devices, sum_order=self.sum_order)

    def scene_handle(self):
        lib = capi.load_library()
        if self._dirty or self._scene is None:
            self.close()
            h = C.c_void_p()
            capi.check(lib.rt_scene_create(C.byref(self.packed().desc), self.device, C.byref(h)))
            self._scene = h
            if self.emitter_sampling:
                capi.check(lib.rt_scene_set_emitter_sampling(h, 1))
            self._dirty = False
        return self._scene

    def emitter_count(self):
        """Listed emitters of the scene on the device (rt_scene_emitter_count; 0 while emitter sampling is off)."""
        n = C.c_int32()
        capi.check(capi.load_library().rt_scene_emitter_count(self.scene_handle(), C.byref(n)))
        return n.value

    def emitter_samples(self, points, keys):
        """rt_emitter_samples: the emitter-sampling kernels' own sample at points (n x 6: hit point, facing normal)
        with the emitter streams' keys (n) -> dict of emitter (n), omega (n, 3), p_l, t_e (n), visible (n, bool)."""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 6)
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        n = len(points)
        assert keys.shape == (n,)
        res = {"emitter": np.zeros(n, dtype=np.int32), "omega": np.zeros((n, 3)), "p_l": np.zeros(n), "t_e": np.zeros(n),
               "visible": np.zeros(n, dtype=np.uint8)}
        dp = C.POINTER(C.c_double)
        capi.check(capi.load_library().rt_emitter_samples(
            self.scene_handle(), self.precision, self.accel, points.ctypes.data_as(dp),
            keys.ctypes.data_as(C.POINTER(C.c_uint32)), n, res["emitter"].ctypes.data_as(C.POINTER(C.c_int32)),
            res["omega"].ctypes.data_as(dp), res["p_l"].ctypes.data_as(dp), res["t_e"].ctypes.data_as(dp),
            res["visible"].ctypes.data_as(C.POINTER(C.c_uint8))))
        res["visible"] = res["visible"].astype(bool)
        return res

    def guided_params(self):
        """rt_guided_params of the current settings (None: the filter is off)."""
        if not self.guided_denoise:
            return None
        return capi.GuidedParams(int(self.guided_levels), 0, float(self.guided_sigma_color), float(self.guided_sigma_albedo),
                                 float(self.guided_sigma_normal), float(self.guided_sigma_depth))

    def _apply_guided(self, lib, scene):
        p = self.guided_params()
        capi.check(lib.rt_scene_set_guided(scene, None if p is None else C.byref(p)))
        # (without guided_denoise or GpuRayTracer(error_estimate=True) the render itself is refused: RT_ERR_INVALID)
        if self.guided_variance and not float(self.guided_sigma_variance) > 0.0:
            raise RuntimeError("RT_ERR_INVALID: guidedSigmaVariance must be > 0")
        capi.check(lib.rt_scene_set_guided_variance(scene, float(self.guided_sigma_variance) if self.guided_variance else 0.0))

    def filtered_variance(self):
        """The propagated variance (h, w, 3) float64 of the last variance-guided render of the full frame
        (rt_guided_filtered_variance); RuntimeError (RT_ERR_INVALID) when there is none."""
        var = np.zeros((self.height, self.width, 3), dtype=np.float64)
        capi.check(capi.load_library().rt_guided_filtered_variance(self.scene_handle(), var.ctypes.data_as(C.POINTER(C.c_double))))
        return var

    def render_aovs(self, crop=None):
        """The feature buffers of the primary hit (rt_aovs): albedo and normal (h, w, 3), depth (h, w) as float32,
        kind and index (h, w) as rt_closest_hits reports them.  One pinhole ray through every pixel centre; no
        random numbers, so the buffers are noise-free whatever the sample count."""
        lib = capi.load_library()
        scene = self.scene_handle()
        st = self.settings(crop=crop)
        cw, ch = st.crop_w or self.width, st.crop_h or self.height
        res = {"albedo": np.zeros((ch, cw, 3), dtype=np.float32), "normal": np.zeros((ch, cw, 3), dtype=np.float32),
               "depth": np.zeros((ch, cw), dtype=np.float32), "kind": np.zeros((ch, cw), dtype=np.int32),
               "index": np.zeros((ch, cw), dtype=np.int32)}
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        out = capi.AovOutput(res["albedo"].ctypes.data_as(fp), res["normal"].ctypes.data_as(fp),
                             res["depth"].ctypes.data_as(fp), res["kind"].ctypes.data_as(ip), res["index"].ctypes.data_as(ip))
        capi.check(lib.rt_aovs(scene, C.byref(st), C.byref(out)))
        return res

    def _apply_error_estimate(self, lib, scene, noise_threshold=0.0, min_samples=0):
        capi.check(lib.rt_scene_set_error_estimate(scene, 1 if self.error_estimate_on else 0))
        capi.check(lib.rt_scene_set_noise_threshold(scene, float(noise_threshold), int(min_samples)))

    def error_stats(self):
        """rt_error_stats_get as a dict: samples, groups, chunk_samples, converged, pixels, nonfinite_pixels,
        frame_error, max_error of the last committed batch (host read only: may be called inside on_progress)."""
        st = capi.ErrorStats()
        capi.check(capi.load_library().rt_error_stats_get(self.scene_handle(), C.byref(st)))
        return {k: getattr(st, k) for k, _ in capi.ErrorStats._fields_}

    def error_estimate(self, crop=None):
        """(var_mean (h, w, 3) float64, rel_error (h, w) float32) of the last render (rt_error_estimate): the estimated
        variance of every pixel's mean per channel and sqrt(sum var) / (sum mean + 0.03).  RuntimeError
        (RT_ERR_INVALID, "no estimate") without at least two chunk partials per pixel."""
        st = self.settings(crop=crop)
        cw, ch = st.crop_w or self.width, st.crop_h or self.height
        var = np.zeros((ch, cw, 3), dtype=np.float64)
        rel = np.zeros((ch, cw), dtype=np.float32)
        out = capi.ErrorOutput(var.ctypes.data_as(C.POINTER(C.c_double)), rel.ctypes.data_as(C.POINTER(C.c_float)))
        capi.check(capi.load_library().rt_error_estimate(self.scene_handle(), C.byref(out)))
        return var, rel

    def render(self, on_progress=None, crop=None, want=("rgba8",), batch_samples=0, resume=None, devices=None,
               noise_threshold=0.0, min_samples=0):
        """RayTracer.render: fills image_data (RGBA8) and float_data (post-gamma RGBA float).
        Returns a dict of the requested host arrays (mean, post, rgba8, segments, draws, preview, and the
        feature buffers albedo, normal, depth of render_aovs).
        resume: a checkpoint() result to continue from (rt_render_resume).
        devices: HIP ordinals to deal the sample batches to (multi-GPU; may repeat a device).
        "preview" in want (with batch_samples): when on_progress runs, image_data (full frame) and the
        returned "preview" array hold the frame of the samples done so far (rt_output.preview_rgba8); a
        cancel (on_progress returning True, or rt_cancel) leaves the frame of the checkpointed samples
        there and raises RuntimeError(RT_ERR_CANCELLED).
        noise_threshold, min_samples (GpuRayTracer(error_estimate=True), with batch_samples): stop at the first batch
        after which the frame's estimated error (error_stats()["frame_error"]) is at or under the threshold and at
        least min_samples samples are in; the result is the frame of the samples done (last_stats.samples,
        error_stats()), and checkpoint() may resume it.  resume = (None, done): from the sums still on the device."""
        lib = capi.load_library()
        scene = self.scene_handle()
        self._apply_guided(lib, scene)
        self._apply_error_estimate(lib, scene, noise_threshold, min_samples)
        st = self.settings(crop=crop, batch_samples=batch_samples, devices=devices)
        cw = st.crop_w or self.width
        ch = st.crop_h or self.height
        n = cw * ch
        res = {}
        out = capi.Output()
        if "mean" in want:
            res["mean"] = np.zeros((ch, cw, 3), dtype=np.float64)
            out.mean = res["mean"].ctypes.data_as(C.POINTER(C.c_double))
        res["post"] = np.zeros((ch, cw, 4), dtype=np.float32)
        out.post = res["post"].ctypes.data_as(C.POINTER(C.c_float))
        res["rgba8"] = np.zeros((ch, cw, 4), dtype=np.uint8)
        out.rgba8 = res["rgba8"].ctypes.data_as(C.POINTER(C.c_uint8))
        if "segments" in want:
            res["segments"] = np.zeros((ch, cw), dtype=np.uint32)
            out.segments = res["segments"].ctypes.data_as(C.POINTER(C.c_uint32))
        if "draws" in want:
            res["draws"] = np.zeros((ch, cw), dtype=np.uint32)
            out.draws = res["draws"].ctypes.data_as(C.POINTER(C.c_uint32))
        if "preview" in want:
            res["preview"] = np.zeros((ch, cw, 4), dtype=np.uint8)
            out.preview_rgba8 = res["preview"].ctypes.data_as(C.POINTER(C.c_uint8))
            if crop is None:                 # the running frame, as the reference's canvas between rows
                self.image_data = res["preview"]
        stats = capi.Stats()
        cb = capi.PROGRESS_FN(lambda f, u: int(bool(on_progress(f)) if on_progress else 0))
        if resume is None:
            rc = lib.rt_render(scene, C.byref(st), C.byref(out), cb, None, C.byref(stats))
        else:
            sums, done = resume
            if sums is not None:
                sums = np.ascontiguousarray(sums, dtype=np.float64)
                assert sums.size == 3 * n, "checkpoint of another frame size"
            rc = lib.rt_render_resume(scene, C.byref(st), None if sums is None else sums.ctypes.data_as(C.POINTER(C.c_double)),
                                      int(done), C.byref(out), cb, None, C.byref(stats))
        if rc == -4 and "preview" in want and crop is None:    # cancelled: the frame of the checkpoint stays
            self.image_data = res["preview"]
        capi.check(rc)
        self.last_stats = stats
        if crop is None:
            self.image_data = res["rgba8"]
            self.float_data = res["post"]
        if any(k in want for k in ("albedo", "normal", "depth")):
            aov = self.render_aovs(crop=crop)
            res.update({k: aov[k] for k in ("albedo", "normal", "depth") if k in want})
        if on_progress:
            on_progress(1.0)
        assert n == res["rgba8"].shape[0] * res["rgba8"].shape[1]
        return res

    def checkpoint(self, crop=None):
        """(per-pixel float64 sums (h, w, 3), samples_done) of the last render, finished or
        cancelled (rt_render_checkpoint); pass it to render(resume=...) to continue."""
        lib = capi.load_library()
        st = self.settings(crop=crop)
        cw, ch = st.crop_w or self.width, st.crop_h or self.height
        sums = np.zeros((ch, cw, 3), dtype=np.float64)
        done = C.c_int32()
        capi.check(lib.rt_render_checkpoint(self.scene_handle(), sums.ctypes.data_as(C.POINTER(C.c_double)), sums.size,
                                            C.byref(done)))
        return sums, done.value

    def close(self):
        if self._scene is not None:
            capi.load_library().rt_scene_destroy(self._scene)
            self._scene = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
