"""The guided filter's two measurements (DEV TOOL, needs a GPU; DESIGN.md §4 "Guided filter").

    python scripts/probe_guided.py sweep    # the defaults' sweep: post-gamma RMS vs a 1024-spp frame, 64x48, 4 spp
    python scripts/probe_guided.py cost     # device time of aov_kernel and of every level at 1920x1080 (HIP events)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime in the process)

from blenderraytracer_amd import capi  # noqa: E402
from blenderraytracer_amd.renderer import GUIDED_LEVELS, GUIDED_SIGMAS, GpuRayTracer  # noqa: E402
from blenderraytracer_amd.scene import load_scene_json  # noqa: E402

SCENES = ("sample_scene", "cornell", "sample_mesh")


def tracer(name, w, h, seed, spp):
    rt = GpuRayTracer(w, h, seed=seed)
    assert rt.load_from_json(load_scene_json(name + ".json"))
    rt.update_render_settings({"samples": spp})
    return rt


def rms(a, b):
    d = np.clip(a[..., :3].astype(np.float64), 0, 1) - np.clip(b[..., :3].astype(np.float64), 0, 1)
    return float(np.sqrt(np.mean(d * d)))


def sweep():
    d = GUIDED_SIGMAS
    grid = [(c, a, d["normal"], d["depth"]) for c in (0.25, 0.5, 1.0) for a in (0.05, 0.1, 0.2)]
    grid += [(d["color"], d["albedo"], n, d["depth"]) for n in (0.2, 0.7)]
    grid += [(d["color"], d["albedo"], d["normal"], z) for z in (0.025, 0.1)]
    refs, plains, tracers = {}, {}, {}
    for name in SCENES:
        ref = tracer(name, 64, 48, 99, 1024)
        refs[name] = ref.render()["post"]
        ref.close()
        tracers[name] = tracer(name, 64, 48, 3, 4)
        plains[name] = rms(tracers[name].render()["post"], refs[name])
    print("| sigma colour | albedo | normal | depth | " + " | ".join(SCENES) + " |")
    print("|---|---|---|---|" + "---|" * len(SCENES))
    print("| plain 4 spp (RMS) | | | | " + " | ".join(f"{plains[n]:.5f}" for n in SCENES) + " |")
    for c, a, n, z in grid:
        row = []
        for name in SCENES:
            rt = tracers[name]
            rt.update_render_settings({"samples": 4, "guidedDenoise": True, "guidedLevels": GUIDED_LEVELS, "guidedSigmaColor": c,
                                       "guidedSigmaAlbedo": a, "guidedSigmaNormal": n, "guidedSigmaDepth": z})
            row.append(rms(rt.render()["post"], refs[name]) / plains[name])
        print(f"| {c:g} | {a:g} | {n:g} | {z:g} | " + " | ".join(f"{r:.3f}" for r in row) + " |")


def cost(name="rtow", w=1920, h=1080, reps=10):
    lib = capi.load_library()
    rt = tracer(name, w, h, 1, 4)
    mean = rt.render(want=("mean",))["mean"]
    scene, st = rt.scene_handle(), rt.settings()
    n = w * h
    d_color = torch.from_numpy(mean).cuda()
    d_guides = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            best.append(a.elapsed_time(b))
        return float(np.median(best))

    t_aov = timed(lambda: capi.check(lib.rt_aovs_device(scene, C.byref(st), ptr(d_guides), None)))
    print(f"{name} {w}x{h}: aov_kernel {t_aov:.3f} ms ({32 * n / t_aov / 1e6:.0f} GB/s of its 32 B/pixel written)")
    sig = [GUIDED_SIGMAS[k] for k in ("color", "albedo", "normal", "depth")]
    prev = 0.0
    for levels in range(1, GUIDED_LEVELS + 1):
        p = capi.GuidedParams(levels, 0, *sig)
        t = timed(lambda: capi.check(lib.rt_guided_filter_device(scene, w, h, C.byref(p), ptr(d_color), ptr(d_guides),
                                                                 ptr(d_out), None)))
        ms = t - prev
        print(f"  level {levels - 1} (step {1 << (levels - 1)}): {ms:.3f} ms, {80 * n / ms / 1e6:.0f} GB/s of the compulsory "
              f"80 B/pixel (24 read + 32 read + 24 written); cumulative {t:.3f} ms")
        prev = t
    rt.update_render_settings({"samples": 4, "guidedDenoise": True})
    rt.render()
    g = rt.last_stats.finalize_ms
    rt.update_render_settings({"samples": 4, "guidedDenoise": False})
    rt.render()
    print(f"  epilogue of rt_render: guided {g:.3f} ms, plain {rt.last_stats.finalize_ms:.3f} ms")
    rt.close()


if __name__ == "__main__":
    {"sweep": sweep, "cost": cost}[sys.argv[1] if len(sys.argv) > 1 else "sweep"]()
