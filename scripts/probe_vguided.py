"""The variance-guided filter's two measurements (DEV TOOL, needs a GPU; DESIGN.md §4 "Variance-guided filter").

    python scripts/probe_vguided.py sweep   # sigma_variance sweep: post-gamma RMS vs a 1024-spp frame, 64x48, 8 and 16 spp
    python scripts/probe_vguided.py cost    # device time of every level at 1920x1080 beside the plain filter's (HIP events)

The protocol is scripts/probe_guided.py's: the same 64x48 views, the 1024-spp frame of another seed, ratios to the
unfiltered frame of the same sample count.
"""
import ctypes as C
import math
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
SIGMAS_V = (1.0, 2.0, 4.0, 8.0, 16.0)


def tracer(name, w, h, seed, spp, estimate=True):
    rt = GpuRayTracer(w, h, seed=seed, error_estimate=estimate)
    assert rt.load_from_json(load_scene_json(name + ".json"))
    rt.update_render_settings({"samples": spp})
    return rt


def rms(a, b):
    d = np.clip(a[..., :3].astype(np.float64), 0, 1) - np.clip(b[..., :3].astype(np.float64), 0, 1)
    return float(np.sqrt(np.mean(d * d)))


def sweep():
    refs = {}
    for name in SCENES:
        ref = tracer(name, 64, 48, 99, 1024, estimate=False)
        refs[name] = ref.render()["post"]
        ref.close()
    rows = {}
    for spp in (8, 16):                                   # batches of 4: K = 2 and K = 4 chunk partials per pixel
        for name in SCENES:
            rt = tracer(name, 64, 48, 3, spp)

            def ratio(keys, plain=None):
                rt.update_render_settings({"samples": spp, "guidedDenoise": False, "guidedVariance": False, **keys})
                e = rms(rt.render(batch_samples=4)["post"], refs[name])
                return e if plain is None else e / plain
            plain = ratio({})
            groups = None
            rows.setdefault(("unfiltered (RMS)", spp), []).append(plain)
            rows.setdefault(("plain guided (defaults)", spp), []).append(ratio({"guidedDenoise": True}, plain))
            for sv in SIGMAS_V:
                rows.setdefault((f"sigma_variance {sv:g}", spp), []).append(
                    ratio({"guidedDenoise": True, "guidedVariance": True, "guidedSigmaVariance": sv}, plain))
                groups = rt.error_stats()["groups"]
            rows.setdefault(("groups K", spp), []).append(groups)
            rt.close()
    print("| filter | spp | " + " | ".join(SCENES) + " | worst | geometric mean |")
    print("|---|---|" + "---|" * (len(SCENES) + 2))
    for (label, spp), r in rows.items():
        if label.startswith("unfiltered"):
            print(f"| {label} | {spp} | " + " | ".join(f"{x:.5f}" for x in r) + " | | |")
        elif label.startswith("groups"):
            print(f"| {label} | {spp} | " + " | ".join(str(x) for x in r) + " | | |")
        else:
            gm = math.exp(sum(math.log(x) for x in r) / len(r))
            print(f"| {label} | {spp} | " + " | ".join(f"{x:.3f}" for x in r) + f" | {max(r):.3f} | {gm:.3f} |")
    print("| both sample counts | | | | | worst | geometric mean |")
    for sv in SIGMAS_V:
        r = rows[(f"sigma_variance {sv:g}", 8)] + rows[(f"sigma_variance {sv:g}", 16)]
        gm = math.exp(sum(math.log(x) for x in r) / len(r))
        print(f"| sigma_variance {sv:g} | 8 + 16 | | | | {max(r):.3f} | {gm:.3f} |")


def cost(name="rtow", w=1920, h=1080, reps=10):
    lib = capi.load_library()
    rt = tracer(name, w, h, 1, 8)
    mean = rt.render(want=("mean",), batch_samples=4)["mean"]
    var, _ = rt.error_estimate()
    scene, st = rt.scene_handle(), rt.settings()
    n = w * h
    d_color, d_var = torch.from_numpy(mean).cuda(), torch.from_numpy(var).cuda()
    d_guides = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_vout = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
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

    capi.check(lib.rt_aovs_device(scene, C.byref(st), ptr(d_guides), None))
    torch.cuda.synchronize()
    sig = [GUIDED_SIGMAS[k] for k in ("color", "albedo", "normal", "depth")]
    sv = capi.RT_GUIDED_DEFAULT_SIGMA_VARIANCE
    print(f"{name} {w}x{h}, {rt.error_stats()['groups']} groups; per level: variance form (128 B/pixel: 48 + 32 read, 48 written) "
          "| plain (80 B/pixel)")
    prev_v = prev_p = 0.0
    for levels in range(1, GUIDED_LEVELS + 1):
        p = capi.GuidedParams(levels, 0, *sig)
        tv = timed(lambda: capi.check(lib.rt_guided_filter_variance_device(scene, w, h, C.byref(p), sv, ptr(d_color), ptr(d_var),
                                                                           ptr(d_guides), ptr(d_out), ptr(d_vout), None)))
        tp = timed(lambda: capi.check(lib.rt_guided_filter_device(scene, w, h, C.byref(p), ptr(d_color), ptr(d_guides),
                                                                  ptr(d_out), None)))
        mv, mp = tv - prev_v, tp - prev_p
        print(f"  level {levels - 1} (step {1 << (levels - 1)}): {mv:.3f} ms ({128 * n / mv / 1e6:.0f} GB/s) | {mp:.3f} ms "
              f"({80 * n / mp / 1e6:.0f} GB/s); cumulative {tv:.3f} | {tp:.3f} ms")
        prev_v, prev_p = tv, tp
    fin = {}
    for label, keys in (("variance", {"guidedDenoise": True, "guidedVariance": True}), ("guided", {"guidedDenoise": True}),
                        ("plain", {})):
        rt.update_render_settings({"samples": 8, "guidedDenoise": False, "guidedVariance": False, **keys})
        ms = []
        for _ in range(reps + 1):
            rt.render(batch_samples=4)
            ms.append(rt.last_stats.finalize_ms)
        fin[label] = float(np.median(ms[1:]))
    print(f"  epilogue of rt_render (median of {reps}): variance-guided {fin['variance']:.3f} ms, guided {fin['guided']:.3f} ms, "
          f"plain {fin['plain']:.3f} ms")
    rt.close()


if __name__ == "__main__":
    {"sweep": sweep, "cost": cost}[sys.argv[1] if len(sys.argv) > 1 else "sweep"]()
