"""Cost and value of emitter sampling (a measurement, not a gate): Cornell 512 x 512, the default scene and
nee_mixed in binary64, plain and with emitter sampling.  Prints kernel ms and Msamples/s of both, shadow queries per
sample and their occluded share (counted by the kernel's own code compiled for the CPU, tests/hostcheck/
nee_check.cpp, on three bands of 4 rows at 4 spp), and the post-gamma RMS against a 4096-spp plain frame of another
seed at equal spp and at equal kernel time (the plain render given time_with / time_plain times the samples).
usage: python scripts/probe_emitters.py [spp] (default 64)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402
from blenderraytracer_amd import capi  # noqa: E402
import neecheck_binding as nb  # noqa: E402

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 64
SCENES = (("cornell", 512, 512), (None, 512, 512), ("nee_mixed", 512, 512))


def timed(rt):
    rt.render()                                    # warm-up + upload
    ms = []
    for _ in range(3):
        res = rt.render()
        ms.append(rt.last_stats.kernel_ms)
    return min(ms), ms, res["post"][..., :3].astype(np.float64)


def rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


for scene, w, h in SCENES:
    name = scene or "default"
    ref_rt = nb.tracer(scene, w, h, seed=977, samples=4096)
    ref = ref_rt.render()["post"][..., :3].astype(np.float64)
    ref_rt.close()
    rows = {}
    for on in (False, True):
        rt = nb.tracer(scene, w, h, seed=1, samples=spp, emitter_sampling=on)
        best, ms, post = timed(rt)
        rows[on] = (best, post)
        print(f"{name} {w}x{h}x{spp} {'sampling' if on else 'plain'}: emitters {rt.emitter_count()}, kernel ms "
              f"{' '.join('%.2f' % m for m in ms)}, {w * h * spp / (best * 1e-3) / 1e6:.0f} Msamples/s (best), "
              f"RMS against the 4096-spp frame {rms(post, ref):.4f}", flush=True)
        rt.close()
    ratio = rows[True][0] / rows[False][0]
    more = max(spp + 1, int(round(spp * ratio)))
    rt = nb.tracer(scene, w, h, seed=1, samples=more)
    best, ms, post = timed(rt)
    rt.close()
    print(f"{name}: sampling costs {ratio:.2f}x the plain kernel time; plain at {more} spp ({best:.2f} ms): RMS "
          f"{rms(post, ref):.4f}; equal-time RMS ratio sampling / plain {rms(rows[True][1], ref) / rms(post, ref):.3f}, "
          f"equal-spp {rms(rows[True][1], ref) / rms(rows[False][1], ref):.3f}", flush=True)
    rt = nb.tracer(scene, w, h, seed=1, samples=4)
    cast = blocked = 0
    for q in (1, 2, 3):
        c, b = nb.shadow_queries(rt.packed(), rt.settings(crop=(0, h * q // 4, w, 4)))
        cast, blocked = cast + c, blocked + b
    print(f"{name}: {cast / (3 * 4 * w * 4):.3f} shadow queries per sample on three bands, "
          f"{100 * blocked / max(cast, 1):.1f} % occluded", flush=True)
