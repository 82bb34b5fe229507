"""Cost of direct lighting (a measurement, not a gate): configs 2, 3 and 5 (Cornell, RTOW, mesh50k) in binary64
with one point light and one sun added, rendered lit (the F_LIGHT kernels: World order or the general ordered
walk, one-wave sample pool) and unlit through the same, lit-capable kernels — two directional lights of
direction (0, 0, 0), which never pass the cosine test, so no shadow ray is cast and no radiance added: what
the lit kernels cost before any shadow ray — plus the unlit scene on the kernel it normally takes.  Prints
kernel ms, Msamples/s and shadow rays per sample (counted by the kernel's own code compiled for the CPU,
tests/hostcheck/light_check.cpp, over three full-width bands of 4 rows at 4 spp).
usage: python scripts/probe_lights.py [spp-divisor] (default 4: a quarter of each config's spp)"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402
from blenderraytracer_amd import capi  # noqa: E402
from blenderraytracer_amd.renderer import GpuRayTracer  # noqa: E402
from blenderraytracer_amd.scene import load_scene_json  # noqa: E402
import bench  # noqa: E402
import lightcheck_binding as lb  # noqa: E402

div = int(sys.argv[1]) if len(sys.argv) > 1 else 4
LIGHTS = {
    "cornell": [{"type": "point", "position": [1.6, -1.9, -2.4], "color": [1, 0.95, 0.9], "intensity": 6},
                {"type": "directional", "direction": [-0.3, -1, -0.4], "color": [1, 1, 0.9], "intensity": 0.5}],
    "rtow": [{"type": "point", "position": [2, 7, 1], "color": [1, 0.9, 0.8], "intensity": 30},
             {"type": "directional", "direction": [-1, -0.25, -0.6], "color": [1, 1, 0.9], "intensity": 1.25}],
    "mesh50k": [{"type": "point", "position": [3, 6, 4], "color": [1, 1, 1], "intensity": 30},
                {"type": "directional", "direction": [-1, -1, -0.5], "color": [1, 1, 0.9], "intensity": 1.0}],
}


def timed(rt, n):
    rt.render()                                    # warm-up + upload
    ms = []
    for _ in range(3):
        rt.render()
        ms.append(rt.last_stats.kernel_ms)
    st = rt.last_stats
    return ms, n / (min(ms) * 1e-3) / 1e6, st


lib = capi.load_library()
for name in ("cornell", "rtow", "mesh50k"):
    cfg = bench.CONFIGS[name]
    spp = max(1, cfg["spp"] // div)
    n = cfg["w"] * cfg["h"] * spp
    data = copy.deepcopy(load_scene_json(cfg["scene"]))
    data["lights"] = LIGHTS[name]
    dark = copy.deepcopy(data)
    dark["lights"] = [{"type": "directional", "direction": [0, 0, 0]} for _ in data["lights"]]
    rows = []
    for label, d, lit in (("unlit, its own kernel", data, False), ("lit kernels, no shadow ray cast", dark, True),
                          ("lit", data, True)):
        rt = GpuRayTracer(cfg["w"], cfg["h"], seed=1, precision=capi.RT_PREC_F64, direct_lighting=lit)
        assert rt.load_from_json(d)
        rt.update_render_settings({"maxBounces": cfg["depth"], "samples": spp})
        ms, rate, st = timed(rt, n)
        walk = lib.rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, capi.RT_ACCEL_AUTO)
        rows.append((label, walk, ms, rate, st.segments / n, st.node_visits / n))
        rt.close()
    for label, walk, ms, rate, segs, nodes in rows:
        print(f"{name} {cfg['w']}x{cfg['h']}x{spp} {label}: walk {walk}, kernel ms {' '.join('%.1f' % m for m in ms)}, "
              f"{rate:.0f} Msamples/s (best), segments/sample {segs:.3f}, node visits/sample {nodes:.1f}", flush=True)
    # shadow rays per sample of the lit render, counted by the CPU build of the kernel's code on three bands
    rt = GpuRayTracer(cfg["w"], cfg["h"], seed=1, precision=capi.RT_PREC_F64, direct_lighting=True)
    assert rt.load_from_json(data)
    rt.update_render_settings({"maxBounces": cfg["depth"], "samples": 4})
    cast = blocked = 0
    for q in (1, 2, 3):
        c, b = lb.shadow_rays(rt.packed(), rt.settings(crop=(0, cfg["h"] * q // 4, cfg["w"], 4)))
        cast, blocked = cast + c, blocked + b
    print(f"{name}: {cast / (3 * 4 * cfg['w'] * 4):.3f} shadow rays per sample on three bands, {100 * blocked / max(cast, 1):.1f} % occluded",
          flush=True)
