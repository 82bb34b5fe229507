"""Throughput of the textured path (a measurement, not a gate): RTOW at config 3's size with a checker
ground (the F_TEX kernel: general ordered walk, one-wave sample pool) and the same scene untextured forced
onto the same kernel family (RT_BVH_WALK=two: the general ordered walk instead of the grid; RT_LEAN=0: its
full form, no lean kernel), so the difference is the texture's cost and not the walk's.  (The untextured
scene on the kernel it normally takes, the grid in LDS, is bench.py's default figure.)
usage: python scripts/probe_textures.py [spp] [precision f64|f32]"""
import copy
import os
import sys

os.environ.setdefault("RT_BVH_WALK", "two")       # read once when librt_hip.so first launches
os.environ.setdefault("RT_LEAN", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402
from blenderraytracer_amd import capi  # noqa: E402
from blenderraytracer_amd.renderer import GpuRayTracer  # noqa: E402
from blenderraytracer_amd.scene import load_scene_json  # noqa: E402
import bench  # noqa: E402

cfg = bench.CONFIGS["rtow"]
spp = int(sys.argv[1]) if len(sys.argv) > 1 else cfg["spp"]
prec = {"f64": capi.RT_PREC_F64, "f32": capi.RT_PREC_F32}[sys.argv[2] if len(sys.argv) > 2 else "f64"]

plain = load_scene_json(cfg["scene"])
textured = copy.deepcopy(plain)
ground = max((o for o in textured["objects"] if o["type"] == "sphere"), key=lambda o: o["radius"])
ground["material"]["texture"] = {"type": "checkerboard"}

lib = capi.load_library()
for name, data in (("untextured, general walk", plain), ("checker ground (F_TEX)", textured)):
    rt = GpuRayTracer(cfg["w"], cfg["h"], seed=1, precision=prec)
    assert rt.load_from_json(data)
    rt.update_render_settings({"maxBounces": cfg["depth"], "samples": spp})
    rt.render()                                    # warm-up + upload
    ms = []
    for _ in range(3):
        rt.render()
        ms.append(rt.last_stats.kernel_ms)
    st = rt.last_stats
    n = cfg["w"] * cfg["h"] * spp
    best = min(ms)
    print(f"rtow {cfg['w']}x{cfg['h']}x{spp} {name}: walk {lib.rt_scene_walk(rt.scene_handle(), prec, capi.RT_ACCEL_AUTO)}, "
          f"kernel ms {' '.join('%.1f' % m for m in ms)}, {n / (best * 1e-3) / 1e6:.0f} Msamples/s (best), "
          f"segments/sample {st.segments / n:.3f}", flush=True)
    rt.close()
