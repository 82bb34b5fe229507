"""Error-estimate probe (DEV TOOL): what the estimate costs, and how well it is calibrated.
usage: python scripts/probe_error_estimate.py cost [reps]      kernel time of config 3 (16 batches) and mesh50k (22
                                                               aligned batches) with the estimate on and off, the
                                                               two interleaved, each pass twice
       python scripts/probe_error_estimate.py calibration [seeds]   Cornell 64 x 64 x 32 spp over `seeds` seeds (32):
                                                               sum over pixels of the sample variance of the mean
                                                               across seeds / sum over pixels of the mean estimated
                                                               var_mean (1 = calibrated)
Each prints one JSON line per figure."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: F401,E402
import bench  # noqa: E402
from blenderraytracer_amd.renderer import GpuRayTracer  # noqa: E402
from blenderraytracer_amd.scene import load_scene_json  # noqa: E402


def cost(reps):
    for name in ("rtow", "mesh50k"):
        rt = bench.make_tracer(bench.CONFIGS[name], "f64", 1, 0)
        rt.render(batch_samples=-16)
        ms = {False: [], True: []}
        for _ in range(2):                                   # interleaved x 2: off, on, off, on
            for on in (False, True):
                rt.error_estimate_on = on
                rt.render(batch_samples=-16)                 # the first render after a switch (allocations)
                for _ in range(reps):
                    rt.render(batch_samples=-16)
                    ms[on].append(rt.last_stats.kernel_ms)
        st = rt.error_stats()
        off, on = statistics.median(ms[False]), statistics.median(ms[True])
        print(json.dumps({"probe": "cost", "config": name, "groups": st["groups"],
                          "chunk_samples": st["chunk_samples"], "frame_error": st["frame_error"],
                          "kernel_ms_off": round(off, 3), "kernel_ms_on": round(on, 3),
                          "spread_off": [round(min(ms[False]), 3), round(max(ms[False]), 3)],
                          "spread_on": [round(min(ms[True]), 3), round(max(ms[True]), 3)],
                          "on_over_off": round(on / off, 5), "reps": 2 * reps}), flush=True)
        rt.close()


def calibration(seeds):
    w = h = 64
    spp = 32
    means, ests = [], []
    for seed in range(1, seeds + 1):
        rt = GpuRayTracer(w, h, seed=seed, error_estimate=True)
        assert rt.load_from_json(load_scene_json("cornell.json"))
        rt.update_render_settings({"maxBounces": 5, "samples": spp})
        means.append(rt.render(want=("mean",), batch_samples=-16)["mean"])
        ests.append(rt.error_estimate()[0])
        groups = rt.error_stats()["groups"]
        rt.close()
    across = np.var(np.stack(means), axis=0, ddof=1)          # the sample variance of the mean, per pixel and channel
    est = np.mean(np.stack(ests), axis=0)
    print(json.dumps({"probe": "calibration", "scene": "cornell 64x64x32spp", "seeds": seeds, "groups": groups,
                      "sum_variance_across_seeds": float(across.sum()), "sum_mean_estimate": float(est.sum()),
                      "ratio": float(across.sum() / est.sum())}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "cost"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else None
    if what == "cost":
        cost(n or 3)
    else:
        calibration(n or 32)
