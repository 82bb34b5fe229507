"""The noise-threshold stop through the other hosts: the Node drop-in (installGpuRender with noiseThreshold) and
rt_render_cli --noise stop at the same batch and give the same bytes as the Python host."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import SCENES_DIR, load_scene_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "blenderraytracer_amd", "lib", "rt_render_cli")
TOOL = os.path.join(ROOT, "tests", "js", "error_host_tool.mjs")
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu

SCENE, W, H, SEED, SPP = "cornell.json", 24, 20, 5, 32
STEPS = -16              # about 16 progress batches: what the CLI's --noise and the drop-in's default ask for

_python = {}


def python_host(gpu):
    """The Python host's figures, once: the frame error after every batch of the plain render, a threshold in the
    middle of them, and the thresholded render (its samples and RGBA8 frame)."""
    if not _python:
        rt = GpuRayTracer(W, H, seed=SEED, error_estimate=True)
        assert rt.load_from_json(load_scene_json(SCENE))
        rt.update_render_settings({"samples": SPP})
        errs = []
        rt.render(batch_samples=STEPS, on_progress=lambda f: f < 1 and errs.append(rt.error_stats()["frame_error"]) and False)
        errs.append(rt.error_stats()["frame_error"])
        assert len(errs) == 16
        thr = errs[7]
        assert math.isfinite(thr)
        k = next(i + 1 for i, e in enumerate(errs) if e <= thr)
        res = rt.render(batch_samples=STEPS, noise_threshold=thr)
        st = rt.error_stats()
        assert st["converged"] == 1 and st["samples"] == 2 * k < SPP
        _python.update(errs=errs, thr=thr, samples=st["samples"], frame_error=st["frame_error"], rgba8=res["rgba8"].copy())
        rt.close()
    return _python


@pytest.mark.skipif(not os.path.exists(CLI), reason="rt_render_cli not built")
def test_cli_noise_stops_like_the_python_host(gpu, tmp_path):
    p = python_host(gpu)
    out = tmp_path / "img.pam"
    r = subprocess.run([CLI, os.path.join(SCENES_DIR, SCENE), "--width", str(W), "--height", str(H), "--seed", str(SEED),
                        "--spp", str(SPP), "--noise", repr(p["thr"]), "--out", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["samples_done"] == p["samples"] and line["converged"] == 1
    assert line["frame_error"] == p["frame_error"]
    body = out.read_bytes().partition(b"ENDHDR\n")[2]
    assert np.array_equal(np.frombuffer(body, dtype=np.uint8).reshape(H, W, 4), p["rgba8"])
    # --min-spp beyond that batch: the whole render here if no later batch qualifies, else the first that does
    k2 = next((i + 1 for i, e in enumerate(p["errs"]) if e <= p["thr"] and 2 * (i + 1) > p["samples"]), 16)
    r = subprocess.run([CLI, os.path.join(SCENES_DIR, SCENE), "--width", str(W), "--height", str(H), "--seed", str(SEED),
                        "--spp", str(SPP), "--noise", repr(p["thr"]), "--min-spp", str(p["samples"] + 1)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["samples_done"] == 2 * k2


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_drop_in_noise_threshold_stops_like_the_python_host(gpu, tmp_path):
    p = python_host(gpu)
    out = tmp_path / "frame.bin"
    r = subprocess.run([NODE, TOOL, SCENE, str(W), str(H), str(SEED), str(SPP), repr(p["thr"]), "0", str(out)], cwd=ROOT,
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = json.loads(r.stdout)
    assert d["stats"]["samples"] == p["samples"] and d["stats"]["converged"] == 1
    assert d["stats"]["frameError"] == p["frame_error"]
    assert d["lastSamples"] == W * H * p["samples"]
    assert (d["relErrorLength"], d["varMeanLength"]) == (W * H, 3 * W * H)
    # onProgress saw the same figures, batch by batch (NaN, as null, after the first: one chunk partial per pixel)
    seen = [float("nan") if e is None else e for e in d["progress"]]
    assert len(seen) == p["samples"] // 2
    assert all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(seen, p["errs"]))
    assert np.array_equal(np.frombuffer(out.read_bytes(), dtype=np.uint8).reshape(H, W, 4), p["rgba8"])
