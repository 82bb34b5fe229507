"""The binary64 lean grid kernel with the expanded sphere filter and the full tiles' shifted pixel
coordinates (RT_FILTER_X, RT_TILE_SHIFT) on the device: RTOW at 72x45 (full tiles and a ragged bottom row) and at
76x45 (a ragged right column of tiles too: the division beside the shift), 8 spp, depth 5, against World order bit
for bit; the closest hits of the host check's adversarial rays; a second process; and the tile mapping against
the lane-per-pixel kernel.  Every frame is rendered twice: with per-pixel segment and draw counts (the kernel's
counting twin, trace_pool_lds_kernel<double, true, 9>) and without (want=("mean",): the kernel a plain render and
the benchmark run, <double, false, 9>)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (HIP runtime first)
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
what = sys.argv[3].split(",")
out = {}
def render(tag, w, h, spp, accel):
    rt = GpuRayTracer(w, h, seed=11, accel=accel, precision=capi.RT_PREC_F64)
    assert rt.load_from_json(load_scene_json("rtow.json"))
    rt.update_render_settings({"samples": spp, "maxBounces": 5})
    if accel == capi.RT_ACCEL_AUTO:
        assert capi.load_library().rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, accel) == 2, "RTOW should walk the grid"
    r = rt.render(want=("mean", "segments", "draws"))
    for k in ("mean", "segments", "draws"):
        out[f"{tag}.{k}"] = r[k]
    out[f"{tag}.plain"] = rt.render(want=("mean",))["mean"]          # the kernel without counting
    return rt
if "frame" in what:
    render("grid", 72, 45, 8, capi.RT_ACCEL_AUTO).close()
if "brute" in what:
    render("brute", 72, 45, 8, capi.RT_ACCEL_BRUTE).close()
    render("ragged", 76, 45, 8, capi.RT_ACCEL_AUTO).close()
    render("ragged_brute", 76, 45, 8, capi.RT_ACCEL_BRUTE).close()
if "tile" in what:
    render("tile", 64, 64, 4, capi.RT_ACCEL_AUTO).close()
if "hits" in what:
    import hostcheck_binding as hb
    from test_gpu_parity import _closest_hits
    rt = GpuRayTracer(64, 36, seed=3)
    assert rt.load_from_json(load_scene_json("rtow.json"))
    r, ht, hk, hi = hb.bvh_rays(rt.packed(), 20000, 99, 0)
    out["bt"], out["bk"], out["bi"] = _closest_hits(rt, r, capi.RT_PREC_F64, capi.RT_ACCEL_BRUTE)
    out["vt"], out["vk"], out["vi"] = _closest_hits(rt, r, capi.RT_PREC_F64, capi.RT_ACCEL_AUTO)
    rt.close()
np.savez(sys.argv[2], **out)
'''


def _child(path, what, **env):
    r = subprocess.run([sys.executable, "-c", _SCRIPT, ROOT, str(path), what], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.fixture(scope="module")
def first(gpu, tmp_path_factory):
    return _child(tmp_path_factory.mktemp("filterx") / "first.npz", "frame,brute,tile,hits")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("grid,brute,w", [("grid", "brute", 72), ("ragged", "ragged_brute", 76)])
def test_default_kernel_equals_world_order(first, grid, brute, w):
    assert first[f"{grid}.segments"].sum() > w * 45 * 8
    assert np.array_equal(first[f"{grid}.segments"], first[f"{brute}.segments"])
    assert np.array_equal(first[f"{grid}.draws"], first[f"{brute}.draws"])
    assert np.array_equal(bits(first[f"{grid}.mean"]), bits(first[f"{brute}.mean"]))
    # the kernel without counting: the same bits, and World order's
    assert np.array_equal(bits(first[f"{grid}.plain"]), bits(first[f"{grid}.mean"]))
    assert np.array_equal(bits(first[f"{grid}.plain"]), bits(first[f"{brute}.plain"]))


def test_closest_hits_grid_equals_world_order(first):
    assert (first["bk"] >= 0).sum() > len(first["bk"]) // 10
    assert np.array_equal(first["bk"], first["vk"]) and np.array_equal(first["bi"], first["vi"])
    assert np.array_equal(bits(first["bt"]), bits(first["vt"]))


def test_second_process_reproduces_the_bits(first, tmp_path):
    again = _child(tmp_path / "again.npz", "frame")
    for k in ("mean", "segments", "draws"):
        assert np.array_equal(first[f"grid.{k}"], again[f"grid.{k}"], equal_nan=True), k
    assert np.array_equal(bits(first["grid.mean"]), bits(again["grid.mean"]))
    assert np.array_equal(bits(first["grid.plain"]), bits(again["grid.plain"]))


def test_tile_mapping_equals_lane_per_pixel(first, tmp_path):
    """64x64 at 4 spp: every tile full.  Per-pixel segments and draws of the pool equal the lane-per-pixel kernel's
    (RT_SAMPLE_POOL=0) exactly; the means are the same four non-negative terms added in another order: each order's
    sum carries 3 roundings of partial sums no larger than the total S, so each is within 3 * 2^-53 S of the exact
    sum and the two agree to 6 * 2^-53 S (6.01 with S replaced by a computed sum)."""
    lpp = _child(tmp_path / "lpp.npz", "tile", RT_SAMPLE_POOL="0")
    assert np.array_equal(first["tile.segments"], lpp["tile.segments"])
    assert np.array_equal(first["tile.draws"], lpp["tile.draws"])
    a, b = first["tile.mean"], lpp["tile.mean"]
    print(f"max relative difference {np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) / 2.0 ** -53:.2f} x 2^-53")
    assert np.allclose(a, b, rtol=6.01 * 2.0 ** -53, atol=0)
    # the kernel without counting adds the same terms in the same order as its counting twin
    assert np.array_equal(bits(first["tile.plain"]), bits(first["tile.mean"]))
    assert np.allclose(first["tile.plain"], lpp["tile.plain"], rtol=6.01 * 2.0 ** -53, atol=0)
