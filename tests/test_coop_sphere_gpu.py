"""The wave-cooperative unit-sphere draw (RT_COOP_SPHERE, pt_path.h unit_sphere_point) on the device.
rt_shade_segments' variant 2 in binary64 runs the function the lean grid kernel's pool loop runs: on RTOW its 12
outputs, done flag, hit and draw count against the host's ptc_shade_segments (each lane's own loop), bit for bit, with
rays and keys chosen per 64-lane wave — every lane needs a point, exactly one, none, and streams of 12 and more rounds
beside missed rays and glass hits — at ray counts that leave partial and single-lane waves.  Then one 64x64 crop of
config 3 at 16 spp through the whole kernel against the library built with RT_COOP_SPHERE=0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import coopcheck_binding as cb
import hostcheck_binding as hb
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
from test_shade_gpu import device_shade_segments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = capi.RT_PREC_F64
COUNTS = [1, 37, 64, 65, 133]
PATTERNS = ["all", "one", "none", "long"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def rtow():
    """RTOW's tracer; rays from its camera position by what their hit asks of the draw — `need` (Lambertian and
    Metal), `glass` (Dielectric: a hit without a point), `miss` — classified by the host's own shade_segment (the draw
    count moves by three and more exactly where a point was drawn); and streams whose loop takes 12 rounds and more."""
    rt = GpuRayTracer(64, 36, seed=5, precision=F64)
    assert rt.load_from_json(load_scene_json("rtow.json"))
    rng = np.random.default_rng(31)
    n = 6000
    target = np.stack([rng.uniform(-7, 7, n), rng.uniform(0.0, 1.4, n), rng.uniform(-7, 7, n)], axis=1)
    target[: n // 4] = np.array([0.0, 1.0, 0.0]) + rng.uniform(-0.9, 0.9, (n // 4, 3))      # the large glass sphere
    target[n // 4: n // 2, 1] = rng.uniform(4.0, 30.0, n // 4)                              # the sky
    o = np.tile([13.0, 2.0, 3.0], (n, 1))
    rays = np.ascontiguousarray(np.concatenate([o, target - o], axis=1))
    out_f, out_i = hb.shade_segments(rt.packed(), F64, capi.RT_ACCEL_BRUTE, rays, np.tile([9, 0], (n, 1)), 5, variant=2)
    # (a round is three draws; a Dielectric hit draws at most its one reflectance draw)
    cls = {"need": rays[out_i[:, 3] >= 3], "glass": rays[(out_i[:, 1] >= 0) & (out_i[:, 3] < 3)], "miss": rays[out_i[:, 1] < 0]}
    assert all(len(v) >= 133 for v in cls.values()), {k: len(v) for k, v in cls.items()}
    keys = rng.integers(0, 1 << 32, 400_000, dtype=np.uint64).astype(np.uint32)
    k0 = rng.integers(0, 40, 400_000).astype(np.uint32)
    long = np.flatnonzero(cb.rounds(keys, k0) >= 12)
    assert len(long) >= 40
    yield {"rt": rt, "cls": cls, "long": np.stack([keys[long], k0[long]], axis=1)}
    rt.close()


def wave_case(f, count, first):
    """`count` rays and keys: wave w (64 consecutive rays) takes pattern (first + w) mod 4"""
    rng = np.random.default_rng(1000 * count + first)
    rays, keys = np.zeros((count, 6)), np.zeros((count, 2), dtype=np.uint32)
    keys[:, 0] = rng.integers(0, 1 << 32, count, dtype=np.uint64)
    keys[:, 1] = rng.integers(0, 50, count)
    take = {k: iter(rng.permutation(len(v))) for k, v in f["cls"].items()}
    longs = iter(rng.permutation(len(f["long"])))
    for w0 in range(0, count, 64):
        pattern = PATTERNS[(first + w0 // 64) % 4]
        lanes = range(w0, min(w0 + 64, count))
        lucky = w0 + int(rng.integers(0, len(lanes)))
        for q in lanes:
            if pattern == "all":
                kind = "need"
            elif pattern == "one":
                kind = "need" if q == lucky else ("miss", "glass")[q % 2]
            elif pattern == "none":
                kind = ("miss", "glass")[q % 2]
            else:
                kind = ("need", "miss", "glass", "need", "glass", "miss", "miss")[(q - w0) % 7] if len(lanes) > 1 else "need"
                if kind == "need" and (q - w0) % 2 == 0:
                    keys[q] = f["long"][next(longs)]
            rays[q] = f["cls"][kind][next(take[kind])]
    return rays, keys


@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH], ids=["brute", "bvh"])
@pytest.mark.parametrize("first", range(4), ids=PATTERNS)
@pytest.mark.parametrize("count", COUNTS)
def test_device_draws_equal_the_lanes_own_loops(gpu, rtow, count, first, accel):
    rays, keys = wave_case(rtow, count, first)
    want_f, want_i = hb.shade_segments(rtow["rt"].packed(), F64, accel, rays, keys, 5, variant=2)
    got_f, got_i = device_shade_segments(gpu, rtow["rt"], F64, accel, rays, keys, 5, variant=2)
    assert np.array_equal(got_i, want_i)                      # done, kind, index, draw count
    assert np.array_equal(bits(got_f), bits(want_f))          # origin, direction, T, L
    drew = want_i[:, 3] - keys[:, 1].astype(np.int32) >= 3    # a point was drawn
    pattern = PATTERNS[first]
    if pattern == "all" or (pattern == "long" and count == 1):
        assert drew[:64].all()
    elif pattern == "one":
        assert drew[:64].sum() == 1
    elif pattern == "none":
        assert not drew[:64].any()
    else:
        assert ((want_i[:64, 3] - keys[:64, 1].astype(np.int32)) >= 36).any() and not drew[:64].all()


_CROP_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401  (HIP runtime first)
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
rt = GpuRayTracer(1920, 1080, seed=1, precision=capi.RT_PREC_F64)
assert rt.load_from_json(load_scene_json("rtow.json"))
rt.update_render_settings({"samples": 16, "maxBounces": 5})
assert capi.load_library().rt_scene_walk(rt.scene_handle(), capi.RT_PREC_F64, capi.RT_ACCEL_AUTO) == 2, "RTOW should walk the grid"
crop = (928, 560, 64, 64)
r = rt.render(crop=crop, want=("mean", "segments", "draws"))
sums, done = rt.checkpoint(crop=crop)
plain = rt.render(crop=crop, want=("mean",))["mean"]        # the kernel without counting
np.savez(sys.argv[2], mean=r["mean"], segments=r["segments"], draws=r["draws"], sums=sums, done=done, plain=plain)
rt.close()
'''


def _crop(path, **env):
    r = subprocess.run([sys.executable, "-c", _CROP_SCRIPT, ROOT, str(path)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


def test_crop_equals_the_build_without_it(gpu, tmp_path):
    """config 3's frame, a 64x64 crop below its middle (the ground's small spheres, the glass and the metal one) at
    16 spp: the sums, the per-pixel segment counts and the draw counts of the default library and of the one built
    with RT_COOP_SPHERE=0 are identical, in the counting kernel and in the plain one"""
    off_lib = os.path.join(ROOT, "blenderraytracer_amd", "lib", "librt_hip_coop0.so")
    assert os.path.exists(off_lib), "build() compiles the RT_COOP_SPHERE=0 twin"
    on, off = _crop(tmp_path / "on.npz"), _crop(tmp_path / "off.npz", RT_HIP_LIB=off_lib)
    assert on["segments"].sum() > 64 * 64 * 16 and on["draws"].sum() > on["segments"].sum()
    assert np.array_equal(on["segments"], off["segments"]) and np.array_equal(on["draws"], off["draws"])
    assert int(on["done"]) == int(off["done"]) == 16
    for k in ("sums", "mean", "plain"):
        assert np.array_equal(bits(on[k]), bits(off[k])), k
    assert np.array_equal(bits(on["plain"]), bits(on["mean"]))
