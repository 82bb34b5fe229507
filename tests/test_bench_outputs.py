"""bench.py --dump-outputs: the arrays of the last timed step as .npy files (float64 sums kept, the rest
as float32), a frame over the byte budget cut to one seeded sample of its pixels; and the plain run's
result line (no --full: none of the figures that take runs of their own)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _frame(n):
    rng = np.random.default_rng(3)
    return {"sum": rng.random((n, 3)), "post": rng.random((n, 4), dtype=np.float32),
            "rgba8": rng.integers(0, 256, (n, 4), dtype=np.uint8)}


def test_dump_outputs_whole_frame(tmp_path):
    f = _frame(1000)
    bench.dump_outputs(str(tmp_path / "d"), f)
    assert sorted(os.listdir(tmp_path / "d")) == ["post.npy", "rgba8.npy", "sum.npy"]
    s, p, r = (np.load(tmp_path / "d" / f"{k}.npy") for k in ("sum", "post", "rgba8"))
    assert (s.dtype, p.dtype, r.dtype) == (np.float64, np.float32, np.float32)
    assert np.array_equal(s, f["sum"]) and np.array_equal(p, f["post"]) and np.array_equal(r, f["rgba8"])


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 * 1000)         # 64 B per pixel: room for 1000 of the 4001
    f = _frame(4001)
    bench.dump_outputs(str(tmp_path / "a"), f)
    bench.dump_outputs(str(tmp_path / "b"), _frame(4001))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["pixel_index.npy", "post.npy", "rgba8.npy", "sum.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / k) for k in names) <= 64 * 1000 + 4 * 128     # + the .npy headers
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 1000 and np.all(np.diff(idx) > 0) and idx[-1] < 4001
    for k in names:                                              # the same pixels in every run
        assert np.array_equal(np.load(tmp_path / "a" / k), np.load(tmp_path / "b" / k)), k
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "sum.npy"), f["sum"][i])
    assert np.array_equal(np.load(tmp_path / "a" / "rgba8.npy"), f["rgba8"][i])


def test_dump_budget_below_64_mb():
    assert 0 < bench.DUMP_BUDGET < 64 * 10 ** 6


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(gpu, tmp_path):
    """One plain run of the smallest config: --steps sets the timed steps, the line carries ms_per_step
    and none of --full's figures, and the .npy outputs are the frame --dump writes (the sums and RGBA8 of
    the same step) and the oracle's frame of the same scene, seed and settings."""
    from oracle import binding
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "sample_scene",
                        "--steps", "2", "--warmup", "1", "--dump", str(tmp_path / "f.npz"), "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "Msamples/s" and line["dtype"] == "f64"
    assert line["metric"] == bench.METRIC and line["higher_is_better"] is True
    assert abs(line["value"] - 256 * 256 * 4 / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-2 * line["value"]
    for k in ("roofline", "cpu_baseline", "end_to_end", "end_to_end_node", "progressive_16"):
        assert k not in line, k
    s, p, c = (np.load(out / f"{k}.npy") for k in ("sum", "post", "rgba8"))
    assert s.shape == (256 * 256, 3) and s.dtype == np.float64
    assert p.shape == c.shape == (256 * 256, 4) and p.dtype == c.dtype == np.float32
    z = np.load(tmp_path / "f.npz")
    assert np.array_equal(s.reshape(-1), z["sum"]) and np.array_equal(c.reshape(-1), z["rgba8"])
    rt = bench.make_tracer(bench.CONFIGS["sample_scene"], "f64", 1, 0)
    o = binding.render(rt.packed(), rt.settings())
    rt.close()
    assert np.max(np.abs(s.reshape(256, 256, 3) / 4 - o["mean"])) <= 1e-12        # smoke()'s bound
    assert np.array_equal(c.reshape(256, 256, 4), o["rgba8"])
