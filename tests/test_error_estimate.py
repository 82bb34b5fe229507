"""The error estimate's arithmetic (csrc/pt_error.h, compiled for the CPU by tests/errcheck_binding.py, driven in
the kernels' order) against the rational reference of tests/error_ref.py, and the estimator's unbiasedness with
unequal groups.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import errcheck_binding as eb
import error_ref as ref

W, H = 11, 9            # four 8x8 tiles, three of them ragged


def running_sum(groups):
    """reduce_kernel's sum: the groups added in chunk order onto zero, binary64"""
    s = np.zeros(groups.shape[1:])
    for g in groups:
        s = s + g
    return s


def host(groups, sizes, batches=None, threshold=0.0, min_samples=0):
    """The CPU build over the group sums (K, h, w, 3), given to the moments pass batch by batch (batches: lists of
    group indices; the chunk of a batch is its first group's size)."""
    K = len(sizes)
    batches = batches or [list(range(K))]
    q = np.zeros(groups.shape[1:])
    for b in batches:
        q = eb.host_moments(q, groups[b], sizes[b[0]], sum(sizes[c] for c in b))
    return eb.host_estimate(running_sum(groups), q, K, sum(sizes), threshold, min_samples)


def check(groups, sizes, batches=None):
    """var_mean, rel_error and the frame's figures within error_ref's bounds (group sums given exactly: n_max = 1)."""
    K = len(sizes)
    var, rel, fig, _ = host(groups, sizes, batches)
    rvar, scale, vp, mp, bad = ref.reference(groups, sizes, running_sum(groups))
    tol = ref.var_tolerance(scale, K, 1)
    good = ~bad
    assert np.all(np.abs(var[good] - rvar[good]) <= tol[good]), np.max(np.abs(var[good] - rvar[good]) / tol[good])
    assert np.all(var[good] >= 0.0)
    assert np.isnan(var[bad]).all() and np.isnan(rel[bad]).all()
    e, etol = ref.rel_reference(vp, mp, np.where(bad[..., None], 0.0, tol), bad)
    assert np.all(np.abs(rel[good].astype(np.float64) - e[good]) <= etol[good] + 2.0 ** -24 * e[good])
    fe, ftol = ref.frame_reference(e, etol, bad)
    assert fig["nonfinite_pixels"] == int(bad.sum()) and fig["pixels"] == bad.size
    assert fig["groups"] == K and fig["samples"] == sum(sizes)
    if good.any():
        assert abs(fig["frame_error"] - fe) <= ftol
        assert np.float32(fig["max_error"]) == rel[good].max()          # the same pixel's e_p, rounded once
    return var, rel, fig


def random_groups(seed, sizes, lo=0.0, hi=4.0):
    rng = np.random.default_rng(seed)
    n = np.asarray(sizes, dtype=np.float64)[:, None, None, None]
    return rng.uniform(lo, hi, (len(sizes), H, W, 3)) * n


def test_bound_constant():
    # c = K + 2 n_max + 3 (tests/error_ref.py's derivation): exact group sums, K = 4 -> 9
    assert ref.var_c(4, 1) == 9 and ref.var_c(2, 8) == 21


def test_two_groups():
    check(random_groups(1, [4, 4]), [4, 4])


def test_unequal_last_group_over_batches():
    # 22 samples in batches of 8 with chunks of 4: groups 4 4 | 4 4 | 4 2, the last one short
    sizes = [4, 4, 4, 4, 4, 2]
    check(random_groups(2, sizes), sizes, batches=[[0, 1], [2, 3], [4, 5]])
    check(random_groups(3, [5, 5, 3]), [5, 5, 3])


def test_equal_groups_give_zero():
    # dyadic values: every product, quotient and sum is exact, so q == S^2 / N and the variance is exactly 0
    g = np.empty((4, H, W, 3))
    g[:] = np.array([1.5, 0.25, 3.0])
    var, rel, fig = check(g, [4, 4, 4, 4])
    assert np.all(var == 0.0) and np.all(rel == 0.0) and fig["frame_error"] == 0.0 and fig["max_error"] == 0.0
    # any values: the rounding of q - S^2/N may fall either side of zero; the clamp keeps it from going negative
    rng = np.random.default_rng(4)
    g = np.broadcast_to(rng.uniform(0.0, 7.0, (1, H, W, 3)), (3, H, W, 3)).copy()
    var, _, _ = check(g, [3, 3, 3])
    assert np.all(var >= 0.0)
    assert not np.any(np.signbit(var))


@pytest.mark.parametrize("scale", [1e-12, 1e-6, 1.0, 1e6])
def test_magnitudes(scale):
    check(random_groups(5, [8, 8, 8, 6]) * scale, [8, 8, 8, 6])


def test_mixed_magnitudes():
    rng = np.random.default_rng(6)
    g = random_groups(7, [4, 4, 4]) * 10.0 ** rng.uniform(-12, 6, (1, H, W, 1))
    check(g, [4, 4, 4])


def test_nonfinite_partials():
    g = random_groups(8, [4, 4, 3])
    g[1, 2, 3, 0] = np.nan
    g[0, 8, 10, 2] = np.inf
    g[2, 0, 0, 1] = -np.inf
    var, rel, fig = check(g, [4, 4, 3])
    assert fig["nonfinite_pixels"] == 3
    for y, x in ((2, 3), (8, 10), (0, 0)):
        assert np.isnan(var[y, x]).all() and np.isnan(rel[y, x])
    assert math.isfinite(fig["frame_error"]) and math.isfinite(fig["max_error"])


def test_threshold_decision():
    g = random_groups(9, [4, 4])
    _, _, fig, conv = host(g, [4, 4])
    fe = fig["frame_error"]
    assert fe > 0 and not conv                                         # no threshold: never
    assert host(g, [4, 4], threshold=fe)[3]                            # at the threshold: stop
    assert not host(g, [4, 4], threshold=np.nextafter(fe, 0.0))[3]
    assert not host(g, [4, 4], threshold=fe, min_samples=9)[3]         # 8 samples are in
    assert host(g, [4, 4], threshold=fe, min_samples=8)[3]
    g[0, 0, 0, 0] = np.nan                                             # a non-finite pixel is left out of the mean
    assert host(g, [4, 4], threshold=1e9)[3]
    g[:] = np.nan                                                      # no finite pixel: NaN, never converged
    _, _, fig, conv = host(g, [4, 4], threshold=1e9)
    assert math.isnan(fig["frame_error"]) and not conv


def test_unbiased_with_unequal_groups():
    """E[B / (K - 1)] = sigma^2 whatever the group sizes: exponential samples (sigma^2 = 1), groups of 4, 4, 4, 3.  The
    mean of the estimates over the trials lies within 4 of its standard errors (from the trials themselves) of 1."""
    sizes = [4, 4, 4, 3]
    N, K = sum(sizes), len(sizes)
    rng = np.random.default_rng(12345)
    trials = 20000
    x = rng.exponential(1.0, (trials, N))
    edges = np.cumsum([0] + sizes)
    S_c = np.stack([x[:, a:b].sum(axis=1) for a, b in zip(edges[:-1], edges[1:])], axis=1)
    B = (S_c ** 2 / np.asarray(sizes)).sum(axis=1) - x.sum(axis=1) ** 2 / N
    est = B / (K - 1)
    se = est.std(ddof=1) / math.sqrt(trials)
    assert abs(est.mean() - 1.0) <= 4 * se, (est.mean(), se)
    # the same through the CPU build: a 50 x 40 frame's 6000 channels are 6000 trials; var_mean * N = sigma^2's estimate
    h, w = 40, 50
    x = rng.exponential(1.0, (N, h, w, 3))
    g = np.stack([x[a:b].sum(axis=0) for a, b in zip(edges[:-1], edges[1:])])
    q = eb.host_moments(np.zeros((h, w, 3)), g, 4, N)
    var, _, _, _ = eb.host_estimate(running_sum(g), q, K, N)
    est = (var * N).ravel()
    se = est.std(ddof=1) / math.sqrt(est.size)
    assert abs(est.mean() - 1.0) <= 4 * se, (est.mean(), se)


def test_host_bodies_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/sanitize/error_main.cpp, its own main) over the CPU build of the bodies, linked with
    ASan and UBSan: ragged frames, short last chunks, exactly-sized buffers."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "error_main")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O1", "-g", "-std=c++17",
                    "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(os.path.dirname(here), "include"), os.path.join(here, "sanitize", "error_main.cpp"),
                    "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.count(" ok") == 6
