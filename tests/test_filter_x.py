"""The expanded binary32 sphere filter of the binary64 lean grid kernel (pt_core.h sphere_filter_x_pass) never
rejects a sphere the binary64 discriminant accepts, stays inside the error bound derived beside it, rejects as
many sure misses as the old filter, and its two obvious mistakes are caught."""
import os
import sys

import pytest

import filterxcheck_binding as fx

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

U = 2.0 ** -24
BOUND = 40 * U        # pt_core.h, the derivation above RT_FILTER_X: |X' - Y - margin| <= 40 u Q (margin 128 u Q)
N = 2_000_000
MODES = {0: "old generator", 1: "|c|/r up to 1e6", 2: "origin on the sphere"}
_runs = {}


def run(mode, mutation=0):
    if (mode, mutation) not in _runs:
        _runs[(mode, mutation)] = fx.filter_check(N, 12345 + mode, mode, mutation)
    return _runs[(mode, mutation)]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_expanded_filter_is_conservative(mode):
    r = run(mode)
    print(f"{MODES[mode]}: violations {r['violations']} (old {r['violations_old']}), worst {r['worst'] / U:.2f} u, "
          f"misses rejected {r['rejected']:.4f} (old {r['rejected_old']:.4f}) of {r['misses']}")
    assert r["violations"] == 0
    assert r["violations_old"] == 0
    assert r["worst"] <= BOUND
    assert r["rejected"] >= 0.99 * r["rejected_old"]


def caught(r):
    return r["violations"] > 0 or r["worst"] > BOUND


def test_k_rounded_down_is_caught():
    r = run(0, 1)
    print(f"k - 64 ulps: violations {r['violations']}, worst {r['worst'] / U:.2f} u")
    assert caught(r)


def test_wrong_sign_is_caught():
    r = run(0, 2)
    print(f"A negated: violations {r['violations']}, worst {r['worst'] / U:.2f} u")
    assert r["violations"] > 0


def test_floor_counts_of_the_lean_walk():
    """bench.py's three crops of config 3 (32 x 32 at 8 spp) through the binary64 lean grid kernel's own walk on the
    CPU (copy_grid_lds<double, true>, make_filter_ray_x on the walk's rays, sphere_records_lds) against the walk the
    floor model has always counted (the old filter; reproduced here and equal to hostcheck_binding.event_counts):
    the same segments, draws, hits, rejection rounds and radiance; filter_tests identical (the dominant spheres keep
    the old form, and every record of a visited cell is filtered once in both); f64_sphere_tests per segment within
    1 % of the old walk's and of DESIGN's 2.358.  (Both figures count the scene set-up's probe rays, once per crop,
    as event_counts does; the walk's own share is printed.)"""
    import hostcheck_binding as hb
    cfg = bench.CONFIGS["rtow"]
    rt = bench.make_tracer(cfg, "f64", 1, 0)
    packed, side = rt.packed(), 32

    def crops():
        sts = []
        for fx_, fy in ((0.5, 0.5), (0.25, 0.7), (0.75, 0.3)):
            st = rt.settings(crop=(int(fx_ * (cfg["w"] - side)), int(fy * (cfg["h"] - side)), side, side))
            st.samples = 8
            sts.append(st)
        return sts
    old, new = fx.work(packed, crops(), False), fx.work(packed, crops(), True)
    ref = hb.event_counts(packed, crops(), "grid")
    seg = old["segments"]
    own = lambda r, k: (r[k] - r["setup"][k]) / seg
    print(f"segments {seg:.0f}; per segment old -> new: filter_tests {old['filter_tests'] / seg:.4f} -> "
          f"{new['filter_tests'] / seg:.4f} (the walk's own {own(old, 'filter_tests'):.4f} -> {own(new, 'filter_tests'):.4f}), "
          f"f64_sphere_tests {old['f64_sphere_tests'] / seg:.4f} -> {new['f64_sphere_tests'] / seg:.4f} "
          f"(own {own(old, 'f64_sphere_tests'):.4f} -> {own(new, 'f64_sphere_tests'):.4f}; counts "
          f"{old['f64_sphere_tests']:.0f} -> {new['f64_sphere_tests']:.0f}), "
          f"sphere rounds {new['sphere_draw_rounds'] / seg:.4f}, disk rounds {new['disk_draw_rounds'] / seg:.4f}")
    assert seg == ref["segments"] > 3 * side * side * 8
    for k in hb.EVENTS:                                        # the old walk here is event_counts' walk
        assert abs(old[k] / seg - ref[k]) < 1e-9, k
    for k in ("segments", "draws", "cells", "sphere_records", "sum", "accept", "miss", "samples", "lambertian", "metal",
              "dielectric", "emissive", "dielectric_schlick", "sphere_draw_rounds", "disk_draw_rounds", "disc_nonneg",
              "second_root", "setup"):
        assert old[k] == new[k], k
    assert new["filter_tests"] == old["filter_tests"] > 0
    assert abs(new["f64_sphere_tests"] / old["f64_sphere_tests"] - 1) <= 0.01
    assert abs(new["f64_sphere_tests"] / seg / 2.358 - 1) <= 0.01
