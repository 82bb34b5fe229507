"""scripts/wave_census.py (DEV TOOL): the pool loop's schedule replayed on the CPU, per-phase SIMT and ideal slots.
Structure only — the figures themselves are DESIGN.md §8.0's, from the script's default 90 tiles: here 6 tiles of
config 3 in 6-sample chunks."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench  # noqa: E402
import wave_census as wc  # noqa: E402


@pytest.fixture(scope="module")
def census():
    return wc.census(wc.spread_tiles(bench.CONFIGS["rtow"], 80, 66), chunk=6, defer=16)


def test_census_structure(census):
    c, e = census, census["extra"]
    assert c["tiles"] == 6 and e["segments"] > 6 * 64 * 6 and e["iterations"] > 0
    assert e["mismatches"] == 0                                   # the stepped walk finds the kernel's closest hits
    assert (c["ideal"] <= c["simt"] * (1 + 1e-12)).all()          # a sum over 64 lanes / 64 never exceeds the maximum
    assert 0.35 <= wc.efficiency(c, wc.EVENT_WALK, wc.SHADING, wc.REGEN) <= 0.55
    assert 0.2 <= wc.efficiency(c, wc.STEPPED) <= 0.6
    assert 32 <= e["active"] / e["iterations"] <= 64


def test_rejection_trips(census):
    """the wave runs the slowest lane's rounds: mean trips at or above mean rounds; sharing never adds trips, and a
    plain first trip never beats sharing from the start"""
    e = census["extra"]
    it = e["iterations"]
    assert e["requesters"] > 0
    assert e["trips_now"] / it >= e["rounds"] / e["requesters"] >= 1.0
    assert e["trips_all_shared"] <= e["trips_first_plain"] <= e["trips_now"]
    assert e["shared_all_shared"] <= e["trips_all_shared"] and e["shared_first_plain"] <= e["trips_first_plain"]


def test_report_names_every_phase(census):
    text = wc.report(census)
    for name, _ in wc.PHASES:
        assert name in text
    assert "every trip shared" in text and "first trip plain, then shared" in text
