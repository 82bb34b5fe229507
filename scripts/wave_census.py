"""Wave-level lane census of the binary64 lean grid kernel's pool loop (DEV TOOL): the schedule of
pt_trace.hip's pool_item replayed on the CPU for a few tiles of config 3 over the kernel's own per-lane code
(tests/hostcheck/wave_census.cpp).  Per phase: the slots the wave spends as SIMT runs it (the slowest lane's count
per loop trip), the ideal (all lanes' counts / 64) and their ratio, the lane efficiency the phase can reach; then the
rejection loop of random_in_unit_sphere: today's trips per iteration and the trips when the wave shares the rounds
(RT_COOP_SPHERE).  Nothing on the GPU reads this.
usage: python scripts/wave_census.py [chunk samples = 45] [RT_DEFER_REGEN = 16] [tile step x = 24] [tile step y = 16]
(the defaults: 10 x 9 tiles spread over the frame, 45-sample chunks as the frame's launch cuts them)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from blenderraytracer_amd import capi  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostcheck", "wave_census.cpp")
DEPS = [SRC, os.path.join(ROOT, "include", "rt_hip.h")] + [
    os.path.join(ROOT, "blenderraytracer_amd", "csrc", f) for f in ("pt_core.h", "pt_path.h", "scene_pack.h", "js_math.h")]
LIB = os.path.join(ROOT, "tests", "hostcheck", "_build", "libwave_census.so")

F = bench.FLOOR_COST
# One event of each phase in VALU slots: bench.py's FLOOR_COST where the floor model has the event (a sample's set-up
# without its lens-disk round, which is a phase of its own).  The stepped walk's own terms are this model's: the ray
# set-up before the walk and the grid entry (slabs, first cell) at 40 each, a cell step at the floor's 12 + 2 of loop,
# a survivor's binary64 test at the floor's 36 + 4 for fetching its record.
PHASES = [
    # by events: the walk
    ("cells", F["walk_step_grid"]), ("filter tests", F["filter_tests"]), ("f64 tests", F["f64_sphere_tests"]),
    ("disc >= 0", F["disc_nonneg"]), ("second root", F["second_root"]),
    # shading
    ("hit record", F["hit"]), ("rejection trips", F["sphere_draw_rounds"]), ("normalize", F["segment"]),
    ("lambertian", F["lambertian"]), ("metal", F["metal"]), ("dielectric", F["dielectric"]),
    ("schlick", F["dielectric_schlick"]), ("miss", F["miss"]),
    # regeneration
    ("regeneration", F["samples"] - F["disk_draw_rounds"]), ("disk trips", F["disk_draw_rounds"]),
    # the stepped walk
    ("ray set-up", 40), ("dominant: filter", F["filter_tests"]), ("dominant: f64", F["f64_sphere_tests"]),
    ("dominant: disc", F["disc_nonneg"]), ("dominant: root2", F["second_root"]), ("grid entry", 40),
    ("cell steps", F["walk_step_grid"] + 2), ("filter trips", F["filter_tests"]), ("survivor: f64", F["f64_sphere_tests"] + 4),
    ("survivor: disc", F["disc_nonneg"]), ("survivor: root2", F["second_root"]),
]
EVENT_WALK, SHADING, REGEN, STEPPED = slice(0, 5), slice(5, 13), slice(13, 15), slice(15, 26)
EXTRA = ["iterations", "active", "waiting", "regens", "regen_lanes", "segments", "requesters", "rounds", "trips_now",
         "trips_all_shared", "shared_all_shared", "trips_first_plain", "shared_first_plain", "disk_trips_now", "max_steps",
         "lane_steps", "entered", "mismatches"]


def build():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = "%s.tmp%d" % (LIB, os.getpid())
    subprocess.check_call([hipcc, "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-DRT_HOST_COUNTERS=1", "-I", os.path.join(ROOT, "include"), SRC, "-o", tmp])
    os.replace(tmp, LIB)
    return LIB


def spread_tiles(cfg, step_x=24, step_y=16):
    """top-left pixels of full tiles spread over the frame: every step_x-th tile column from the 4th, every step_y-th
    tile row from the 3rd (config 3: 10 x 9 tiles)"""
    return np.array([[x * 8, y * 8] for y in range(3, cfg["h"] // 8, step_y) for x in range(4, cfg["w"] // 8, step_x)],
                    dtype=np.int32)


def census(tiles, chunk=45, defer=16, config="rtow"):
    """dict: per phase name (SIMT slots, ideal slots), "extra": the counts of EXTRA"""
    cfg = bench.CONFIGS[config]
    rt = bench.make_tracer(cfg, "f64", 1, 0)
    packed, st = rt.packed(), rt.settings()
    L = C.CDLL(build())
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.wcs_census.argtypes = [C.POINTER(capi.SceneDesc), C.POINTER(capi.Settings), C.c_int, ip, C.c_int, C.c_int, dp, dp, dp]
    tiles = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 2)
    cost = np.array([c for _, c in PHASES], dtype=np.float64)
    out, extra = np.zeros(2 * len(PHASES)), np.zeros(len(EXTRA))
    rc = L.wcs_census(C.byref(packed.desc), C.byref(st), len(tiles), tiles.ctypes.data_as(ip), chunk, defer,
                      cost.ctypes.data_as(dp), out.ctypes.data_as(dp), extra.ctypes.data_as(dp))
    assert rc == 0, rc
    n = len(PHASES)
    return {"simt": out[:n], "ideal": out[n:], "extra": dict(zip(EXTRA, extra)), "tiles": len(tiles), "chunk": chunk,
            "defer": defer}


def efficiency(c, *parts):
    """ideal / SIMT over the phases of the given slices"""
    return sum(c["ideal"][p].sum() for p in parts) / sum(c["simt"][p].sum() for p in parts)


def report(c):
    e = c["extra"]
    it = e["iterations"]
    lines = [f"tiles {c['tiles']}, chunk {c['chunk']} samples, RT_DEFER_REGEN {c['defer']}: {int(e['segments'])} segments, "
             f"{int(it)} wave iterations, {e['active'] / it:.1f} lanes trace and {e['waiting'] / it:.2f} wait per iteration; "
             f"stepped walk against the kernel's: {int(e['mismatches'])} mismatches"]
    stepped_total = sum(c["simt"][p].sum() for p in (STEPPED, SHADING, REGEN))

    def table(title, parts, total):
        lines.append(f"-- {title}: slots per iteration (SIMT, ideal), share of the view's SIMT slots, efficiency")
        for p in parts:
            for (name, _), a, b in zip(PHASES[p], c["simt"][p], c["ideal"][p]):
                lines.append(f"{name:18s} {a / it:8.1f} {b / it:8.1f}   {a / total:6.3f}   {b / a if a else 0:5.2f}")

    by_events = sum(c["simt"][p].sum() for p in (EVENT_WALK, SHADING, REGEN))
    table("by events (each event's maximum over the lanes)", (EVENT_WALK, SHADING, REGEN), by_events)
    lines.append(f"overall ideal / SIMT {efficiency(c, EVENT_WALK, SHADING, REGEN):.3f}   ({by_events / it:.0f} slots per iteration)")
    table("stepped walk (cell by cell), with the same shading and regeneration", (STEPPED,), stepped_total)
    lines.append(f"grid walk alone, stepped: ideal / SIMT {efficiency(c, STEPPED):.3f}   ({c['simt'][STEPPED].sum() / it:.0f} slots per iteration); "
                 f"with shading and regeneration {efficiency(c, STEPPED, SHADING, REGEN):.3f} ({stepped_total / it:.0f})")
    lines.append(f"cell steps: {e['max_steps'] / it:.2f} per iteration, {e['lane_steps'] / e['active']:.2f} per lane; "
                 f"{e['entered'] / e['active']:.3f} of the queries enter the grid")
    lines.append(f"regeneration: {e['regens'] / it:.3f} per iteration for {e['regen_lanes'] / max(e['regens'], 1):.1f} lanes, "
                 f"{e['disk_trips_now'] / max(e['regens'], 1):.2f} disk trips each")
    lines.append(f"-- random_in_unit_sphere per iteration: {e['requesters'] / it:.1f} lanes need a point, "
                 f"{e['rounds'] / max(e['requesters'], 1):.2f} rounds each")
    lines.append(f"{'scheme':34s} trips   of them shared")
    lines.append(f"{'today (each lane its own loop)':34s} {e['trips_now'] / it:5.2f}   -")
    lines.append(f"{'every trip shared':34s} {e['trips_all_shared'] / it:5.2f}   {e['shared_all_shared'] / it:5.2f}")
    lines.append(f"{'first trip plain, then shared':34s} {e['trips_first_plain'] / it:5.2f}   {e['shared_first_plain'] / it:5.2f}")
    return "\n".join(lines)


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    chunk, defer, step_x, step_y = (a + [45, 16, 24, 16][len(a):])[:4]
    print(report(census(spread_tiles(bench.CONFIGS["rtow"], step_x, step_y), chunk, defer)))
