"""The sphere walks (World order, the two-child and the stackless tree walk, the uniform grid in its three forms)
as the kernels compile them, run on the CPU (tests/hostcheck), against tests/sphere_ref.py: a NumPy restatement of
the reference's World.hit that shares no code with them.  Every scene family fixes a scale-dependent part of
build_grid or of a walk to another value than RTOW does, and every ray class is one bvh_rays never makes
(sphere_ref's docstrings; DESIGN.md §4 "Sphere walks beyond RTOW")."""
import copy
import functools

import numpy as np
import pytest

import guidedcheck_binding as gb
import hostcheck_binding as hb
import lightcheck_binding as lb
import sphere_ref as sr
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
from oracle import binding

SCENES = sr.FAMILIES + ("rtow.json",)
PER_CLASS = {"many": 600}            # rays per class (default 2000); `many`: 6,000 spheres per reference ray
STRESS = {"many": 400}               # bvh_rays on top (default 2000)
CLASSES = sr.RAY_CLASSES + ("stress",)
BVH_SPHERES, GRID, GRID_LDS_LEAN = 4, 6, 9      # csrc/pt_core.h enum Accel (tests/test_walk_select.py)
W, H, SPP, DEPTH = 76, 45, 4, 5     # ragged in both directions against the 8 x 8 tiles


def scene_data(name):
    return load_scene_json(name) if name.endswith(".json") else sr.scene(name)


def tracer(name, w=W, h=H, **kw):
    rt = GpuRayTracer(w, h, seed=17, **kw)
    assert rt.load_from_json(scene_data(name))
    rt.update_render_settings({"samples": SPP, "maxBounces": DEPTH})
    return rt


@functools.lru_cache(maxsize=None)
def family(name, per_class=None, stress=None):
    """The scene's tracer, rays of every class (sphere_ref's and bvh_rays') and the reference's closest hits,
    computed once and shared (read-only) by the tests."""
    rt = tracer(name)
    centers, radii = sr.spheres_of(scene_data(name))
    grid = hb.grid_geometry(rt.packed())
    rays, cls, label = sr.all_rays(centers, radii, per_class or PER_CLASS.get(name, 2000), 4242, grid)
    s = hb.bvh_rays(rt.packed(), stress or STRESS.get(name, 2000), 99, 0)[0]
    rays = np.ascontiguousarray(np.concatenate([rays, s]))
    cls = np.concatenate([cls, np.full(len(s), len(sr.RAY_CLASSES))])
    label = np.concatenate([label, np.zeros(len(s), dtype=np.int64)])
    t, idx = sr.world_hit(centers, radii, rays)
    for a in (rays, cls, label, t, idx):
        a.setflags(write=False)
    return {"rt": rt, "centers": centers, "radii": radii, "grid": grid, "rays": rays, "cls": cls, "label": label,
            "t": t, "idx": idx}


@pytest.mark.parametrize("name", SCENES)
def test_every_ray_class_mostly_hits(name):
    """A class that mostly misses proves little: the reference alone reports a hit on at least 25 % of each
    class's rays in each scene."""
    f = family(name)
    for k, c in enumerate(CLASSES):
        share = float(np.mean(f["idx"][f["cls"] == k] >= 0))
        print(f"{name} {c}: {share:.2f} hit")
        assert share >= 0.25, (name, c, share)


def test_families_pin_what_they_are_for():
    """flat takes the lean LDS grid by default; many fits neither the grid nor the sphere tree into LDS, so
    RT_BVH_WALK=grid runs the global grid in both precisions; clump has a cell beyond sphere_records_lds' 32
    records; offset registers more than cloud (margin and pad scale with B); far's camera is beyond grid_far."""
    F64, F32 = capi.RT_PREC_F64, capi.RT_PREC_F32
    p = {n: tracer(n).packed() for n in ("flat", "many", "clump", "offset", "cloud", "far")}
    c = hb.kernel_choice(p["flat"], F64, True)
    assert c["use_grid"] == 1 and (c["acc"], c["walk"]) == (GRID_LDS_LEAN, 2)
    for prec in (F64, F32):
        g = hb.kernel_choice(p["many"], prec, True, bvh_walk="grid")
        assert (g["acc"], g["lds"], g["walk"]) == (GRID, 0, 2)
        t = hb.kernel_choice(p["many"], prec, True, bvh_walk="tree")
        assert (t["acc"], t["lds"], t["walk"]) == (BVH_SPHERES, 0, 1)
    assert hb.grid_geometry(p["clump"])["largest"] > 32
    regs = {n: hb.kernel_choice(p[n], F64, True)["grid_lds_bytes"] for n in ("cloud", "offset")}
    assert regs["offset"] > regs["cloud"]
    far = scene_data("far")["camera"]["position"]
    assert max(abs(x) for x in far) > hb.grid_geometry(p["far"])["far"] > 0


def _mismatch(f, t, idx):
    bad = (sr.bits(t) != sr.bits(f["t"])) | (idx != f["idx"])
    return {c: int(bad[f["cls"] == k].sum()) for k, c in enumerate(CLASSES) if bad[f["cls"] == k].any()}


@pytest.mark.parametrize("walk", hb.WALKS)
@pytest.mark.parametrize("name", SCENES)
def test_walk_equals_world_hit(name, walk):
    """Each walk's closest hit, t bit for bit and the sphere's World-order index, is sphere_ref.world_hit's."""
    f = family(name)
    res = hb.walk_hits(f["rt"].packed(), walk, f["rays"])
    assert res is not None, "the family has no grid"
    assert _mismatch(f, *res) == {}


@functools.lru_cache(maxsize=None)
def ref_occluded(name, j):
    """sphere_ref.occluded of the family's rays for limit j of _tmax3 (shared by both accels, read-only)"""
    f = family(name)
    v = sr.occluded(f["centers"], f["radii"], f["rays"], _tmax3(f["t"])[j])
    v.setflags(write=False)
    return v


def _tmax3(t):
    """the limit at the hit's t (not occluded), the next double above (occluded) and the next below"""
    return (t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf))


@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BVH, capi.RT_ACCEL_BRUTE], ids=["bvh", "brute"])
@pytest.mark.parametrize("name", SCENES)
def test_host_closest_hits_equal_world_hit(name, accel):
    """rt_closest_hits' code on the CPU (closest_hit_acc), both accels: t (bit for bit) and index are world_hit's."""
    f = family(name)
    t, kind, idx = gb.host_closest_hits(f["rt"].packed(), capi.RT_PREC_F64, accel, f["rays"])
    assert _mismatch(f, t, idx) == {}
    assert np.array_equal(kind >= 0, f["idx"] >= 0)


@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BVH, capi.RT_ACCEL_BRUTE], ids=["bvh", "brute"])
@pytest.mark.parametrize("name", SCENES)
def test_host_occluded_equals_the_reference(name, accel):
    """rt_occluded's code on the CPU (the any-hit walks), both accels: sphere_ref.occluded's verdict for limits
    at the hit's t (never occluded), the next double above (occluded) and the next below."""
    f = family(name)
    for j, lim in enumerate(_tmax3(f["t"])):
        want = ref_occluded(name, j)
        occ, by_closest = lb.host_occluded(f["rt"].packed().desc, accel, f["rays"], lim)
        bad = occ != want
        assert not bad.any(), {c: int(bad[f["cls"] == k].sum()) for k, c in enumerate(CLASSES)}
        assert np.array_equal(by_closest, want)


def rel_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@functools.lru_cache(maxsize=None)
def oracle_render(name):
    rt = tracer(name)
    return binding.render(rt.packed(), rt.settings())


@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH, 3, 4], ids=["brute", "two_child", "stackless", "grid"])
@pytest.mark.parametrize("name", [s for s in SCENES if s not in ("tiny", "far")])
def test_render_matches_oracle(name, accel):
    """76 x 45, 4 spp, depth 5, binary64: trace_pixel through each walk against the C oracle: the same segments
    and draws per pixel, means within the summation-order bound (1e-12 relative, tests/test_gpu_parity.py)."""
    rt = tracer(name)
    assert int(np.prod(hb.grid_geometry(rt.packed())["n"])) > 0
    rt.accel = accel
    r = hb.render(rt.packed(), rt.settings())
    o = oracle_render(name)
    assert np.array_equal(r["segments"], o["segments"])
    assert np.array_equal(r["draws"], o["draws"])
    assert rel_err(r["mean"], o["mean"]) <= 1e-12


LIGHTS = {"sun": {"type": "directional", "direction": [0, -1, 0], "intensity": 1.0},
          "point_above_centre": {"type": "point", "position": [4, 9, 0], "intensity": 60.0}}   # RTOW's sphere at (4, 1, 0)


def lit_rtow(light, **kw):
    data = copy.deepcopy(load_scene_json("rtow.json"))
    data["lights"] = [LIGHTS[light]]
    rt = GpuRayTracer(96, 54, seed=17, direct_lighting=True, **kw)
    assert rt.load_from_json(data)
    rt.update_render_settings({"samples": 2, "maxBounces": DEPTH, "directLighting": True})
    return rt


@pytest.mark.parametrize("light", list(LIGHTS))
def test_lit_render_bvh_equals_brute(light):
    """A sun straight down (every shadow ray has two zero components) and a point light exactly above a sphere's
    centre: the lit render through the trees gives World order's bits."""
    out = {}
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt = lit_rtow(light, accel=accel)
        assert rt.packed().num_lights == 1
        out[accel] = lb.host_render(rt.packed(), rt.settings())
    a, b = out[capi.RT_ACCEL_BRUTE], out[capi.RT_ACCEL_BVH]
    assert np.array_equal(a["segments"], b["segments"]) and np.array_equal(a["draws"], b["draws"])
    differ = np.any(lb.bits(a["mean"]) != lb.bits(b["mean"]), axis=-1)
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} pixels differ"
    assert a["mean"].max() > 0
