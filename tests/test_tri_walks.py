"""Triangle, box and plane hits (and the spheres among them) as the kernels compile them, run on the CPU
(tests/hostcheck), against tests/prim_ref.py: a NumPy restatement of the reference's World.hit over all five
primitives that shares no code with them.  Every scene family is built for something the shipped scenes lack
(concave meshes, coincident triangles, degenerate boxes ...) and every ray class is one bvh_rays never makes
(prim_ref's docstrings; DESIGN.md §4 "Triangle, box and plane hits beyond the goldens")."""
import ctypes as C
import functools

import numpy as np
import pytest

import guidedcheck_binding as gb
import hostcheck_binding as hb
import lightcheck_binding as lb
import prim_ref as pr
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
from oracle import binding

SCENES = pr.FAMILIES + ("sample_mesh.json", "kitchen_sink.json", "cornell.json")
RENDERED = tuple(s for s in pr.FAMILIES if s != "tiny")          # tMin = 0.001 swallows tiny's render
PER_CLASS, STRESS = 2000, 2000
CLASSES = pr.RAY_CLASSES + ("stress",)
BVH_STACK, BVH_TRI_LDS, BVH_STACK_LEAN = 3, 8, 10       # csrc/pt_core.h enum Accel (tests/test_walk_select.py)
W, H, SPP, DEPTH = 76, 45, 4, 5                         # ragged in both directions against the 8 x 8 tiles
WALKS = ("world", "two_child", "stackless")


def scene_data(name):
    return load_scene_json(name) if name.endswith(".json") else pr.scene(name)


def tracer(name, w=W, h=H, data=None, **kw):
    rt = GpuRayTracer(w, h, seed=17, **kw)
    assert rt.load_from_json(data or scene_data(name))
    rt.update_render_settings({"samples": SPP, "maxBounces": DEPTH})
    return rt


@functools.lru_cache(maxsize=None)
def family(name):
    """The scene's tracer, rays of every class (prim_ref's and bvh_rays') and the reference's closest hits,
    computed once and shared (read-only) by the tests."""
    rt = tracer(name)
    objects = pr.objects_of(scene_data(name))
    rays, cls, label, target, miss = pr.all_rays(objects, PER_CLASS, 4242, tiny=name == "tiny")
    s = hb.bvh_rays(rt.packed(), STRESS, 99, 0)[0]
    rays = np.ascontiguousarray(np.concatenate([rays, s]))
    cls = np.concatenate([cls, np.full(len(s), len(pr.RAY_CLASSES))])
    label = np.concatenate([label, np.zeros(len(s), dtype=np.int64)])
    target = np.concatenate([target, np.full(len(s), -1)])
    # bvh_rays' directions are of unit scale: on `tiny` they see nothing (|a| < 1e-4 on every triangle)
    miss = np.concatenate([miss, np.full(len(s), pr.MISS_BUILT if name == "tiny" else 0, dtype=np.int8)])
    t, kind, idx = pr.world_hit(objects, rays)
    for a in (rays, cls, label, target, miss, t, kind, idx):
        a.setflags(write=False)
    return {"rt": rt, "objects": objects, "rays": rays, "cls": cls, "label": label, "target": target, "miss": miss,
            "t": t, "kind": kind, "idx": idx}


def hit_shares(name):
    """class -> the share of its rays on which the reference hits, without the two kinds of sub-case that are built to
    miss (prim_ref.MISS_BUILT: `threshold` below 1, unit-scale directions on `tiny`)"""
    f = family(name)
    counted = f["miss"] != pr.MISS_BUILT
    return {c: float(np.mean(f["kind"][(f["cls"] == k) & counted] >= 0)) for k, c in enumerate(CLASSES)
            if ((f["cls"] == k) & counted).any()}


@pytest.mark.parametrize("name", SCENES)
def test_every_ray_class_mostly_hits(name):
    """A class that mostly misses proves little: the reference alone reports a hit on at least 25 % of each class's
    rays in each scene (tests/test_sphere_walks.py's cap).  Two kinds of sub-case are built to miss and are not
    counted: `threshold` below 1 and unit-scale directions on `tiny`.  They, and the `zero` rays in their target's own
    plane (which are counted), must miss the triangle they were aimed at on every ray, and tiny's unit-scale stress
    rays must miss everything."""
    f = family(name)
    shares = hit_shares(name)
    print(name, {c: round(s, 2) for c, s in shares.items()})
    for c, share in shares.items():
        assert share >= 0.25, (name, c, share)
    tris = pr.triangles_of(f["objects"])
    aimed = np.nonzero((f["miss"] > 0) & (f["target"] >= 0))[0]
    assert len(aimed) > 0 or not len(tris)
    for i in np.unique(f["target"][aimed]):
        q = aimed[f["target"][aimed] == i]
        hit, _, _ = pr.tri_hit(tris[i], f["rays"][q])
        assert not hit.any(), (name, int(i), CLASSES[int(f["cls"][q[0]])])
        assert not ((f["kind"][q] == pr.TRI) & (f["idx"][q] == i)).any()
    if name == "tiny":
        assert (f["kind"][f["cls"] == len(pr.RAY_CLASSES)] == -1).all()


def test_threshold_rays_straddle_the_parallel_test():
    """The `threshold` rays sit where they say: |a| of the target triangle is 1e-4 times the sub-case's factor to
    1e-12 relative, so the factors 1 - 1e-9 and 1 + 1e-9 lie on either side of `|a| < 0.0001`: Triangle.hit of the target
    alone misses below 1 and hits above it (the closest hit may still be something nearer)."""
    for name in ("torus", "tiny", "soup"):
        f = family(name)
        tris = pr.triangles_of(f["objects"])
        sel = np.nonzero((f["cls"] == pr.RAY_CLASSES.index("threshold")) & (f["target"] >= 0))[0]
        a = np.array([pr.tri_hit(tris[f["target"][q]], f["rays"][q])[2][0] for q in sel])
        fac = np.array(pr.THRESHOLD_FACTORS)[f["label"][sel] % 4]
        assert np.all(np.abs(np.abs(a) / (1e-4 * fac) - 1) < 1e-12)
        assert (a > 0).any() and (a < 0).any()
        above = fac > 1
        hit = np.array([pr.tri_hit(tris[f["target"][q]], f["rays"][q])[0][0] for q in sel])
        assert hit[above].all() and not hit[fac < 1].any()
        on_target = (f["kind"][sel] == pr.TRI) & (f["idx"][sel] == f["target"][sel])
        print(f"{name}: the closest hit is the target on {on_target[above].mean():.2f} of the rays above the threshold")


def test_lattice_exercises_both_tie_rules():
    """`lattice`: on the axis-aligned rays through its vertices and edges several triangles of one mesh report the
    same t (the reference keeps the last), a standalone triangle placed before the mesh wins over the mesh triangle it
    coincides with, and the first mesh always wins over its coincident copy."""
    f = family("lattice")
    parts = [p for k, p, _ in f["objects"] if k == pr.TRI]
    sizes = [len(p) for p in parts]
    mesh0 = sizes.index(max(sizes))                          # the first mesh among the triangle objects
    first = sum(sizes[:mesh0])
    n_mesh = sizes[mesh0]
    sel = np.nonzero((f["cls"] == pr.RAY_CLASSES.index("axis")) & (f["kind"] == pr.TRI))[0][:400]
    hits = [pr.tri_hit(v, f["rays"][sel])[:2] for v in parts[mesh0]]
    ts = np.array([np.where(ok, t, np.inf) for ok, t in hits])               # triangle x ray
    ties = last_wins = 0
    for k, q in enumerate(sel):
        same = np.nonzero(ts[:, k] == f["t"][q])[0]
        if len(same) >= 2 and first <= f["idx"][q] < first + n_mesh:
            ties += 1
            last_wins += f["idx"][q] == first + same[-1]
    assert ties >= 20 and last_wins == ties, (ties, last_wins)
    hit_tri = f["kind"] == pr.TRI
    assert (hit_tri & (f["idx"] < first)).sum() >= 20                         # a standalone triangle before the mesh
    assert not (hit_tri & (f["idx"] >= first + n_mesh + sum(sizes[mesh0 + 1:-1]))).any()    # never the copy


def test_families_pin_what_they_are_for():
    """torus takes the lean two-child kernel by default; mixed has boxes, so it takes the general one; under lds_tri = 1
    torus takes the triangle tree's LDS kernel; under lds_tri = 2 with 64 staged nodes the tree is larger than the
    prefix, so a walk crosses from LDS nodes to global ones."""
    F64 = capi.RT_PREC_F64
    torus, mixed = tracer("torus").packed(), tracer("mixed").packed()
    assert hb.kernel_choice(torus, F64, True)["acc"] == BVH_STACK_LEAN
    c = hb.kernel_choice(mixed, F64, True)
    assert c["acc"] == BVH_STACK and c["num_boxes"] > 0
    for name in RENDERED:
        p = tracer(name).packed()
        assert hb.kernel_choice(p, F64, True, lds_tri=1)["acc"] == BVH_TRI_LDS, name
        c = hb.kernel_choice(p, F64, True, lds_tri=2, tri_lds_nodes=64)
        assert c["acc"] == BVH_TRI_LDS and c["tri_lds_nodes"] == 64 and c["num_tri_wide"] > 64, (name, c)


def _mismatch(f, t, kind, idx):
    bad = (pr.bits(t) != pr.bits(f["t"])) | (kind != f["kind"]) | (np.where(kind >= 0, idx, -1) != f["idx"])
    return {c: int(bad[f["cls"] == k].sum()) for k, c in enumerate(CLASSES) if bad[f["cls"] == k].any()}


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", SCENES)
def test_walk_equals_world_hit(name, walk):
    """Each walk's closest hit (t bit for bit, kind, and the index within the kind) is prim_ref.world_hit's."""
    f = family(name)
    assert _mismatch(f, *hb.walk_hits_kind(f["rt"].packed(), walk, f["rays"])) == {}


ACCELS = pytest.mark.parametrize("accel", [capi.RT_ACCEL_BVH, capi.RT_ACCEL_BRUTE], ids=["bvh", "brute"])


@ACCELS
@pytest.mark.parametrize("name", SCENES)
def test_host_closest_hits_equal_world_hit(name, accel):
    """rt_closest_hits' code on the CPU (closest_hit_acc), both accels: t (bit for bit), kind and index are world_hit's."""
    f = family(name)
    assert _mismatch(f, *gb.host_closest_hits(f["rt"].packed(), capi.RT_PREC_F64, accel, f["rays"])) == {}


def _tmax3(t):
    """the limit at the hit's t (not occluded), the next double above (occluded) and the next below"""
    return (t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf))


def ref_occluded(name, j):
    """prim_ref.occluded of the family's rays for limit j of _tmax3: world_hit(tMin, inf).t < tmax"""
    f = family(name)
    return f["t"] < _tmax3(f["t"])[j]


@ACCELS
@pytest.mark.parametrize("name", SCENES)
def test_host_occluded_equals_the_reference(name, accel):
    """rt_occluded's code on the CPU (the any-hit walks), both accels: prim_ref.occluded's verdict for limits at the
    hit's t (never occluded), the next double above (occluded) and the next below."""
    f = family(name)
    for j, lim in enumerate(_tmax3(f["t"])):
        want = ref_occluded(name, j)
        occ, by_closest = lb.host_occluded(f["rt"].packed().desc, accel, f["rays"], lim)
        bad = occ != want
        assert not bad.any(), (j, {c: int(bad[f["cls"] == k].sum()) for k, c in enumerate(CLASSES)})
        assert np.array_equal(by_closest, want)


def test_occluded_is_the_documented_rule():
    """prim_ref.occluded restates INTEGRATION.md §8 on its own: it is what ref_occluded reads off the shared hits."""
    f = family("mixed")
    for j, lim in enumerate(_tmax3(f["t"])):
        assert np.array_equal(pr.occluded(f["objects"], f["rays"], lim), ref_occluded("mixed", j))


def rel_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@functools.lru_cache(maxsize=None)
def oracle_render(name):
    rt = tracer(name)
    return binding.render(rt.packed(), rt.settings())


@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH, 3], ids=["brute", "two_child", "stackless"])
@pytest.mark.parametrize("name", RENDERED)
def test_render_matches_oracle(name, accel):
    """76 x 45, 4 spp, depth 5, binary64: trace_pixel through each walk against the C oracle: the same segments
    and draws per pixel, means within the summation-order bound (1e-12 relative, tests/test_gpu_parity.py)."""
    rt = tracer(name)
    rt.accel = accel
    r = hb.render(rt.packed(), rt.settings())
    o = oracle_render(name)
    assert o["segments"].max() > 1, "no pixel's path met anything"
    assert np.array_equal(r["segments"], o["segments"])
    assert np.array_equal(r["draws"], o["draws"])
    assert rel_err(r["mean"], o["mean"]) <= 1e-12


# RT_HCOUNT's events are counted by builds with RT_HOST_COUNTERS; HC_TRI_FILTERS counts the binary32 pre-filter's
# tests, which run only with RT_TRI_FILTER=1 (off by default since the exit skip), so both builds switch it on
COUNTING = ("RT_HOST_COUNTERS=1", "RT_TRI_FILTER=1")
DEFAULT_COUNTING = ("RT_HOST_COUNTERS=1",)               # the shipped configuration: every leaf triangle is an HC_TRI_TESTS event
TRI_FILTERS, TRI_TESTS = hb.EVENTS.index("tri_filter_tests"), hb.EVENTS.index("tri_tests")


@functools.lru_cache(maxsize=None)
def counted_render(name, exit_skip, defines=COUNTING):
    """(render, event counts) of the two-child walk by a counting build with or without the exit skip"""
    L = hb.lib(defines if exit_skip else defines + ("RT_TRI_EXIT=0",))
    L.ptc_host_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    rt = tracer(name)
    rt.accel = capi.RT_ACCEL_BVH
    cnt = (C.c_ulonglong * 16)()
    L.ptc_host_counts(cnt, 1)
    r = hb.render(rt.packed(), rt.settings(), L)
    L.ptc_host_counts(cnt, 1)
    return r, list(cnt)


@pytest.mark.parametrize("name", RENDERED)
def test_exit_skip_is_exercised_and_changes_nothing(name):
    """A build without the exit skip (RT_TRI_EXIT=0) renders identical segments, draws and bits of the mean, which are
    the default build's as well; on the meshes whose reflections leave them (torus, bowl, pair) it runs strictly more
    pre-filter tests (HC_TRI_FILTERS) and no fewer binary64 triangle tests, so the skip fires in the default build's render.
    In the shipped configuration (RT_TRI_FILTER=0: every leaf triangle takes the binary64 test) the same holds of
    HC_TRI_TESTS."""
    (a, ca), (b, cb) = counted_render(name, True), counted_render(name, False)
    rt = tracer(name)
    rt.accel = capi.RT_ACCEL_BVH
    d = hb.render(rt.packed(), rt.settings())
    for r in (a, b):
        assert np.array_equal(r["segments"], d["segments"]) and np.array_equal(r["draws"], d["draws"])
        assert np.array_equal(pr.bits(r["mean"]), pr.bits(d["mean"]))
    print(f"{name}: HC_TRI_FILTERS {ca[TRI_FILTERS]} with the exit skip, {cb[TRI_FILTERS]} without; HC_TRI_TESTS {ca[TRI_TESTS]}, {cb[TRI_TESTS]}")
    assert cb[TRI_FILTERS] >= ca[TRI_FILTERS] > 0 and cb[TRI_TESTS] >= ca[TRI_TESTS]
    if name in ("torus", "bowl", "pair"):
        assert cb[TRI_FILTERS] > ca[TRI_FILTERS]
    # the shipped configuration (no pre-filter): the same renders, and the skip saves binary64 triangle tests
    (a, ca), (b, cb) = counted_render(name, True, DEFAULT_COUNTING), counted_render(name, False, DEFAULT_COUNTING)
    for r in (a, b):
        assert np.array_equal(r["segments"], d["segments"]) and np.array_equal(r["draws"], d["draws"])
        assert np.array_equal(pr.bits(r["mean"]), pr.bits(d["mean"]))
    print(f"{name}: without the pre-filter HC_TRI_TESTS {ca[TRI_TESTS]} with the exit skip, {cb[TRI_TESTS]} without")
    assert ca[TRI_FILTERS] == cb[TRI_FILTERS] == 0 and cb[TRI_TESTS] >= ca[TRI_TESTS] > 0
    if name in ("torus", "bowl", "pair"):
        assert cb[TRI_TESTS] > ca[TRI_TESTS]


SUN = {"type": "directional", "direction": [0, -1, 0], "intensity": 1.0}


def lit_torus(**kw):
    """torus under a directional light straight down: every shadow ray has two zero components"""
    data = dict(pr.scene("torus"), lights=[SUN])
    rt = GpuRayTracer(W, H, seed=17, direct_lighting=True, **kw)
    assert rt.load_from_json(data)
    rt.update_render_settings({"samples": 2, "maxBounces": DEPTH, "directLighting": True})
    return rt


def test_lit_render_bvh_equals_brute():
    """The lit torus: the triangle tree's any-hit walk gives World order's bits."""
    out = {}
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt = lit_torus(accel=accel)
        assert rt.packed().num_lights == 1
        out[accel] = lb.host_render(rt.packed(), rt.settings())
    a, b = out[capi.RT_ACCEL_BRUTE], out[capi.RT_ACCEL_BVH]
    assert np.array_equal(a["segments"], b["segments"]) and np.array_equal(a["draws"], b["draws"])
    assert np.array_equal(lb.bits(a["mean"]), lb.bits(b["mean"]))
    assert a["mean"].max() > 0
