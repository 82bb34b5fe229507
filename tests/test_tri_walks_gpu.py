"""The device's triangle, box and plane hits against tests/prim_ref.py (the NumPy restatement of the reference's
World.hit over all five primitives) on the scene families and ray classes of tests/test_tri_walks.py: rt_closest_hits,
rt_occluded and renders under the knobs that choose the triangle tree's kernel, each knob set in one child process
(the trace-kernel choices are read once per process).  RT_LDS_TRI runs ACC_BVH_TRI_LDS, the triangle tree's top levels
in LDS, and RT_TRI_LDS_NODES=64 makes every walk cross from the LDS prefix into global memory."""
import numpy as np
import pytest

import guidedcheck_binding as gb
import hostcheck_binding as hb
import lightcheck_binding as lb
import prim_ref as pr
import test_tri_walks as cpu
from blenderraytracer_amd import capi
from test_gpu_parity import _render_in_child, rel_err

pytestmark = pytest.mark.gpu

SCENES = cpu.SCENES
RENDERED = cpu.RENDERED

_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (HIP runtime first)
import test_tri_walks as cpu
from blenderraytracer_amd import capi
from test_gpu_parity import _closest_hits
from test_lights_gpu import _occluded
lib = capi.load_library()
inp = np.load(sys.argv[2][:-len("out.npz")] + "in.npz")
out = {}
F64, F32, BRUTE, BVH = capi.RT_PREC_F64, capi.RT_PREC_F32, capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH
for name in cpu.SCENES:
    rays, t = inp[name + ".rays"], inp[name + ".t"]
    rt = cpu.tracer(name)
    for prec, pn in ((F64, "f64"), (F32, "f32")):
        for accel, an in ((BRUTE, "brute"), (BVH, "bvh")):
            ht, hk, hi = _closest_hits(rt, rays, prec, accel)
            out[f"{name}.{pn}.{an}.t"], out[f"{name}.{pn}.{an}.kind"], out[f"{name}.{pn}.{an}.idx"] = ht, hk, hi
    for accel, an in ((BRUTE, "brute"), (BVH, "bvh")):
        for j, lim in enumerate((t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf))):
            out[f"{name}.occ.{an}.{j}"] = _occluded(lib, rt, rays, lim, F64, accel)
    out[name + ".walk"] = np.array([lib.rt_scene_walk(rt.scene_handle(), F64, a) for a in (capi.RT_ACCEL_AUTO, BRUTE, BVH)])
    if name in cpu.RENDERED:
        rt.accel = BVH
        full = rt.render(want=("mean", "segments", "draws"))
        plain = rt.render(want=("mean",))                    # the kernels without counting
        for k in ("mean", "segments", "draws", "rgba8"):
            out[f"{name}.render.{k}"] = full[k]
        out[name + ".render.plain"] = plain["mean"]
    rt.close()
for accel, an in ((BRUTE, "brute"), (BVH, "bvh")):
    rt = cpu.lit_torus(accel=accel)
    r = rt.render(want=("mean", "segments", "draws"))
    for k in ("mean", "segments", "draws"):
        out[f"lit.{an}.{k}"] = r[k]
    rt.close()
np.savez(sys.argv[2], **out)
'''

# knob set -> (the environment, the same knobs for hb.kernel_choice, the kernel torus' render takes: pt_core.h enum Accel)
KNOBS = {"default": ({}, {}, cpu.BVH_STACK_LEAN),
         "skip": ({"RT_BVH_WALK": "skip"}, {"bvh_walk": "skip"}, 2),
         "general": ({"RT_LEAN": "0"}, {"lean": 0}, cpu.BVH_STACK),
         "tri_lds": ({"RT_LDS_TRI": "1"}, {"lds_tri": 1}, cpu.BVH_TRI_LDS),
         "tri_lds_64": ({"RT_LDS_TRI": "2", "RT_TRI_LDS_NODES": "64"}, {"lds_tri": 2, "tri_lds_nodes": 64}, cpu.BVH_TRI_LDS)}

_host = {}


def host(key, make):
    """CPU-side results shared by the knob sets (computed once, never changed)"""
    if key not in _host:
        _host[key] = make()
    return _host[key]


_children = {}


@pytest.fixture
def child(gpu, tmp_path_factory):
    """knobs -> the results of the child process that ran _CHILD under that knob set.  Each knob set starts at most
    one child per session: a child that failed (a fault, an abort, the time limit) is not started again; every test
    of that knob set fails with the first child's error."""
    def run(knobs):
        if knobs not in _children:
            try:
                d = tmp_path_factory.mktemp("tri_walks_" + knobs)
                np.savez(d / "in.npz", **{f"{n}.{k}": cpu.family(n)[k] for n in SCENES for k in ("rays", "t")})
                _children[knobs] = _render_in_child(_CHILD, d / "out.npz", **KNOBS[knobs][0])
            except BaseException as e:          # AssertionError of the child's exit status, TimeoutExpired, ...
                _children[knobs] = e
                raise
        if isinstance(_children[knobs], BaseException):
            raise AssertionError(f"the child of knob set {knobs!r} failed earlier in this session") from _children[knobs]
        return _children[knobs]
    return run


def well_conditioned(f):
    """The binary32 subset: `threshold` rays at 10 times the threshold, aimed at a triangle's centroid (no vertex or
    edge in reach) from 30 degrees or more above its plane (the mode that sets |d|, labels below 4)."""
    return (f["cls"] == pr.RAY_CLASSES.index("threshold")) & (f["label"] == 3) & (f["target"] >= 0)


# (tiny's subset starts as near as tMin allows, prim_ref._threshold_rays: from farther away binary32 rounds the origin
# and the direction by more than its triangles' 10^-4)
F32_SUBSET = tuple(s for s in SCENES if s != "cornell.json")      # cornell.json has no triangle


@pytest.mark.parametrize("knobs", list(KNOBS))
def test_device_hit_queries_equal_the_reference(child, knobs):
    """rt_closest_hits and rt_occluded, binary64, World order and the knob's walk, every family and ray class:
    prim_ref.world_hit's t (bit for bit), kind and index, and prim_ref.occluded's verdict for limits at the hit's t,
    the next double above and the next below, mismatches counted per ray class; select_kernel under the same knobs
    names the kernel the knob set is for.  Binary32 has no exactness proof: the tree walk must agree with World order
    (kind, index) on the well-conditioned subset only; every class's agreement is printed (DESIGN.md §4 records it)."""
    res = child(knobs)
    env, kw, acc = KNOBS[knobs]
    assert hb.kernel_choice(cpu.tracer("torus").packed(), capi.RT_PREC_F64, True, **kw)["acc"] == acc
    for name in SCENES:
        f = cpu.family(name)
        for an in ("brute", "bvh"):
            t, kind, idx = (res[f"{name}.f64.{an}.{k}"] for k in ("t", "kind", "idx"))
            assert cpu._mismatch(f, t, kind, idx) == {}, (name, an)
            for j, lim in enumerate(cpu._tmax3(f["t"])):
                bad = res[f"{name}.occ.{an}.{j}"] != cpu.ref_occluded(name, j)
                assert not bad.any(), (name, an, j, {c: int(bad[f["cls"] == k].sum()) for k, c in enumerate(cpu.CLASSES)})
        # rt_scene_walk: 0 World order, 1 a tree walk, 2 the grid
        auto, brute, bvh = res[name + ".walk"]
        assert brute == 0
        if name in pr.FAMILIES:
            assert bvh == 1, name
        h32 = host(("f32", name), lambda: gb.host_closest_hits(f["rt"].packed(), capi.RT_PREC_F32, capi.RT_ACCEL_BRUTE, f["rays"]))
        same = (res[f"{name}.f32.brute.kind"] == res[f"{name}.f32.bvh.kind"]) & (res[f"{name}.f32.brute.idx"] == res[f"{name}.f32.bvh.idx"])
        shares = {c: round(float(same[f["cls"] == k].mean()), 4) for k, c in enumerate(cpu.CLASSES)}
        subset = well_conditioned(f)
        kept = subset & (h32[1] == f["kind"]) & (np.where(h32[1] >= 0, h32[2], -1) == f["idx"])
        print(f"f32 {knobs} {name}: subset kept {kept.sum()}/{subset.sum()}; BVH == World order (kind, index) per class: {shares}")
        if name in F32_SUBSET:
            assert subset.sum() >= 100
            assert kept.sum() >= 0.9 * subset.sum(), (name, int(kept.sum()), int(subset.sum()))
            assert same[kept].all(), (name, int((~same[kept]).sum()))


@pytest.mark.parametrize("name", RENDERED)
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_device_render_matches_oracle(child, knobs, name):
    """76 x 45, 4 spp, depth 5, binary64, RT_ACCEL_BVH under the knob set: the C oracle's segments, draws and RGBA8,
    means within the summation-order bound (1e-12 relative); the non-counting kernels give the counting kernels'
    bits.  torus, bowl and pair are where a reflected ray must meet the mesh again (a wrong exit bound drops the hit),
    lattice where coincident triangles tie (tri_mat[idx] after the walk)."""
    res = child(knobs)
    o = cpu.oracle_render(name)
    seg, drw = res[name + ".render.segments"], res[name + ".render.draws"]
    print(f"{knobs} {name}: segments differ in {int((seg != o['segments']).sum())} pixels, draws in {int((drw != o['draws']).sum())}")
    assert np.array_equal(seg, o["segments"])
    assert np.array_equal(drw, o["draws"])
    assert np.array_equal(res[name + ".render.rgba8"], o["rgba8"])
    assert rel_err(res[name + ".render.mean"], o["mean"]) <= 1e-12
    assert np.array_equal(lb.bits(res[name + ".render.mean"]), lb.bits(res[name + ".render.plain"]))


@pytest.mark.parametrize("knobs", list(KNOBS))
def test_device_lit_render_under_a_vertical_sun(child, knobs):
    """torus, 76 x 45, 2 spp, one directional light straight down (every shadow ray has two zero components and goes
    through the triangle tree's any-hit walk): the tree gives World order's bits; World order gives the CPU build's
    segments and draws, means within 1e-12."""
    res = child(knobs)
    assert np.array_equal(lb.bits(res["lit.bvh.mean"]), lb.bits(res["lit.brute.mean"]))
    for k in ("segments", "draws"):
        assert np.array_equal(res[f"lit.bvh.{k}"], res[f"lit.brute.{k}"])
    rt = cpu.lit_torus(accel=capi.RT_ACCEL_BRUTE)
    h = host("lit", lambda: lb.host_render(rt.packed(), rt.settings()))
    assert np.array_equal(res["lit.brute.segments"], h["segments"]) and np.array_equal(res["lit.brute.draws"], h["draws"])
    assert rel_err(res["lit.brute.mean"], h["mean"]) <= 1e-12
