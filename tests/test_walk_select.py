"""The one kernel selection of every trace launch (csrc/kernel_select.h select_kernel), pinned on the CPU through
tests/hostcheck: the committed scenes staged exactly as rt_scene_create stages them, both precisions, BVH on and
off, the default knobs and the A/B knobs.  Every expected value is a rule the sources state (kernel_select.h's
comments, DESIGN.md §0 item 4 for the lean kernels, §4 for the textured and lit kernels), cited beside its case;
where the outcome hangs on the host's sampled grid-versus-tree estimate (choose_walk) the rule is asserted given
use_grid.  The GPU tier sees the same function: rt_scene_walk and every launch_trace* report and run its choice."""
import copy

import pytest

import hostcheck_binding as hb
import lightcheck_binding as lb
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json

# csrc/pt_core.h enum Accel (profiles/*_kernel_resource_usage.txt name kernels by these numbers)
(BRUTE, BRUTE_LEAN, BVH, BVH_STACK, BVH_SPHERES, BVH_SPHERES_LDS, GRID, GRID_LDS, BVH_TRI_LDS, GRID_LDS_LEAN,
 BVH_STACK_LEAN, BRUTE_TEX, BVH_STACK_TEX, BRUTE_LIT, BVH_STACK_LIT) = range(15)
LDS_FORMS = {BVH_SPHERES_LDS, GRID_LDS, BVH_TRI_LDS, GRID_LDS_LEAN}
LEAN_FORMS = {BRUTE_LEAN, GRID_LDS_LEAN, BVH_STACK_LEAN}
F64, F32 = capi.RT_PREC_F64, capi.RT_PREC_F32
PRECISIONS = pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
RT_BVH_STACK = 24            # pt_core.h: the traversal stack's entries
RT_TRI_TOP_NODES = 1023      # pt_core.h: the triangle-tree nodes a launch stages at most

_packed = {}


def packed(name, edit=None, lights=False):
    """The scene's descriptor as the renderer packs it (cached: the tests only read it)."""
    key = (name, edit, lights)
    if key not in _packed:
        data = copy.deepcopy(load_scene_json(name))
        if edit == "ortho":
            data["camera"]["type"] = "orthographic"
        elif edit == "solid":
            data["background"] = {"type": "solid", "color": [0.2, 0.3, 0.4], "intensity": 1.0}
        rt = GpuRayTracer(64, 48, seed=1, direct_lighting=lights)
        assert rt.load_from_json(data)
        _packed[key] = rt.packed()
    return _packed[key]


def choice(name, prec, bvh, **kw):
    p = packed(name, kw.pop("edit", None), kw.pop("lights", False))
    c = hb.kernel_choice(p, prec, bvh, **kw)
    assert c["lds"] == (c["acc"] in LDS_FORMS) and (c["lds_bytes"] > 0) == bool(c["lds"])
    assert (c["tri_lds_nodes"] > 0) == (c["acc"] == BVH_TRI_LDS)
    return c


# ---- the committed scenes, default knobs -------------------------------------------------------------------
@PRECISIONS
def test_rtow_takes_the_grid_in_lds_in_its_lean_form(prec):
    """Spheres alone, sky gradient, perspective camera: where choose_walk took the grid (use_grid) the pool launch
    runs the grid with its cells and records in LDS whenever the copy fits (RT_LDS_GRID=1), in the lean form
    (ACC_GRID_LDS_LEAN, spheres alone); else the sphere-only ordered walk, its nodes in LDS
    in binary32 only (RT_LDS_NODES=1).  World order: the lean kernel for spheres and planes (ACC_BRUTE_LEAN)."""
    c = choice("rtow.json", prec, True)
    assert c["num_grid_cells"] > 0 and c["num_tri_nodes"] == 0 and c["num_planes"] == c["num_boxes"] == 0
    if c["use_grid"]:
        assert (c["acc"], c["walk"]) == (GRID_LDS_LEAN, 2)
        # the grid's copy, rounded up to 16 B (RT_MAT_LDS off: no material records behind it)
        assert c["lds_bytes"] == (c["grid_lds_bytes"] + 15) // 16 * 16
    else:
        assert (c["acc"], c["walk"]) == (BVH_SPHERES_LDS if prec == F32 else BVH_SPHERES, 1)
    assert choice("rtow.json", prec, False)["acc"] == BRUTE_LEAN
    # the lane-per-pixel kernel has no lean or LDS form
    assert choice("rtow.json", prec, True, pool=False)["acc"] == (GRID if c["use_grid"] else BVH_SPHERES)
    assert choice("rtow.json", prec, False, pool=False)["acc"] == BRUTE


def test_rtow_binary64_walks_the_grid():
    """DESIGN.md §0 item 4 / smoke(): RTOW in binary64 takes the lean grid LDS kernel (config 3's kernel,
    trace_pool_lds_kernel<double, false, 9>).  The estimate behind use_grid is the host's; the smoke test asserts
    the same of rt_scene_walk on the device."""
    c = choice("rtow.json", F64, True)
    assert c["use_grid"] == 1 and (c["acc"], c["walk"]) == (GRID_LDS_LEAN, 2)


@PRECISIONS
def test_cornell_and_sample_scene(prec):
    """Spheres and planes, no grid built for so few spheres: the sphere-only ordered walk (no triangle code),
    nodes in LDS in binary32 (RT_LDS_NODES=1: binary64 only when asked); World order takes config 2's lean kernel."""
    for name in ("cornell.json", "sample_scene.json"):
        c = choice(name, prec, True)
        assert c["num_tri_nodes"] == 0 and c["num_grid_cells"] == 0 and c["num_boxes"] == 0
        assert (c["acc"], c["walk"]) == (BVH_SPHERES_LDS if prec == F32 else BVH_SPHERES, 1)
        if prec == F32:   # [48 B boxes + 8 B references] x nodes + the workgroup's stacks (the deepest leaf's entries)
            assert c["lds_bytes"] == 56 * c["num_sphere_wide"] + c["sphere_lds_waves"] * min(c["stack_entries"], RT_BVH_STACK) * 256
        b = choice(name, prec, False)
        assert (b["acc"], b["walk"]) == (BRUTE_LEAN, 0)


@PRECISIONS
def test_sample_mesh_takes_the_lean_two_child_kernel(prec):
    """A triangle scene without boxes under the sky gradient: the general ordered walk in its lean form
    (ACC_BVH_STACK_LEAN: spheres, planes, triangles; config 5's kernel).  World order has no lean form with
    triangles (ACC_BRUTE_LEAN is spheres and planes)."""
    c = choice("sample_mesh.json", prec, True)
    assert c["num_tri_nodes"] > 0 and c["num_boxes"] == 0
    assert (c["acc"], c["walk"]) == (BVH_STACK_LEAN, 1)
    assert choice("sample_mesh.json", prec, False)["acc"] == BRUTE
    assert choice("sample_mesh.json", prec, True, pool=False)["acc"] == BVH_STACK


@PRECISIONS
@pytest.mark.parametrize("name", ["kitchen_sink.json", "kitchen_sink_ortho.json"])
def test_kitchen_sink_takes_the_general_kernels(name, prec):
    """Boxes (no lean kernel tests them) and, in the second scene, the orthographic camera: the general ordered
    walk and plain World order."""
    c = choice(name, prec, True)
    assert c["num_boxes"] > 0 and c["num_tri_nodes"] > 0
    assert (c["acc"], c["walk"]) == (BVH_STACK, 1)
    assert (choice(name, prec, False)["acc"], choice(name, prec, False)["walk"]) == (BRUTE, 0)


# ---- textures and lights: the F_TEX / F_LIGHT kernels, whatever the knobs ------------------------------------
KNOB_SETS = [{}, {"lean": 2}, {"lean": 0}, {"lds_grid": 0}, {"lds_nodes": 2}, {"lds_tri": 2, "tri_lds_nodes": 64},
             {"bvh_walk": "grid"}, {"bvh_walk": "tree"}, {"bvh_walk": "skip"}, {"bvh_walk": "two"}]


@PRECISIONS
@pytest.mark.parametrize("name", ["tex_checker_spheres.json", "tex_mesh_wood_crop.json"])
def test_textured_scenes_take_the_tex_kernels(name, prec):
    """DESIGN.md §4 (procedural textures): World order and the general ordered walk, one-wave forms only; never
    the grid, a lean kernel or an LDS kernel.  rt_scene_walk: 0 or 1 (tests/test_textures_gpu.py)."""
    for knobs in KNOB_SETS:
        for pool in (True, False):
            c, b = choice(name, prec, True, pool=pool, **knobs), choice(name, prec, False, pool=pool, **knobs)
            assert c["num_tex"] > 0
            assert (c["acc"], c["walk"], c["lds"]) == (BVH_STACK_TEX, 1, 0)
            assert (b["acc"], b["walk"], b["lds"]) == (BRUTE_TEX, 0, 0)


@PRECISIONS
def test_lit_scenes_take_the_lit_kernels(prec):
    """DESIGN.md §4 (direct lighting): a render with scene lights runs the F_LIGHT kernels, textures included —
    RTOW leaves the grid and the lean kernels (tests/test_lights_gpu.py: rt_scene_walk 2 unlit, 1 / 0 lit)."""
    unlit = choice("rtow.json", prec, True)
    assert unlit["num_lights"] == 0 and unlit["walk"] == (2 if unlit["use_grid"] else 1)
    for case in ("lit_rtow_crop", "lit_tex_mesh_crop", "lit_kitchen_sink"):
        rt, _ = lb.tracer_for(case)
        p = rt.packed()
        for knobs in KNOB_SETS:
            c, b = hb.kernel_choice(p, prec, True, **knobs), hb.kernel_choice(p, prec, False, **knobs)
            assert c["num_lights"] > 0
            assert (c["acc"], c["walk"], c["lds"], c["lds_bytes"]) == (BVH_STACK_LIT, 1, 0, 0)
            assert (b["acc"], b["walk"], b["lds"], b["lds_bytes"]) == (BRUTE_LIT, 0, 0, 0)
        # the lights packed only on request: without them the scene's own kernels
        rt, _ = lb.tracer_for(case, direct_lighting=False)
        assert hb.kernel_choice(rt.packed(), prec, True)["acc"] not in (BVH_STACK_LIT, BRUTE_LIT)


# ---- the knobs ---------------------------------------------------------------------------------------------
def test_rt_lean_and_rt_lds_grid_on_rtow():
    """RT_LEAN=0: the general grid LDS kernel; RT_LDS_GRID=0: the global-memory grid kernel (one-wave, no lean
    form); RT_LEAN=2 keeps the grid's lean form only."""
    assert choice("rtow.json", F64, True)["acc"] == GRID_LDS_LEAN
    assert choice("rtow.json", F64, True, lean=0)["acc"] == GRID_LDS
    assert choice("rtow.json", F64, True, lean=0)["lds_bytes"] == choice("rtow.json", F64, True)["lds_bytes"]
    g = choice("rtow.json", F64, True, lds_grid=0)
    assert (g["acc"], g["lds"], g["walk"]) == (GRID, 0, 2)
    assert choice("rtow.json", F64, True, lean=2)["acc"] == GRID_LDS_LEAN
    assert choice("rtow.json", F64, False, lean=2)["acc"] == BRUTE            # not the World-order lean kernel
    assert choice("sample_mesh.json", F64, True, lean=2)["acc"] == BVH_STACK  # nor the two-child one
    assert choice("cornell.json", F64, False, lean=2)["acc"] == BRUTE
    assert choice("sample_mesh.json", F64, True, lean=0)["acc"] == BVH_STACK
    assert choice("cornell.json", F64, False, lean=0)["acc"] == BRUTE


@PRECISIONS
def test_rt_bvh_walk(prec):
    """RT_BVH_WALK: tree = the sphere tree even where the grid was chosen (binary32: its LDS form; binary64 only
    with RT_LDS_NODES=2, RT_LDS_NODES=0 never); grid = the grid wherever one was built; skip = the stackless
    walk; two = the general ordered walk (lean where the scene allows: RTOW has no boxes)."""
    t = choice("rtow.json", prec, True, bvh_walk="tree")
    assert (t["acc"], t["walk"]) == (BVH_SPHERES_LDS if prec == F32 else BVH_SPHERES, 1)
    t2 = choice("rtow.json", prec, True, bvh_walk="tree", lds_nodes=2)
    assert t2["acc"] == BVH_SPHERES_LDS
    assert t2["lds_bytes"] == 56 * t2["num_sphere_wide"] + t2["sphere_lds_waves"] * min(t2["stack_entries"], RT_BVH_STACK) * 256
    # the budget the choice passed: this workgroup's share of the CU's 160 KiB beside its partials and 256 B
    per_cu = 4 * t2["sphere_lds_occ"] // t2["sphere_lds_waves"]
    assert t2["lds_bytes"] + t2["sphere_lds_waves"] * 3 * 64 * 8 + 256 <= 160 * 1024 // per_cu
    assert choice("rtow.json", prec, True, bvh_walk="tree", lds_nodes=0)["acc"] == BVH_SPHERES
    assert choice("rtow.json", prec, True, bvh_walk="grid")["walk"] == 2
    assert choice("cornell.json", prec, True, bvh_walk="grid")["acc"] in (BVH_SPHERES, BVH_SPHERES_LDS)   # no grid built
    assert choice("rtow.json", prec, True, bvh_walk="skip")["acc"] == BVH
    assert choice("sample_mesh.json", prec, True, bvh_walk="skip")["acc"] == BVH
    assert choice("rtow.json", prec, True, bvh_walk="two")["acc"] == BVH_STACK_LEAN
    assert choice("kitchen_sink.json", prec, True, bvh_walk="two")["acc"] == BVH_STACK
    # with triangles only `skip` changes the walk
    for w in ("tree", "grid", "two"):
        assert choice("sample_mesh.json", prec, True, bvh_walk=w)["acc"] == BVH_STACK_LEAN
    assert choice("rtow.json", prec, False, bvh_walk="grid")["walk"] == 0       # World order is not a BVH walk


@PRECISIONS
def test_lean_needs_the_gradient_the_perspective_camera_and_supersampling(prec):
    """the lean kernels are compiled for the sky gradient, the perspective camera and
    supersampling AA; any other launch falls back to the general kernel of the same walk and form."""
    general = {GRID_LDS_LEAN: GRID_LDS, BVH_STACK_LEAN: BVH_STACK, BRUTE_LEAN: BRUTE}
    for name, bvh in (("rtow.json", True), ("rtow.json", False), ("sample_mesh.json", True), ("cornell.json", False)):
        lean = choice(name, prec, bvh)
        if not (name == "rtow.json" and bvh and not lean["use_grid"]):
            assert lean["acc"] in LEAN_FORMS, name
        for kw in ({"edit": "ortho"}, {"edit": "solid"}, {"aa_mode": capi.RT_AA_STOCHASTIC}):
            c = choice(name, prec, bvh, **kw)
            assert c["acc"] not in LEAN_FORMS
            if c["use_grid"] == lean["use_grid"]:      # (the edited camera may move choose_walk's estimate)
                assert c["acc"] == general.get(lean["acc"], lean["acc"]), (name, kw)
    assert capi.RT_AA_STOCHASTIC != 0 and capi.RT_AA_SUPERSAMPLING == 0


def test_rt_lds_tri():
    """RT_LDS_TRI=1 selects the triangle-LDS kernel in binary64 only (2: both); the staged nodes are the tree's
    breadth-first prefix clamped to RT_TRI_LDS_NODES (<= RT_TRI_TOP_NODES) and to what fits the CU's LDS beside
    the workgroups' stacks and partials, and at least 64: a smaller tree stays on the one-wave kernel."""
    small = choice("sample_mesh.json", F64, True, lds_tri=1)
    assert small["num_tri_wide"] < 64 and small["acc"] == BVH_STACK_LEAN and small["tri_lds_nodes"] == 0
    p = big_mesh()
    off = hb.kernel_choice(p, F64, True)
    assert off["num_tri_wide"] > RT_TRI_TOP_NODES and off["acc"] == BVH_STACK_LEAN      # RT_LDS_TRI=0: never
    for prec, lds_tri, on in ((F64, 1, True), (F32, 1, False), (F32, 2, True), (F64, 2, True)):
        c = hb.kernel_choice(p, prec, True, lds_tri=lds_tri)
        assert (c["acc"] == BVH_TRI_LDS) == on and c["walk"] == 1
        if not on:
            assert c["acc"] == BVH_STACK_LEAN
            continue
        W, entries = c["tri_lds_waves"], min(c["stack_entries"], RT_BVH_STACK)
        budget = 160 * 1024 // (4 * c["tri_lds_occ"] // W)
        fit = (budget - (W * entries * 256 + W * 3 * 64 * 8 + 256)) // 56
        assert c["tri_lds_nodes"] == min(c["num_tri_wide"], RT_TRI_TOP_NODES, fit) >= 64
        assert c["lds_bytes"] == 56 * c["tri_lds_nodes"] + W * entries * 256
        for cap in (64, 100, 5000):
            k = hb.kernel_choice(p, prec, True, lds_tri=lds_tri, tri_lds_nodes=min(cap, RT_TRI_TOP_NODES))
            assert k["tri_lds_nodes"] == min(c["num_tri_wide"], cap, RT_TRI_TOP_NODES, fit)
        assert hb.kernel_choice(p, prec, True, lds_tri=lds_tri, tri_lds_nodes=63)["acc"] == BVH_STACK_LEAN
    # the lane-per-pixel kernel and World order have no such form
    assert hb.kernel_choice(p, F64, True, pool=False, lds_tri=1)["acc"] == BVH_STACK
    assert hb.kernel_choice(p, F64, False, lds_tri=1)["acc"] == BRUTE


_big = []


def big_mesh():
    """sample_mesh.json with its mesh replaced by a 40 x 40 grid of quads: a triangle tree of > 1023 two-child nodes"""
    if not _big:
        data = copy.deepcopy(load_scene_json("sample_mesh.json"))
        mesh = next(o for o in data["objects"] if o["type"] == "mesh")
        n = 40
        mesh["vertices"] = [[x / n - 0.5, 0.1 * ((x + z) % 2), -1.5 - z / n] for z in range(n + 1) for x in range(n + 1)]
        mesh["indices"] = [i for z in range(n) for x in range(n)
                           for i in (z * (n + 1) + x, z * (n + 1) + x + 1, (z + 1) * (n + 1) + x,
                                     z * (n + 1) + x + 1, (z + 1) * (n + 1) + x + 1, (z + 1) * (n + 1) + x)]
        rt = GpuRayTracer(64, 48, seed=1)
        assert rt.load_from_json(data)
        _big.append(rt.packed())
    return _big[0]


def test_rt_bvh_walk_values_parse_as_documented():
    """kernel_select.h parse_bvh_walk: by prefix; anything else (and unset) is the default walk."""
    L = hb.lib()
    L.ptc_parse_bvh_walk.argtypes = [__import__("ctypes").c_char_p]
    default = L.ptc_parse_bvh_walk(None)
    assert default == BVH_SPHERES
    assert [L.ptc_parse_bvh_walk(v) for v in (b"skip", b"two", b"grid", b"")] == [BVH, BVH_STACK, GRID, default]
    assert L.ptc_parse_bvh_walk(b"tree") not in (BVH, BVH_STACK, GRID, default)
    assert L.ptc_parse_bvh_walk(b"other") == default
