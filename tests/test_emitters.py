"""Emitter sampling (next-event estimation with MIS) on the CPU: the emitter lists, the CPU
build of the kernels' sample function against its numpy restatement (tests/nee_ref.py) bit for bit, the sample
density's normalisation, the estimator's expectation against the plain render's (and two deliberate errors that
must be caught), counters, the variance on Cornell, and the hosts' settings.  The GPU side is
tests/test_emitters_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import golden_cases as gc
import nee_ref
import neecheck_binding as nb
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GpuRayTracer

SPHERE, TRI = 0, 1


# ---- 1: emitter lists ------------------------------------------------------------------------------------------
def test_emitter_lists():
    """Cornell lists exactly its light sphere, the default scene its one emissive sphere; nee_mixed lists the quad's
    two triangles, the lamp sphere and the mesh's four triangles in World.objects order — not the box, not the
    sphere whose r^2 is zero, not the planes."""
    rt = nb.tracer("cornell")
    lst = nb.emitters(rt.packed())
    assert len(lst) == 1 and lst[0][0] == SPHERE
    d = rt.packed().desc
    spheres = [i for i in range(d.num_objects) if d.objects[i].type == capi.RT_OBJ_SPHERE]
    light = [k for k, i in enumerate(spheres) if d.materials[d.objects[i].material].type == capi.RT_MAT_EMISSIVE]
    assert [lst[0][1]] == light
    rt = nb.tracer(None)
    lst = nb.emitters(rt.packed())
    assert len(lst) == 1 and lst[0][0] == SPHERE
    rt = nb.tracer("nee_mixed")
    lst, rec = nb.emitters(rt.packed(), records=True)
    # objects: floor, back, quad-a, metal, quad-b, lamp, box, zero-radius lamp, glass, glow-tetra (4), wedge (4)
    assert lst == [(TRI, 0), (TRI, 1), (SPHERE, 1), (TRI, 2), (TRI, 3), (TRI, 4), (TRI, 5)]
    assert np.array_equal(rec[0, 12:15], [6.0, 6.0 * 0.95, 6.0 * 0.85]) and rec[0, 15] == 2.0 and rec[2, 15] == 0.0
    for scene in (None, "cornell", "nee_mixed"):          # the numpy restatement lists the same
        p = nb.tracer(scene).packed()
        assert [(e["kind"], e["idx"]) for e in nee_ref.emitter_list(p.desc)] == nb.emitters(p)


def test_emitter_limit():
    assert nb.lib().ptn_emitter_limit(3) == 0
    assert nb.lib().ptn_emitter_limit((1 << 20) + 1) == -1


# ---- 2: the sample function, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene", nb.SCENES)
def test_samples_equal_numpy_bit_for_bit(scene):
    """emitter_query of the CPU build on 10,000 points x keys: the emitter, omega, p_l and t_e are nee_ref.py's bits
    in both walks, and for the same (o, omega) the hit side's density equals the sample side's within 1e-9."""
    p = nb.tracer(scene).packed()
    pts, keys = nb.query_set(scene)
    ems = nee_ref.emitter_list(p.desc)
    ref = nee_ref.sample(ems, pts[:, :3], pts[:, 3:], keys)
    got = {a: nb.host_samples(p, a, pts, keys) for a in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH)}
    for a, g in got.items():
        assert np.array_equal(g["emitter"], ref["emitter"])
        for k in ("omega", "p_l", "t_e"):
            same = nb.bits(g[k]) == nb.bits(ref[k])
            assert same.all(), (scene, a, k, float(same.mean()))
    g = got[capi.RT_ACCEL_BVH]
    assert np.array_equal(g["visible"], got[capi.RT_ACCEL_BRUTE]["visible"])
    sampled, reached = int((g["p_l"] > 0).sum()), int((g["t_e"] > 0).sum())
    print(f"{scene}: {sampled} of {len(keys)} queries have a sample, {reached} a candidate, {int(g['visible'].sum())} visible")
    assert reached > 1000 and g["visible"].sum() > 500 and (g["visible"] <= (g["t_e"] > 0)).all()
    # the hit side: the same direction's density, recomputed from the hit (t_e along omega)
    hit = g["t_e"] > 0
    N = len(ems)
    rel = np.abs(g["pO_hit"][hit] - g["p_l"][hit] * N) / (g["p_l"][hit] * N)
    print(f"{scene}: hit-side against sample-side density, max relative difference {rel.max():.2e}")
    assert (g["pO_hit"][hit] > 0).all() and rel.max() <= 1e-9
    for e in range(N):                                     # ... and as the specification states it
        m = hit & (g["emitter"] == e)
        if m.any():
            pr = nee_ref.hit_pdf(ems[e], pts[m, :3], g["omega"][m], g["t_e"][m])
            assert np.array_equal(nb.bits(pr), nb.bits(g["pO_hit"][m]))


# ---- 3: normalisation, independent of the code's own density --------------------------------------------------------
def _estimate(p, x, n, count=200000):
    keys = (np.arange(count, dtype=np.uint64) * 2654435761 + 12345).astype(np.uint32)
    pts = np.tile(np.concatenate([x, n]), (count, 1))
    g = nb.host_samples(p, capi.RT_ACCEL_BVH, pts, keys)
    cs = g["omega"] @ np.asarray(n)
    with np.errstate(all="ignore"):
        f = np.where(g["visible"], (cs / np.pi) / g["p_l"], 0.0)
    return g, f


def test_sphere_density_integrates_to_the_projected_solid_angle():
    """Cornell's light sphere from a floor point below it (unoccluded, wholly above the horizon):
    mean(visible (cs / pi) / p_l) = (r^2 / D^2) cos(theta) within 5 standard errors."""
    p = nb.tracer("cornell").packed()
    _, rec = nb.emitters(p, records=True)
    c, r2 = rec[0, 0:3], rec[0, 3]
    # the sphere's centre lies in the ceiling's plane: from this point every tangent ray meets it below the ceiling
    x, n = np.array([0.3, -2.5, -2.8]), np.array([0.0, 1.0, 0.0])
    g, f = _estimate(p, x, n)
    assert g["visible"].all()
    w = c - x
    D2 = w @ w
    want = (r2 / D2) * (w @ n) / np.sqrt(D2)
    se = f.std(ddof=1) / np.sqrt(len(f))
    print(f"sphere: estimate {f.mean():.6f} +- {se:.6f}, (r^2 / D^2) cos = {want:.6f}")
    assert abs(f.mean() - want) <= 5 * se


def test_triangle_density_integrates_to_the_form_factor():
    """One triangle of nee_mixed's quad from a floor point that sees all of it: the mean over the keys that choose
    it against a midpoint quadrature of cos cos' / (pi D^2) over the triangle, within 5 standard errors."""
    p = nb.tracer("nee_mixed").packed()
    _, rec = nb.emitters(p, records=True)
    x, n = np.array([-0.3, -1.0, -3.9]), np.array([0.0, 1.0, 0.0])
    g, f = _estimate(p, x, n)
    mine = g["emitter"] == 0
    assert mine.sum() > 20000 and g["visible"][mine].all()
    f = np.where(mine, f, 0.0)
    v0, e1, e2, nt, area = rec[0, 0:3], rec[0, 3:6], rec[0, 6:9], rec[0, 9:12], rec[0, 15]
    m = 600
    a, b = np.meshgrid((np.arange(m) + 0.5) / m, (np.arange(m) + 0.5) / m, indexing="ij")
    keep = a + b < 1.0                                     # midpoints of the lower-left cells; the diagonal's halves
    half = np.isclose(a + b, 1.0)
    wgt = np.where(keep, 1.0, 0.0) + np.where(half, 0.5, 0.0)
    y = v0 + a[..., None] * e1 + b[..., None] * e2
    v = y - x
    D2 = (v * v).sum(-1)
    om = v / np.sqrt(D2)[..., None]
    integrand = np.maximum(0.0, om @ n) * np.abs(om @ nt) / (np.pi * D2)
    want = (integrand * wgt).sum() * (2.0 * area / (m * m))
    se = f.std(ddof=1) / np.sqrt(len(f))
    print(f"triangle: estimate {f.mean():.6f} +- {se:.6f}, quadrature {want:.6f}")
    assert abs(f.mean() - want) <= 5 * se


# ---- 4: same expectation as the plain render -----------------------------------------------------------------------
SEEDS = 16
SPP = 256
_renders = {}


def _blocks(scene, on, first_seed, mutation=0, direct=False):
    """(SEEDS, 8, 8, 3) block means of 32 x 32 x SPP renders at depth 5 with seeds first_seed .., computed once"""
    key = (scene, on, first_seed, mutation, direct)
    if key not in _renders:
        out = []
        for s in range(SEEDS):
            rt = nb.tracer(scene, seed=first_seed + s, samples=SPP, direct_lighting=direct)
            rt.accel = capi.RT_ACCEL_BVH
            out.append(nb.block_means(nb.host_render(rt.packed(), rt.settings(), on, mutation)["mean"]))
        _renders[key] = np.array(out)
    return _renders[key]


def _report(name, t, blocks):
    mx, share, mt, bound = nb.expectation_conditions(t, blocks)
    print(f"{name}: max |t| {mx:.2f}, |t| > 3 in {100 * share:.2f} %, |mean t| {mt:.3f} (bound {bound:.3f})")


@pytest.mark.parametrize("scene,direct", [("cornell", False), ("nee_mixed", False), ("nee_mixed", True)],
                         ids=["cornell", "nee_mixed", "nee_mixed_lit"])
def test_same_expectation_as_the_plain_render(scene, direct):
    """Welch's t of 4 x 4 block means, 16 seeds x 256 spp a side: no |t| >= 6, at most 2 % above 3, and
    |mean t| <= 4 / sqrt(blocks) — for emitter sampling against plain, as for plain against plain (the control)."""
    plain = _blocks(scene, False, 1, direct=direct)
    t, blocks = nb.welch(_blocks(scene, True, 101, direct=direct), plain)
    _report(f"{scene} sampling against plain", t, blocks)
    tc, _ = nb.welch(_blocks(scene, False, 201, direct=direct), plain)
    _report(f"{scene} plain against plain", tc, blocks)
    assert nb.conditions_hold(tc, blocks)
    assert nb.conditions_hold(t, blocks)


@pytest.mark.parametrize("scene,mutation", [("cornell", 1), ("nee_mixed", 1), ("nee_mixed", 2)])
def test_deliberate_errors_break_the_conditions(scene, mutation):
    """Compiled into the check library only: 1 = the emission weight forced to 1 after a diffuse bounce (light
    counted twice), 2 = the hit side's p_l without 1 / N.  Either must fail the conditions above."""
    t, blocks = nb.welch(_blocks(scene, True, 101, mutation=mutation), _blocks(scene, False, 1))
    _report(f"{scene} mutation {mutation}", t, blocks)
    assert not nb.conditions_hold(t, blocks)


# ---- 5: counters and the no-emitter case -----------------------------------------------------------------------------
@pytest.mark.parametrize("scene", nb.SCENES)
def test_counters_are_the_plain_renders(scene):
    """The emitter draws come from a stream of their own: per-pixel segments and draws equal the plain render's"""
    rt = nb.tracer(scene, samples=16)
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt.accel = accel
        a = nb.host_render(rt.packed(), rt.settings(), False)
        b = nb.host_render(rt.packed(), rt.settings(), True)
        assert np.array_equal(a["segments"], b["segments"]) and np.array_equal(a["draws"], b["draws"])
        assert not np.array_equal(a["mean"], b["mean"])


def test_scene_without_emitters_renders_the_plain_bits():
    rt, c = gc.tracer_for("cfg3_rtow_crop")
    p = rt.packed()
    assert nb.emitters(p) == []
    st = rt.settings(crop=c["crop"])
    a, b = nb.host_render(p, st, False), nb.host_render(p, st, True)
    assert np.array_equal(nb.bits(a["mean"]), nb.bits(b["mean"]))
    assert np.array_equal(nb.bits(a["mean"]), nb.bits(gc.load_array("cfg3_rtow_crop", "linear")))
    for bvh in (False, True):
        for pool in (False, True):
            assert nb.select(p, True, bvh, pool) == nb.select(p, False, bvh, pool)


def test_selection_routes_emitters_first():
    """num_emitters > 0 selects the F_NEE modes (15 World order, 16 the ordered walk), whatever else the scene has;
    rt_scene_walk's report follows the walk"""
    for scene, direct in (("cornell", False), ("nee_mixed", False), ("nee_mixed", True)):
        p = nb.tracer(scene, direct_lighting=direct).packed()
        for pool in (False, True):
            assert nb.select(p, True, False, pool) == (15, 0)
            assert nb.select(p, True, True, pool) == (16, 1)
            assert nb.select(p, False, True, pool)[0] not in (15, 16)


# ---- 6: variance ---------------------------------------------------------------------------------------------------
def test_cornell_variance_is_smaller_with_sampling():
    """Across-seed variance of the 32 x 32 x 256 spp Cornell renders, summed over the frame (block means: the
    renders of test 4): with sampling below without, at equal spp"""
    va = _blocks("cornell", True, 101).var(axis=0, ddof=1).sum()
    vb = _blocks("cornell", False, 1).var(axis=0, ddof=1).sum()
    print(f"cornell: variance with sampling / without = {va / vb:.4f}")
    assert va / vb < 1


# ---- 7: the setter and the hosts' settings -------------------------------------------------------------------------
def test_setter_errors_need_no_device():
    lib = capi.load_library()
    n = C.c_int32(7)
    assert lib.rt_scene_set_emitter_sampling(None, 1) == -1 and b"scene" in lib.rt_last_error()
    assert lib.rt_scene_emitter_count(None, C.byref(n)) == -1
    assert lib.rt_emitter_samples(None, capi.RT_PREC_F64, capi.RT_ACCEL_AUTO, None, None, 0, None, None, None, None, None) == -1


def test_settings_plumbing():
    rt = GpuRayTracer(16, 16)
    assert rt.emitter_sampling is False
    rt._dirty = False
    rt.update_render_settings({"samples": 8})
    assert rt.emitter_sampling is False and rt._dirty is False        # without the key: unchanged, not dirty
    rt.update_render_settings({"emitterSampling": False})
    assert rt._dirty is False
    rt.update_render_settings({"emitterSampling": True})
    assert rt.emitter_sampling is True and rt._dirty is True
    rt._dirty = False
    rt.update_render_settings({"emitterSampling": 1})
    assert rt._dirty is False
    rt.update_render_settings({"emitterSampling": 0})
    assert rt.emitter_sampling is False and rt._dirty is True
    assert GpuRayTracer(16, 16, emitter_sampling=True).emitter_sampling is True
