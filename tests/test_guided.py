"""The guided filter and the feature buffers without a GPU: the CPU build of the product's per-pixel code
(tests/hostcheck/guided_check.cpp) against the independent restatement of tests/guided_ref.py, bit for bit,
plus the new ABI structs, parameter validation and the Python host's settings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guided_ref as gr
import guidedcheck_binding as gb
import texcheck_binding as tb
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GUIDED_LEVELS, GUIDED_SIGMAS, GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json

INF = float("inf")
AOV_SCENES = ("sample_scene", "cornell", "kitchen_sink", "kitchen_sink_ortho", "sample_mesh", "tex_checker_spheres",
              "tex_mesh_wood_crop")
_levels_cache = {}


def ref_levels(w, h, sigmas=gr.SIGMAS):
    """guided_ref's eight levels of frame (w, h), computed once and shared."""
    key = (w, h, sigmas)
    if key not in _levels_cache:
        color, guides = gr.frame(w, h)
        _levels_cache[key] = gr.filter_levels(color, guides, 8, sigmas)
    return _levels_cache[key]


# ---- the filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", gr.FRAME_SIZES, ids=[f"{w}x{h}" for w, h in gr.FRAME_SIZES])
def test_cpu_filter_equals_reference_at_every_level_count(w, h):
    """Frames with NaN, +inf and negative pixels, a row of misses, a guide edge on a colour edge and one off it;
    levels 1..8 (from level 3 on the step exceeds the small frames: only the centre tap survives)."""
    color, guides = gr.frame(w, h)
    ref = ref_levels(w, h)
    for levels in range(1, 9):
        got = gb.host_filter(color, guides, levels, gr.SIGMAS)
        assert gr.same(got, ref[levels - 1]), (levels, int(np.count_nonzero(gr.bits(got) != gr.bits(ref[levels - 1]))))


@pytest.mark.parametrize("which", range(4), ids=["color", "albedo", "normal", "depth"])
@pytest.mark.parametrize("w,h", [(5, 3), (17, 9)], ids=["5x3", "17x9"])
def test_each_sigma_infinite_in_turn(w, h, which):
    sigmas = tuple(INF if k == which else s for k, s in enumerate(gr.SIGMAS))
    color, guides = gr.frame(w, h)
    ref = gr.filter_levels(color, guides, 3, sigmas)
    for levels in (1, 3):
        assert gr.same(gb.host_filter(color, guides, levels, sigmas), ref[levels - 1]), levels
    if which == 3:      # an infinite-versus-finite depth pair still skips the tap: hits never mix with the misses
        hit_only = color.copy()
        hit_only[h - 1] = 1e6
        other = gb.host_filter(hit_only, guides, 3, sigmas)
        assert gr.same(other[: h - 1], gb.host_filter(color, guides, 3, sigmas)[: h - 1])


def test_every_sigma_infinite_is_the_plain_wavelet_kernel():
    """All terms off: weights are the B3 taps alone, so a hit-only frame is smoothed across every guide edge."""
    color, guides = gr.frame(17, 9)
    sig = (INF,) * 4
    assert gr.same(gb.host_filter(color, guides, 2, sig), gr.guided_filter(color, guides, 2, sig))


def test_constant_image_comes_back():
    """25 products, their sum and the division: about 51 roundings of 2^-53 -> 1e-14 relative."""
    _, guides = gr.frame(40, 24)
    for value in (0.37, 1e-3, 123.456):
        color = np.full((24, 40, 3), value)
        for levels in (1, 5, 8):
            out = gb.host_filter(color, guides, levels, gr.SIGMAS)
            assert np.max(np.abs(out - value)) <= 1e-14 * value, (value, levels)


def test_nan_passes_through_and_never_spreads():
    color, guides = gr.frame(17, 9)
    nan_in = np.isnan(color).any(axis=2)
    inf_in = np.isinf(color).any(axis=2)
    assert nan_in.sum() == 1 and inf_in.sum() == 1
    for levels in (1, 2, 5):
        out = gb.host_filter(color, guides, levels, gr.SIGMAS)
        assert gr.same(out[nan_in], color[nan_in]) and gr.same(out[inf_in], color[inf_in])
        assert np.isfinite(out[~(nan_in | inf_in)]).all()


def test_guide_edge_is_kept_and_flat_regions_are_smoothed():
    """The albedo edge in the middle column keeps its step (no weight crosses it at sigma_albedo 0.1 for an
    albedo distance of 0.98: exp(-98) < 1e-42), while the noise inside each half shrinks."""
    rng = np.random.default_rng(5)
    h, w = 24, 40
    left = np.mgrid[0:h, 0:w][1] < w // 2
    color = np.where(left[..., None], 0.8, 0.2) + rng.uniform(-0.05, 0.05, (h, w, 3))
    g = np.zeros((h, w, 8), dtype=np.float32)
    g[..., 0:3] = np.where(left[..., None], (0.9, 0.2, 0.2), (0.2, 0.2, 0.9))
    g[..., 4] = 1.0
    g[..., 6] = 3.0
    out = gb.host_filter(color, g, 5, (1.0, 0.1, 0.35, 0.05))
    assert out[left].min() > 0.7 and out[~left].max() < 0.3
    assert out[left].std() < 0.25 * color[left].std() and out[~left].std() < 0.25 * color[~left].std()


# ---- the feature buffers --------------------------------------------------------------------------------
def tracer(scene, precision=capi.RT_PREC_F64, accel=capi.RT_ACCEL_AUTO):
    rt = GpuRayTracer(64, 48, seed=3, precision=precision, accel=accel)
    assert rt.load_from_json(load_scene_json(scene + ".json"))
    return rt


def cpu_reference_aovs(rt, accel=capi.RT_ACCEL_BVH, crop=None):
    """guided_ref.aovs with the closest hits and texture values of the CPU build (the albedo buffer's texture
    function: test_albedo_texture_function pins it to texture_value)."""
    packed = rt.packed()
    hits = lambda rays: gb.host_closest_hits(packed, rt.precision, accel, rays)                     # noqa: E731
    tex = lambda t, pts: gb.host_texture_values(packed.desc, t, pts, precision=rt.precision)          # noqa: E731
    return gr.aovs(packed.desc, rt.width, rt.height, rt.precision, hits, tex, crop=crop)


@pytest.mark.parametrize("precision", [capi.RT_PREC_F64, capi.RT_PREC_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("scene", AOV_SCENES)
def test_cpu_aovs_equal_reference(scene, precision):
    rt = tracer(scene, precision)
    ref_g, ref_kind, ref_idx = cpu_reference_aovs(rt)
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        st = rt.settings()
        st.accel = accel
        g, kind, idx = gb.host_aovs(rt.packed(), st)
        assert np.array_equal(kind, ref_kind) and np.array_equal(idx, ref_idx), accel
        assert gr.same(g, ref_g), (accel, int(np.count_nonzero(gr.bits(g) != gr.bits(ref_g))))
    assert (g[..., 7] == 0).all()
    miss = ref_kind < 0
    assert np.isinf(g[miss][:, 6]).all() and not g[miss][:, :6].any()
    assert (ref_kind >= 0).any()


@pytest.mark.parametrize("scene", ["tex_checker_spheres", "tex_kitchen_sink", "tex_mesh_wood_crop"])
def test_albedo_texture_function(scene):
    """aov_texture_value against texture_value (tests/test_textures.py pins that one to the reference's fixtures).
    Binary64: the same function, bit for bit.  Binary32: the same operations with the sine of V8's binary64
    Math.sin rounded to binary32 instead of the platform's sinf; each sine is within one binary32 ulp of the
    true one (<= 2^-24 for |sin| <= 1), so the two differ by at most 2^-23 there, and the colour is
    lerp-like in 0.5 (1 + sin) with channel slopes <= 0.4 plus four roundings of values below 1: 2^-22 covers
    it.  The checker only reads the sign of a product of sines, so away from the zeros it is the same colour."""
    rt = tracer(scene)
    desc = rt.packed().desc
    assert desc.num_textures > 0
    pts = np.random.default_rng(11).uniform(-3, 3, (400, 3))
    for t in range(desc.num_textures):
        a = gb.host_texture_values(desc, t, pts)
        assert gr.same(a, tb.host_texture_values(desc, t, pts)), t
        a32 = gb.host_texture_values(desc, t, pts, precision=capi.RT_PREC_F32)
        b32 = tb.host_texture_values(desc, t, pts, precision=capi.RT_PREC_F32)
        if desc.textures[t].type == capi.RT_TEX_CHECKER:
            assert np.mean(np.all(a32 == b32, axis=1)) > 0.99, t
        else:
            assert np.max(np.abs(a32 - b32)) <= 2.0 ** -22, (t, float(np.max(np.abs(a32 - b32))))
        assert gr.same(a32.astype(np.float32).astype(np.float64), a32)          # values of binary32


def test_cpu_aovs_of_a_crop_are_the_frames_window():
    rt = tracer("kitchen_sink")
    full, kind, _ = gb.host_aovs(rt.packed(), rt.settings())
    crop = (9, 5, 21, 13)
    part, pkind, _ = gb.host_aovs(rt.packed(), rt.settings(crop=crop))
    assert gr.same(part, full[5:18, 9:30]) and np.array_equal(pkind, kind[5:18, 9:30])
    assert gr.same(cpu_reference_aovs(rt, crop=crop)[0], part)


# ---- ABI, validation, settings ----------------------------------------------------------------------------
def test_new_structs_are_laid_out_as_gcc_lays_them_out(tmp_path):
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_hip.h")
    structs = {"rt_guided_params": capi.GuidedParams, "rt_aov_output": capi.AovOutput}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append('printf("levels %d\\n", RT_GUIDED_MAX_LEVELS);')
    lines.append('printf("defaults %d,%.17g,%.17g,%.17g,%.17g\\n", RT_GUIDED_DEFAULT_LEVELS, RT_GUIDED_DEFAULT_SIGMA_COLOR, '
                 'RT_GUIDED_DEFAULT_SIGMA_ALBEDO, RT_GUIDED_DEFAULT_SIGMA_NORMAL, RT_GUIDED_DEFAULT_SIGMA_DEPTH);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().split("\n") if l)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f in py._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(py, f[0]).offset, (cname, f[0])
    assert int(got["levels"]) == capi.RT_GUIDED_MAX_LEVELS == 8
    assert C.sizeof(capi.GuidedParams) == 40 and C.sizeof(capi.AovOutput) == 40
    d = [float(x) for x in got["defaults"].split(",")]             # the hosts share the header's defaults
    assert d == [GUIDED_LEVELS] + [GUIDED_SIGMAS[k] for k in ("color", "albedo", "normal", "depth")]


BAD_PARAMS = [(0, gr.SIGMAS), (9, gr.SIGMAS), (-1, gr.SIGMAS), (5, (0.0, 0.1, 0.35, 0.05)), (5, (0.5, -0.1, 0.35, 0.05)),
              (5, (0.5, 0.1, float("nan"), 0.05)), (5, (0.5, 0.1, 0.35, 0.0)), (5, (0.5, 0.1, 0.35, -INF))]


@pytest.mark.parametrize("levels,sigmas", BAD_PARAMS)
def test_invalid_parameters_are_refused_without_a_device(lib, levels, sigmas):
    """The parameters are checked before the scene and before any device: RT_ERR_INVALID naming the parameter,
    with the same verdict from the shared validation compiled for the CPU."""
    p = gb.params(levels, sigmas)
    assert gb.lib().ptg_params_ok(C.byref(p)) == 0
    assert lib.rt_scene_set_guided(None, C.byref(p)) == -1
    assert b"guided" in lib.rt_last_error()
    assert lib.rt_guided_filter_device(None, 4, 4, C.byref(p), None, None, None, None) == -1
    assert b"guided" in lib.rt_last_error()


def test_valid_parameters_pass_validation(lib):
    for levels, sigmas in [(1, gr.SIGMAS), (8, gr.SIGMAS), (5, (INF,) * 4), (5, (1e-300, 1e300, 0.35, 0.05))]:
        p = gb.params(levels, sigmas)
        assert gb.lib().ptg_params_ok(C.byref(p)) == 1
        assert lib.rt_scene_set_guided(None, C.byref(p)) == -1 and b"scene is NULL" in lib.rt_last_error()


def test_abi_version_is_still_3(lib):
    assert lib.rt_abi_version() == 3 == capi.RT_ABI_VERSION


def test_settings_without_the_guided_keys_leave_the_filter_alone():
    rt = GpuRayTracer(8, 8)
    assert rt.guided_params() is None and rt.guided_levels == GUIDED_LEVELS == 5
    rt.update_render_settings({"guidedDenoise": True, "guidedLevels": 3, "guidedSigmaColor": 0.25, "guidedSigmaDepth": 0.1})
    p = rt.guided_params()
    assert (p.levels, p.sigma_color, p.sigma_albedo, p.sigma_normal, p.sigma_depth) == (
        3, 0.25, GUIDED_SIGMAS["albedo"], GUIDED_SIGMAS["normal"], 0.1)
    rt.update_render_settings({"samples": 8})                  # the reference's keys only
    p = rt.guided_params()
    assert rt.samples == 8 and (p.levels, p.sigma_color, p.sigma_depth) == (3, 0.25, 0.1)
    rt.update_render_settings({"guidedDenoise": False})
    assert rt.guided_params() is None and rt.guided_levels == 3
