"""The variance-guided form of the guided filter without a GPU: the CPU build of the product's per-pixel body
(tests/hostcheck/vguided_check.cpp) against the independent restatement of tests/vguided_ref.py, bit for bit and
for both outputs, the filter's statistical properties, parameter validation and the Python host's settings."""
import ctypes as C

import numpy as np
import pytest

import guided_ref as gr
import guidedcheck_binding as gb
import vguided_ref as vr
import vguidedcheck_binding as vb
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GUIDED_SIGMA_VARIANCE, GpuRayTracer

INF = float("inf")
_levels_cache = {}


def ref_levels(w, h, sv, sigmas=gr.SIGMAS):
    """vguided_ref's eight levels of frame (w, h), computed once and shared."""
    key = (w, h, sv, sigmas)
    if key not in _levels_cache:
        color, guides = gr.frame(w, h)
        _levels_cache[key] = vr.filter_levels(color, vr.variance_frame(w, h), guides, 8, sigmas, sv)
    return _levels_cache[key]


def mismatches(a, b):
    return int(np.count_nonzero(gr.bits(a) != gr.bits(b)))


# ---- the filter against the reference ---------------------------------------------------------------------
@pytest.mark.parametrize("sv", [0.5, 4.0], ids=["sv0.5", "sv4"])
@pytest.mark.parametrize("w,h", gr.FRAME_SIZES, ids=[f"{w}x{h}" for w, h in gr.FRAME_SIZES])
def test_cpu_filter_equals_reference_at_every_level_count(w, h, sv):
    """guided_ref.frame's colours and guides with a variance frame of positive noise, a block of exact zeros, a
    negative value, a NaN-variance and a +inf-variance pixel; levels 1..8 (the steps reach far past the frames)."""
    color, guides = gr.frame(w, h)
    var = vr.variance_frame(w, h)
    ref = ref_levels(w, h, sv)
    for levels in range(1, 9):
        c, v = vb.host_filter(color, var, guides, levels, gr.SIGMAS, sv)
        rc, rv = ref[levels - 1]
        assert gr.same(c, rc), ("colour", levels, mismatches(c, rc))
        assert gr.same(v, rv), ("variance", levels, mismatches(v, rv))


def test_variance_frame_has_its_features():
    v = vr.variance_frame(40, 24)
    color, _ = gr.frame(40, 24)
    assert (v == 0).sum() >= 3 * 12 and (v < 0).sum() == 1
    nan_v, inf_v = np.isnan(v).any(axis=2), np.isinf(v).any(axis=2)
    assert nan_v.sum() == 1 and inf_v.sum() == 1
    assert np.isfinite(color[nan_v | inf_v]).all()          # the colour there is finite: the variance alone excludes


@pytest.mark.parametrize("w,h", [(17, 9), (40, 24)], ids=["17x9", "40x24"])
def test_non_finite_pixels_pass_through_and_never_spread(w, h):
    color, guides = gr.frame(w, h)
    var = vr.variance_frame(w, h)
    bad = ~(np.isfinite(color).all(axis=2) & np.isfinite(var).all(axis=2))
    assert bad.sum() == 4                                   # NaN and +inf colour, NaN and +inf variance
    for levels in (1, 2, 5):
        c, v = vb.host_filter(color, var, guides, levels, gr.SIGMAS, 4.0)
        assert gr.same(c[bad], color[bad]) and gr.same(v[bad], var[bad])
        assert np.isfinite(c[~bad]).all() and np.isfinite(v[~bad]).all() and (v[~bad] >= 0).all()


def test_a_negative_variance_reads_as_zero():
    color, guides = gr.frame(17, 9)
    var = vr.variance_frame(17, 9)
    neg = var < 0
    assert neg.sum() == 1
    zeroed = np.where(neg, 0.0, var)
    a, b = vb.host_filter(color, var, guides, 3, gr.SIGMAS, 4.0), vb.host_filter(color, zeroed, guides, 3, gr.SIGMAS, 4.0)
    assert gr.same(a[0], b[0]) and gr.same(a[1], b[1])


def test_constant_image_comes_back_at_any_variance():
    """dc = 0 exactly, so the colour term is 0 whatever the variance (zero included: 0 * 2^40 = 0).  25 products,
    their sum and the division: about 51 roundings of 2^-53 -> 1e-14 relative."""
    _, guides = gr.frame(40, 24)
    rng = np.random.default_rng(3)
    for var in (np.zeros((24, 40, 3)), np.full((24, 40, 3), 1e-4), 10.0 ** rng.uniform(-12, 2, (24, 40, 3))):
        for value in (0.37, 1e-3, 123.456):
            color = np.full((24, 40, 3), value)
            for levels in (1, 5, 8):
                c, v = vb.host_filter(color, var, guides, levels, gr.SIGMAS, 4.0)
                assert np.max(np.abs(c - value)) <= 1e-14 * value, (value, levels)
                assert np.isfinite(v).all() and (v >= 0).all()


# ---- infinite sigmas ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4), ids=["variance", "albedo", "normal", "depth"])
@pytest.mark.parametrize("w,h", [(5, 3), (17, 9)], ids=["5x3", "17x9"])
def test_each_sigma_infinite_in_turn(w, h, which):
    sigmas = tuple(INF if k == which and k > 0 else s for k, s in enumerate(gr.SIGMAS))
    sv = INF if which == 0 else 4.0
    color, guides = gr.frame(w, h)
    var = vr.variance_frame(w, h)
    ref = vr.filter_levels(color, var, guides, 3, sigmas, sv)
    for levels in (1, 3):
        c, v = vb.host_filter(color, var, guides, levels, sigmas, sv)
        assert gr.same(c, ref[levels - 1][0]) and gr.same(v, ref[levels - 1][1]), levels


def test_every_sigma_infinite_is_the_plain_wavelet_kernel():
    """All terms off: the weights are the B3 taps alone, exactly what the plain filter computes with every sigma
    infinite (finite variances: the same pixels take part), and the variance reference agrees."""
    color, guides = gr.frame(17, 9)
    var = np.full((9, 17, 3), 1e-3)
    sig = (INF,) * 4
    c, v = vb.host_filter(color, var, guides, 2, sig, INF)
    assert gr.same(c, gr.guided_filter(color, guides, 2, sig))
    assert gr.same(c, gb.host_filter(color, guides, 2, sig))
    assert gr.same(v, vr.vguided_filter(color, var, guides, 2, sig, INF)[1])


def test_infinite_sigma_variance_with_zero_variance_has_no_nan():
    """isv = 0 and vb = 0: ec = (dc * 0) * 2^40 = 0, never inf * 0."""
    color, guides = gr.frame(17, 9)
    fin = np.isfinite(color).all(axis=2)
    var = np.zeros((9, 17, 3))
    for sig in (gr.SIGMAS, (INF,) * 4):
        c, v = vb.host_filter(color, var, guides, 3, sig, INF)
        assert np.isfinite(c[fin]).all() and not v.any()
        rc, rv = vr.vguided_filter(color, var, guides, 3, sig, INF)
        assert gr.same(c, rc) and gr.same(v, rv)


# ---- what the propagated variance means ------------------------------------------------------------------------
def test_propagated_variance_is_the_variance_of_the_output():
    """sigma_variance = +inf over flat guides: the weights do not depend on the colours, so c' is a fixed linear
    map of independent inputs and v' = sum w^2 v / (sum w)^2 is its variance exactly.  4000 draws of the 48 x 32
    frame with known per-pixel variance, one level: one pixel's empirical variance has relative standard error
    sqrt(2 / 3999) = 2.2 %; the sum over 4608 values is far tighter, 0.02 is more than four of its standard errors
    even with the 25-tap correlation between neighbours."""
    clean, sigma, guides = vr.stripes_frame()
    h, w = sigma.shape
    var = (sigma * sigma)[..., None] * np.ones(3)
    sig = (1.0, 0.1, 0.35, 0.05)
    rng = np.random.default_rng(42)
    draws = 4000
    s1 = np.zeros((h, w, 3))
    s2 = np.zeros((h, w, 3))
    vout = None
    for _ in range(draws):
        c, v = vb.host_filter(clean + sigma[..., None] * rng.standard_normal((h, w, 3)), var, guides, 1, sig, INF)
        d = c - clean                                   # the map keeps constants: E c' is the filtered clean frame
        s1 += d
        s2 += d * d
        assert vout is None or gr.same(v, vout)         # deterministic weights: the same v' every draw
        vout = v
    emp = (s2 - s1 * s1 / draws) / (draws - 1)
    ratio = float(emp.sum() / vout.sum())
    pix = emp / vout
    print(f"variance propagation: sum ratio {ratio:.4f}, per-value ratios {pix.min():.3f} .. {pix.max():.3f}")
    assert abs(ratio - 1.0) <= 0.02, ratio


def batch_means(samples, groups):
    """(mean, var_mean) of samples (N, h, w, 3) in `groups` equal groups, as the error estimate forms them:
    B = sum S_c^2 / n_c - S^2 / N, var_mean = max(0, B) / ((K - 1) N)."""
    n = samples.shape[0]
    nc = n // groups
    assert nc * groups == n
    s = samples.sum(axis=0)
    q = sum((samples[k * nc:(k + 1) * nc].sum(axis=0) ** 2) / nc for k in range(groups))
    b = q - s * s / n
    return s / n, np.where(b > 0, b, 0.0) / ((groups - 1) * n)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("groups", [2, 4, 16], ids=["K2", "K4", "K16"])
def test_heteroscedastic_frame(groups, seed):
    """What the feature is for.  Left half: sigma 0.01 noise over 3-pixel stripes the guides do not see; right half:
    sigma 0.25 noise over a flat colour.  One frame-wide colour stop either blurs the stripes or keeps the noise;
    the per-pixel stop does neither.  16 samples in K groups, 5 levels, sigmas (., 0.1, 0.35, 0.05): the variance form
    at sigma_variance 4 has an RMS error against the clean frame below half the best plain guided filter's over
    sigma_color in {0.05, 0.25, 1.0}."""
    clean, sigma, guides = vr.stripes_frame()
    h, w = sigma.shape
    rng = np.random.default_rng(100 + seed)
    samples = clean + sigma[..., None] * rng.standard_normal((16, h, w, 3))
    mean, var = batch_means(samples, groups)
    rms = lambda a: float(np.sqrt(np.mean((a - clean) ** 2)))                        # noqa: E731
    plain = {sc: rms(gb.host_filter(mean, guides, 5, (sc, 0.1, 0.35, 0.05))) for sc in (0.05, 0.25, 1.0)}
    got = rms(vb.host_filter(mean, var, guides, 5, (1.0, 0.1, 0.35, 0.05), 4.0)[0])
    print(f"K={groups} seed={seed}: unfiltered {rms(mean):.4f}, plain {plain}, variance form {got:.4f}, "
          f"ratio {got / min(plain.values()):.3f}")
    assert got < 0.5 * min(plain.values()), (got, plain)


# ---- validation and hosts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sv", [-1.0, -0.0 - 1e-300, -INF, float("nan")])
def test_invalid_sigma_variance_is_refused_without_a_device(lib, sv):
    assert vb.lib().ptv_sigma_ok(sv) == 0
    assert lib.rt_scene_set_guided_variance(None, sv) == -1 and b"sigma_variance" in lib.rt_last_error()
    p = gb.params(5, gr.SIGMAS)
    assert lib.rt_guided_filter_variance_device(None, 4, 4, C.byref(p), sv, None, None, None, None, None, None) == -1
    assert b"sigma_variance" in lib.rt_last_error()


def test_zero_is_off_for_the_scene_and_invalid_for_the_filter(lib):
    assert vb.lib().ptv_sigma_ok(0.0) == 0
    assert lib.rt_scene_set_guided_variance(None, 0.0) == -1 and b"scene is NULL" in lib.rt_last_error()
    p = gb.params(5, gr.SIGMAS)
    assert lib.rt_guided_filter_variance_device(None, 4, 4, C.byref(p), 0.0, None, None, None, None, None, None) == -1
    assert b"sigma_variance" in lib.rt_last_error()


def test_valid_parameters_pass_validation(lib):
    for sv in (1e-300, 4.0, 1e300, INF):
        assert vb.lib().ptv_sigma_ok(sv) == 1
        assert lib.rt_scene_set_guided_variance(None, sv) == -1 and b"scene is NULL" in lib.rt_last_error()
        p = gb.params(5, gr.SIGMAS)
        assert lib.rt_guided_filter_variance_device(None, 4, 4, C.byref(p), sv, None, None, None, None, None, None) == -1
        assert b"NULL argument" in lib.rt_last_error()
    bad = gb.params(9, gr.SIGMAS)                        # the guided parameters are checked first, as before
    assert lib.rt_guided_filter_variance_device(None, 4, 4, C.byref(bad), 4.0, None, None, None, None, None, None) == -1
    assert b"guided parameters" in lib.rt_last_error()
    assert lib.rt_guided_filtered_variance(None, None) == -1


def test_abi_version_is_still_3(lib):
    assert lib.rt_abi_version() == 3 == capi.RT_ABI_VERSION


def test_default_sigma_variance_is_the_headers(tmp_path):
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_hip.h")
    src = tmp_path / "d.c"
    src.write_text(f'#include <stdio.h>\n#include "{header}"\n'
                   'int main(void){printf("%.17g\\n", (double)RT_GUIDED_DEFAULT_SIGMA_VARIANCE);return 0;}')
    exe = tmp_path / "d"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    assert float(subprocess.check_output([str(exe)]).decode()) == GUIDED_SIGMA_VARIANCE == capi.RT_GUIDED_DEFAULT_SIGMA_VARIANCE


def test_settings_without_the_new_keys_leave_the_filter_alone():
    rt = GpuRayTracer(8, 8, error_estimate=True)
    assert rt.guided_variance is False and rt.guided_sigma_variance == GUIDED_SIGMA_VARIANCE
    rt.update_render_settings({"guidedDenoise": True, "guidedVariance": True, "guidedSigmaVariance": 2.5})
    assert rt.guided_variance is True and rt.guided_sigma_variance == 2.5 and rt.guided_params() is not None
    rt.update_render_settings({"samples": 8})                  # the reference's keys only
    assert rt.samples == 8 and rt.guided_variance is True and rt.guided_sigma_variance == 2.5
    rt.update_render_settings({"guidedVariance": False})
    assert rt.guided_variance is False and rt.guided_sigma_variance == 2.5 and rt.guided_params() is not None
