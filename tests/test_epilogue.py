"""The CPU oracle's epilogue (orc_finalize, orc_tone_map, orc_denoise) against the independent reference
of tests/epilogue_ref.py: numpy binary64 for everything that is exact IEEE arithmetic (bit for bit), mpmath
for the gamma pow (one binary64 ulp, see epilogue_ref).  No GPU: tests/test_epilogue_gpu.py holds the
device to the same reference.

Measured with these input sets (oracle alone; the three tone maps within 0.001 of each other): exempt
share of the near-threshold set 0.063 (gamma 2.2), 0.064 (2.4), 0.035 (1.0), 0.010 (0.25), 0.066 (4.0),
against a cap of 0.08; of the random and special values 0; wrong bytes outside the exemption 0; wrong
binary32 values 0.  Each test prints its shares.
"""
import ctypes as C

import numpy as np
import pytest

import epilogue_ref as er
from oracle import binding


def _oracle_tone_map(st, mean):
    L = binding.lib()
    out = np.zeros_like(mean)
    dp = C.POINTER(C.c_double)
    src, dst = mean.ctypes.data, out.ctypes.data
    for q in range(mean.shape[0]):
        L.orc_tone_map(st.tone_map, st.exposure, C.cast(src + 24 * q, dp), C.cast(dst + 24 * q, dp))
    return out


@pytest.mark.parametrize("tone", er.TONE_MAPS)
@pytest.mark.parametrize("exposure,gamma,samples", er.GRID, ids=er.GRID_IDS)
def test_oracle_finalize_against_numpy_and_mpmath(tone, exposure, gamma, samples):
    sums, n_near = er.input_sums(tone, exposure, gamma, samples)
    st = er.settings(sums.size // 3, tone, exposure, gamma, samples)
    mean, post, rgba = binding.finalize(sums, st)
    ref_mean, ref_tm = er.stage_a(tone, exposure, samples, sums)
    assert er.same_bits(mean.ravel(), ref_mean).all()
    assert er.same_bits(_oracle_tone_map(st, mean).ravel(), ref_tm).all()
    assert (rgba[:, 3] == 255).all()
    byte = rgba[:, :3].ravel()
    with np.errstate(over="ignore"):
        post32 = post.ravel().astype(np.float32)                                # floatData is a Float32Array
    er.check_post_and_bytes(f"oracle {tone} {exposure:g} {gamma:g} {samples}", gamma, ref_tm, n_near, post32, byte)
    assert np.array_equal(byte, er.bytes_of(post).ravel())                    # to_u8 of the oracle's own floats
    if exposure != 0:
        assert len(np.unique(byte[:n_near])) == 256                            # every byte value occurs
    else:
        assert not byte.any()                                                   # tm is 0 or NaN everywhere


def test_special_sums_give_the_bytes_of_the_reference_formulas():
    """What the JS formulas make of sums no render should produce (one sample, exposure 1, gamma 2.2):
    Reinhard -1 -> -inf -> byte 0, below -1 -> a large positive value -> 255; ACES at an overflowing
    x -> inf/inf = NaN -> 0 and at -0.25 -> 1.03 -> 255; Math.max(0, NaN) stays NaN -> 0; -0 -> 0."""
    sums = np.array([-1.0, np.nextafter(-1.0, -2.0), -2.0, 1e300, np.nan, np.inf, -np.inf, -0.0, 5e-324,
                     0.25, -0.25, 1.0])
    want = {"reinhard": [0, 255, 255, 255, 0, 0, 0, 0, 0, 122, 0, 186],
            "aces": [255, 255, 255, 0, 0, 0, 0, 0, 0, 163, 255, 230],
            "linear": [0, 0, 0, 255, 0, 255, 0, 0, 0, 135, 0, 255]}
    for tone, w in want.items():
        _, post, rgba = binding.finalize(sums, er.settings(4, tone, 1.0, 2.2, 1))
        assert rgba[:, :3].ravel().tolist() == w, tone
        assert np.isnan(post.ravel()[4])


def _frames32(w, h):
    for name, f in er.denoise_frames(w, h).items():
        fl = np.ones((h, w, 4), dtype=np.float32)
        fl[..., :3] = np.maximum(0.0, f)                       # what a linear, gamma-1 epilogue stores
        fl[..., 3] = np.linspace(0.0, 1.0, w * h, dtype=np.float32).reshape(h, w)     # alpha is copied, not filtered
        yield name, fl


@pytest.mark.parametrize("w,h", er.DENOISE_SHAPES)
def test_oracle_denoise_against_numpy_and_exact_mean(w, h):
    L = binding.lib()
    fp = C.POINTER(C.c_float)
    for strength in er.DENOISE_STRENGTHS:
        wts = np.array(er.denoise_weights(strength))
        assert np.allclose(wts, [np.exp(-1 / (2 * strength ** 2)), np.exp(-2 / (2 * strength ** 2))], rtol=1e-13, atol=0)
        for name, fl in _frames32(w, h):
            out = np.zeros_like(fl)
            L.orc_denoise(fl.ctypes.data_as(fp), w, h, wts.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(fp))
            ref = er.denoise_ref(fl, wts)
            assert er.same_bits(out.ravel(), ref.ravel()).all(), (strength, name)
            assert np.array_equal(out[..., 3], fl[..., 3])
            if name == "nan_inf_negative":
                assert np.array_equal(np.isnan(out[..., :3]).all(axis=2), er.nan_neighbourhood(fl)), strength
                assert np.array_equal(np.isnan(out[..., :3]).any(axis=2), er.nan_neighbourhood(fl)), strength
                continue
            exact = er.denoise_exact(fl, wts)
            for o, e in zip(out[..., :3].ravel(), exact.ravel()):
                near = np.float32(float(e))
                assert np.nextafter(near, np.float32(-np.inf)) <= o <= np.nextafter(near, np.float32(np.inf)), \
                    (strength, name, o, float(e))
