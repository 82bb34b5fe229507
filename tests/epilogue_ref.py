"""An independent reference of the epilogue (mean, tone map, gamma, RGBA8, denoise) for
tests/test_epilogue.py (the CPU oracle against it) and tests/test_epilogue_gpu.py (the device against it).

Stage A is plain numpy binary64 in the operation order of post-processor.js: exact IEEE arithmetic, so the
code under test must give its bits.  Stage B, p = tm^(1/gamma), is mpmath at 128 bits: neither the oracle's
nor the device's pow is a port of it.  V8's pow is not correctly rounded (measured error below 1 ulp), so
stage B allows one binary64 ulp before the binary32 rounding, and exempts a byte only where 255 p lies within
3 binary64 ulps of an integer k (pow error < 1 ulp + the product's rounding 0.5 ulp < 2 ulps): there the byte
may be k - 1 or k.  The share of exempt values is capped by the callers.
"""
import ctypes as C
from fractions import Fraction

import mpmath
import numpy as np

from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import settings_struct

TONE_MAPS = ("reinhard", "aces", "linear")
# (exposure, gamma, samples)
GRID = ((1.0, 2.2, 1), (1.7, 2.4, 3), (0.6, 1.0, 7), (1.0, 0.25, 512), (1.0, 4.0, 1024), (1e200, 2.2, 1), (0.0, 2.2, 1))
GRID_IDS = tuple(f"e{e:g}-g{g:g}-s{s}" for e, g, s in GRID)
NEAR_CAP = 0.08           # exempt share allowed on the near-threshold set
OTHER_CAP = 1e-4          # ... on the random and special values
EPS = 2.0 ** -52

SPARSE_STEPS = np.union1d(np.arange(-3000, 3001, 25), np.arange(-8, 9)).astype(np.int64)
DENSE_STEPS = np.arange(-3000, 3001, dtype=np.int64)


def settings(n_or_wh, tone_map, exposure, gamma, samples, denoise_strength=None):
    """rt_settings of a frame of n x 1 (or w x h) pixels with this epilogue."""
    w, h = (n_or_wh, 1) if isinstance(n_or_wh, int) else n_or_wh
    return settings_struct(w, h, samples, 5, "supersampling", tone_map, exposure, gamma, 1,
                           denoising=denoise_strength is not None, denoise_strength=denoise_strength or 0.5)


# ---- stage A: numpy binary64 ---------------------------------------------------------------------
def tone_map(name, x):
    """toneMap of x = mean * exposure (post-processor.js:9-30); np.maximum propagates NaN like Math.max,
    and the + 0.0 makes its -0 the +0 of Math.max(0, -0)."""
    with np.errstate(all="ignore"):
        if name == "aces":
            return np.maximum(0.0, (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)) + 0.0
        if name == "linear":
            return x
        return x / (1.0 + x)


def stage_a(name, exposure, samples, sums):
    """(mean, tm) of the sample sums."""
    with np.errstate(all="ignore"):
        mean = sums / float(samples)
        return mean, tone_map(name, mean * exposure)


def inverse_tone_map(name, tm):
    """An x whose tone-mapped value is tm up to a few ulps (where one exists)."""
    with np.errstate(all="ignore"):
        if name == "linear":
            return tm
        if name == "reinhard":
            return tm / (1.0 - tm)
        qa, qb, qc = 2.51 - 2.43 * tm, 0.03 - 0.59 * tm, 0.14 * tm        # qa x^2 + qb x - qc = 0
        root = np.sqrt(qb * qb + 4.0 * qa * qc)
        return np.where(qb >= 0, 2.0 * qc / (qb + root), (root - qb) / (2.0 * qa))   # no cancellation


def same_bits(a, b):
    """Equal bit patterns (the sign of zero included); any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def input_sums(name, exposure, gamma, samples, steps=SPARSE_STEPS):
    """The sample sums of one parameter set -> (sums padded to whole pixels, count of near-threshold values).
    Near-threshold: (k/255)^gamma for k = 1..255 offset by `steps` ulps, each value mapped through the
    inverse tone map, exposure and sample count into sum space.  Then 5000 tone-mapped values uniform in
    [-0.5, 1.5] and 2000 log-uniform in 1e-30 .. 1e30, mapped back the same way (as x itself where the
    tone map has no such value: the saturated end of ACES), and the special sums.  With exposure 0 nothing
    maps back: the values are scaled by the sample count alone."""
    k = np.arange(1, 256, dtype=np.float64)
    approx = (k / 255.0) ** gamma
    near = (approx.view(np.int64)[:, None] + steps[None, :]).ravel().view(np.float64)
    rng = np.random.default_rng(20)
    rand = np.concatenate([rng.uniform(-0.5, 1.5, 5000), 10.0 ** rng.uniform(-30, 30, 2000)])
    with np.errstate(all="ignore"):
        scale = float(samples) / exposure if exposure != 0 else float(samples)
        inv_e = np.float64(1.0) / np.float64(exposure)
        special = np.array([0.0, -0.0, -1.0, 1.0, np.nextafter(-1.0, -2.0) * inv_e, np.inf, -np.inf, np.nan, 5e-324,
                            1e300, 1e-300, -1.0 * scale, np.nextafter(-1.0, -2.0) * scale, -2.0 * scale, 1e300 * scale])
        targets = np.concatenate([near, rand])
        x = inverse_tone_map(name, targets)
        sums = np.concatenate([np.where(np.isnan(x), targets, x) * scale, special])
    pad = -sums.size % 3
    return np.concatenate([sums, np.zeros(pad)]), near.size


# ---- stage B: mpmath -----------------------------------------------------------------------------
_mp = mpmath.mp.clone()
_mp.prec = 128
_cache = {}           # (1/gamma, bits of tm) -> the binary64 nearest p: independent of the tone map


def _pow(inv_gamma, t):
    return _mp.power(_mp.mpf(t), _mp.mpf(inv_gamma))


def _round_f32(r):
    """The binary32 nearest the real r (an mpf), ties to even, without a double rounding."""
    d = float(r)                                   # correctly rounded binary64
    f = np.float32(d)
    if not np.isfinite(f) or float(f) == d:
        return float(f)
    other = np.nextafter(f, np.float32(np.inf if d > float(f) else -np.inf))
    if np.isfinite(other) and abs(d - float(f)) == abs(float(other) - d):     # d is the tie: r decides
        if (r > d) == (float(other) > d) and r != d:
            return float(other)
    return float(f)


def _nearest_pow(inv_gamma, bits):
    """The binary64 nearest t^inv_gamma for the finite positive binary64 t of these bit patterns."""
    if len(_cache) > 400_000:
        _cache.clear()
    out = np.empty(bits.size)
    for i, (b, t) in enumerate(zip(bits.tolist(), bits.view(np.float64).tolist())):
        d = _cache.get((inv_gamma, b))
        if d is None:
            d = _cache[(inv_gamma, b)] = float(_pow(inv_gamma, t))
        out[i] = d
    return out


def stage_b(gamma, tm):
    """For every tone-mapped value: (lo32, hi32, byte, exempt, k).  float32(p (1 -+ 2^-52)), the byte
    min(255, floor(255 p)), and whether 255 p is within 3 ulps of the integer k in 1..255.  mpmath gives
    the binary64 nearest p for every value; binary64 arithmetic on it decides wherever it provably can
    (its error bounds are in the comments), and the exact criteria are evaluated in mpmath elsewhere."""
    inv_gamma = 1.0 / gamma                         # the rounded double, as the code under test uses
    bits, inverse = np.unique(np.ascontiguousarray(tm, dtype=np.float64).ravel().view(np.uint64), return_inverse=True)
    with np.errstate(all="ignore"):
        t = np.maximum(0.0, bits.view(np.float64))                             # Math.max(0, tm)
        d = t.copy()                                # NaN, 0, inf and 1 are their own powers (1/gamma > 0)
        plain = np.isfinite(t) & (t > 0) & (t != 1.0)
        d[plain] = _nearest_pow(inv_gamma, t[plain].view(np.uint64))
        # binary32: p (1 -+ 2^-52) lie within 4 binary64 ulps of d, and rounding is monotone
        dn = up = d
        for _ in range(4):
            dn, up = np.nextafter(dn, -np.inf), np.nextafter(up, np.inf)
        lo, hi = dn.astype(np.float32), up.astype(np.float32)
        for i in np.flatnonzero(plain & (lo != hi)):                           # next to a binary32 tie: exactly
            p = _pow(inv_gamma, float(t[i]))
            lo[i], hi[i] = _round_f32(p * (1 - _mp.mpf(EPS))), _round_f32(p * (1 + _mp.mpf(EPS)))
        # bytes: |255 d - 255 p| <= 2^-52 * 255 p (the rounding of d and of the product), so where 255 d is
        # further than 5 * 2^-52 k from the nearest integer k, floor(255 d) = floor(255 p) and p is not exempt
        vd = 255.0 * d
        k = np.rint(vd)
        want = np.where(np.isnan(vd), 0, np.minimum(255.0, np.floor(vd))).astype(np.int64)
        exempt = np.zeros(d.size, dtype=bool)
        kk = np.where((k >= 1) & (k <= 255), k, 0).astype(np.int64)
        for i in np.flatnonzero(plain & (kk > 0) & (np.abs(vd - k) <= 5 * EPS * k)):
            v = 255 * _pow(inv_gamma, float(t[i]))
            want[i] = min(255, int(_mp.floor(v)))
            exempt[i] = abs(v - int(kk[i])) <= 3 * EPS * int(kk[i])
    return lo[inverse], hi[inverse], want[inverse], exempt[inverse], kk[inverse]


def check_post_and_bytes(label, gamma, tm, n_near, post32, byte):
    """The stage-B criteria on the flat per-channel arrays of one epilogue (tm from stage A, post as
    binary32, the RGB bytes); the first n_near values are the near-threshold set.  Prints the exempt
    shares and asserts the caps."""
    lo, hi, want, exempt, k = stage_b(gamma, tm)
    post32 = np.asarray(post32, dtype=np.float32)
    byte = np.asarray(byte).astype(np.int64)
    nan = np.isnan(lo)
    bad_post = np.where(nan, ~np.isnan(post32), (post32 != lo) & (post32 != hi))
    assert not bad_post.any(), (label, "post", int(bad_post.sum()),
                                [(tm[i], post32[i], lo[i], hi[i]) for i in np.flatnonzero(bad_post)[:5]])
    bad_byte = (byte != want) & ~(exempt & ((byte == k - 1) | (byte == k)))
    assert not bad_byte.any(), (label, "byte", int(bad_byte.sum()),
                                [(tm[i], byte[i], want[i], exempt[i]) for i in np.flatnonzero(bad_byte)[:5]])
    near_share = float(exempt[:n_near].mean())
    other_share = float(exempt[n_near:].mean())
    used = int(np.count_nonzero(exempt & (byte != want)))
    print(f"{label}: exempt share near-threshold {near_share:.4f}, other {other_share:.2e}; "
          f"exempt bytes that differ from floor(255 p): {used}")
    assert near_share <= NEAR_CAP, (label, near_share)
    assert other_share <= OTHER_CAP, (label, other_share)


# ---- denoise ---------------------------------------------------------------------------------------
DENOISE_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (16, 17), (19, 27), (257, 3))     # (w, h)
DENOISE_STRENGTHS = (0.5, 1.3, 0.05, 10.0)


def denoise_weights(strength):
    """(w1, w2) as the renderer computes them."""
    return tuple(settings((1, 1), "linear", 1.0, 1.0, 1, denoise_strength=strength).denoise_weights)


def denoise_ref(fl, wts):
    """PostProcessor.denoise of an (h, w, 4) binary32 frame: binary64 accumulation, ky outer and kx inner,
    clamp to edge, divided by the accumulated weight, rounded to binary32; alpha copied."""
    h, w = fl.shape[:2]
    acc = np.zeros((h, w, 3))
    weight = np.zeros((h, w, 1))
    with np.errstate(all="ignore"):
        for ky in (-1, 0, 1):
            for kx in (-1, 0, 1):
                ny = np.clip(np.arange(h) + ky, 0, h - 1)
                nx = np.clip(np.arange(w) + kx, 0, w - 1)
                d2 = kx * kx + ky * ky
                wt = 1.0 if d2 == 0 else wts[d2 - 1]
                acc = acc + fl[ny][:, nx, :3].astype(np.float64) * wt
                weight = weight + wt
        out = fl.copy()
        out[..., :3] = (acc / weight).astype(np.float32)
    return out


def denoise_exact(fl, wts):
    """The weighted mean as exact rationals -> an (h, w, 3) array of Fractions (finite frames only)."""
    h, w = fl.shape[:2]
    fw = (Fraction(1), Fraction(float(wts[0])), Fraction(float(wts[1])))
    out = np.empty((h, w, 3), dtype=object)
    for y in range(h):
        for x in range(w):
            for c in range(3):
                num = den = Fraction(0)
                for ky in (-1, 0, 1):
                    for kx in (-1, 0, 1):
                        wt = fw[kx * kx + ky * ky]
                        num += Fraction(float(fl[min(h - 1, max(0, y + ky)), min(w - 1, max(0, x + kx)), c])) * wt
                        den += wt
                out[y, x, c] = num / den
    return out


def denoise_frames(w, h):
    """Post-gamma test frames (h, w, 3) as binary64 sums for a linear, gamma-1 epilogue: random values in
    [0, 1.2], a checkerboard of 0 and 1, and random values with one NaN, one +Inf and one negative pixel."""
    rng = np.random.default_rng(w * 1000 + h)
    rand = rng.uniform(0.0, 1.2, (h, w, 3))
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.repeat(((xx + yy) % 2).astype(np.float64)[..., None], 3, axis=2)
    bad = rng.uniform(0.0, 1.2, (h, w, 3)).reshape(-1, 3)
    n = w * h
    if n > 1:
        bad[0] = np.inf
    if n > 2:
        bad[n - 1] = -0.75
    bad[n // 2] = np.nan
    return {"random": rand, "checker": checker, "nan_inf_negative": bad.reshape(h, w, 3)}


def nan_neighbourhood(frame):
    """The pixels whose 3x3 clamp-to-edge neighbourhood holds a NaN (frame: (h, w, C))."""
    m = np.isnan(frame).any(axis=2)
    h, w = m.shape
    out = np.zeros_like(m)
    for ky in (-1, 0, 1):
        for kx in (-1, 0, 1):
            out |= m[np.clip(np.arange(h) + ky, 0, h - 1)][:, np.clip(np.arange(w) + kx, 0, w - 1)]
    return out


def bytes_of(post):
    """RGBA8 of post-gamma floats: min(255, max(0, floor(255 c))), NaN -> 0 (ray-tracer.js:245-247)."""
    with np.errstate(all="ignore"):
        v = np.floor(post.astype(np.float64) * 255.0)
        return np.where(np.isnan(v), 0, np.clip(v, 0, 255)).astype(np.uint8)


# ---- device calls (tests/test_epilogue_gpu.py) ------------------------------------------------------
def finalize_device(scene, st, sums, mean=False, post=False, stream=None):
    """rt_finalize_device on synthetic sums -> dict of host arrays.  Without mean and post the call is
    RGBA8-only (the threshold kernel for gammas that have a table), else finalize_kernel."""
    import torch
    lib = capi.load_library()
    n = (st.crop_w or st.width) * (st.crop_h or st.height)
    d_sum = torch.from_numpy(np.ascontiguousarray(sums, dtype=np.float64).ravel()).cuda()
    assert d_sum.numel() == 3 * n
    d_rgba = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    d_mean = torch.zeros(3 * n, dtype=torch.float64, device="cuda") if mean else None
    d_post = torch.zeros(4 * n, dtype=torch.float32, device="cuda") if post else None
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    capi.check(lib.rt_finalize_device(scene, C.byref(st), ptr(d_sum), ptr(d_mean), ptr(d_post), ptr(d_rgba), stream))
    torch.cuda.synchronize()
    res = {"rgba8": d_rgba.cpu().numpy().reshape(n, 4)}
    if mean:
        res["mean"] = d_mean.cpu().numpy().reshape(n, 3)
    if post:
        res["post"] = d_post.cpu().numpy().reshape(n, 4)
    return res
