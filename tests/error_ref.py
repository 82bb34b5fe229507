"""The error estimate's rational-arithmetic reference (fractions) and its error bounds.  TEST INFRASTRUCTURE ONLY.

Definition (DESIGN.md §4 "Error estimate"): a pixel channel's K group sums S_c over n_c samples (N = sum n_c), the
sum S the estimator reads (the render's binary64 sum, taken as given):

    Q = sum_c S_c^2 / n_c        var_mean = max(0, Q - S^2 / N) / ((K - 1) N)
    e_p = sqrt(sum_ch var_mean) / (sum_ch S / N + 0.03)        frame_error = mean of e_p over the finite pixels

The bound on var_mean, u = 2^-53, first order, every rounding counted once (csrc/pt_error.h computes in this order):

  * a group sum S_c that is itself a floating-point sum of n_c non-negative samples (the GPU tests rebuild the
    groups from exact per-sample radiances; the CPU tests give the group sums exactly): relative (n_c - 1) u, so
    2 (n_c - 1) u on S_c^2
  * S_c * S_c and the division by n_c: 2 u on each term of Q
  * the K additions into q, all terms non-negative, the first onto zero (exact): (K - 1) u Q
        => |q - Q| <= (K + 1 + 2 (n_max - 1)) u Q
  * S * S and the division by N: 2 u S^2 / N
  * the subtraction: u |q - S^2/N| <= u (Q + S^2/N);  max(0, .) moves no value away from the clamped reference
  * (K - 1) * N (exact for these sizes, counted once) and the final division: 2 u var <= 2 u (Q + S^2/N) / ((K - 1) N)

Q's coefficient is K + 2 n_max + 2, S^2/N's is 5 (smaller: K >= 2, n_max >= 1); one more for the second-order terms:

    |var - var_ref| <= c u (Q + S^2/N) / ((K - 1) N),    c = K + 2 n_max + 3
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def var_c(groups, n_max):
    """c of the bound above"""
    return groups + 2 * n_max + 3


def reference(group_sums, sizes, sums, per_sample=False):
    """group_sums (K, h, w, 3) float64 — or, per_sample, the N samples' values (N, h, w, 3), whose groups' exact sums
    are taken — sizes (K ints), sums (h, w, 3) float64 -> (var (h, w, 3) float64 rounded from the exact value, NaN
    where the pixel is not finite; scale (h, w, 3) = (Q + S^2/N) / ((K - 1) N); the exact var and the exact mean sums
    per pixel as Fractions (dicts keyed by (y, x)); bad (h, w) bool)."""
    g = np.asarray(group_sums, dtype=np.float64)
    s = np.asarray(sums, dtype=np.float64)
    K = len(sizes)
    N = int(sum(sizes))
    _, h, w, _ = g.shape
    assert g.shape[0] == (N if per_sample else K) and K >= 2
    edges = np.cumsum([0] + [int(n) for n in sizes])

    def group(c, y, x, k):
        if not per_sample:
            return Fraction(float(g[c, y, x, k]))
        return sum((Fraction(float(v)) for v in g[edges[c]:edges[c + 1], y, x, k]), Fraction(0))
    bad = ~(np.isfinite(g).all(axis=(0, 3)) & np.isfinite(s).all(axis=2))
    var = np.full((h, w, 3), np.nan)
    scale = np.full((h, w, 3), np.nan)
    vp, mp = {}, {}
    den = (K - 1) * N
    for y in range(h):
        for x in range(w):
            if bad[y, x]:
                continue
            v_sum, m_sum = Fraction(0), Fraction(0)
            for k in range(3):
                Q = sum((group(c, y, x, k) ** 2 / int(sizes[c]) for c in range(K)), Fraction(0))
                S = Fraction(float(s[y, x, k]))
                t = S * S / N
                v = max(Fraction(0), Q - t) / den
                var[y, x, k] = float(v)
                scale[y, x, k] = float((Q + t) / den)
                v_sum += v
                m_sum += S / N
            vp[(y, x)], mp[(y, x)] = v_sum, m_sum
    return var, scale, vp, mp, bad


def var_tolerance(scale, groups, n_max):
    return var_c(groups, n_max) * U * scale


# e_p: the device's sqrt, three S / N, two additions of them, the + 0.03, the division and two additions of v: 9
# roundings; the reference's own binary64 evaluation below: float(v_p), sqrt, float(m_p), + 0.03, the division: 5
E_ROUNDINGS = 16


def rel_reference(vp, mp, tol_var, bad):
    """(e (h, w) float64, tol (h, w)) from reference()'s exact v_p and m_p and the per-channel var tolerances:
    |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)) carries var's bound through the root."""
    h, w = bad.shape
    e = np.full((h, w), np.nan)
    tol = np.full((h, w), np.nan)
    for (y, x), v in vp.items():
        m = float(mp[(y, x)]) + 0.03
        fv = float(v)
        e[y, x] = math.sqrt(fv) / m
        dv = float(np.sum(tol_var[y, x]))
        droot = math.sqrt(dv) if fv <= 0.0 else min(math.sqrt(dv), dv / math.sqrt(fv))
        tol[y, x] = droot / m + E_ROUNDINGS * U * e[y, x]
    return e, tol


def frame_reference(e, tol, bad):
    """(frame_error, its tolerance, max_error's pixel set) over the finite pixels: every e_p goes through at most
    6 (tile tree) + ceil(tiles / 64) (a lane's tiles) + 6 (frame tree) additions of non-negative values and one
    division."""
    h, w = bad.shape
    good = ~bad
    n = int(good.sum())
    if n == 0:
        return float("nan"), 0.0
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    adds = 6 + (tiles + 63) // 64 + 6 + 1
    fe = math.fsum(e[good]) / n
    return fe, float(np.sum(tol[good])) / n + adds * U * fe
