// pt_vguided.h — the variance-guided form of the guided filter's per-pixel body: one level of the à-trous
// filter whose colour stop is normalised by the pixel's estimated variance (the error estimate's var_mean,
// pt_error.h), with the variance carried through the levels as SVGF has it (Schied et al. 2017).
// Host and device (RT_HD): tests/hostcheck compiles it for the CPU.  DESIGN.md §4 "Variance-guided filter" is
// the definition; this is its arithmetic, operation for operation, always in binary64 and unfused
// (-ffp-contract=off), whatever the render's precision.  guided_pixel (pt_guided.h) is untouched.
#pragma once
#include "pt_guided.h"

namespace rt {

// One level: step 2^l, isv = 1 / sigma_variance^2, ia = 1 / sigma_albedo^2, in = 1 / sigma_normal^2,
// sz = sigma_depth.  No sigma is scaled per level: the propagated variance shrinks and tightens the stop by
// itself.  An infinite sigma gives the factor 0 (sz: the quotient 0): its term drops out.
struct VGuidedLevel { int w, h, step, pad; double isv, ia, in, sz; };

inline VGuidedLevel vguided_level(int w, int h, const rt_guided_params& p, double sigma_variance, int level) {
    return VGuidedLevel{w, h, 1 << level, 0, 1.0 / (sigma_variance * sigma_variance),
                        1.0 / (p.sigma_albedo * p.sigma_albedo), 1.0 / (p.sigma_normal * p.sigma_normal), p.sigma_depth};
}

// sigma_variance > 0 (+inf allowed) and not NaN
inline bool vguided_sigma_ok(double sigma_variance) { return sigma_variance > 0.0; }

// a variance as the filter reads it: negative values (and -0) read as 0
RT_HD double vguided_pos(double v) { return v > 0.0 ? v : 0.0; }
// a pixel takes part when its three colour and its three variance channels are finite
RT_HD bool vguided_finite(const double* c, const double* v) { return guided_finite3(c) && guided_finite3(v); }

// the 3 x 3 variance prefilter's taps (1/4, 1/2, 1/4) at offset -1..1
RT_HD double vguided_tap3(int d) { return d == 0 ? 0.5 : 0.25; }

// 2^-40: keeps 1 / vb finite where the prefiltered variance is zero
#define RT_VGUIDED_EPS 0x1p-40

// cout[0..2] and vout[0..2] of pixel (x, y) (top-down row-major; c and v: 3 doubles per pixel, g: 8 floats per
// pixel).  A pixel with a non-finite colour or variance channel passes through in both; taps outside the
// image, non-finite taps and taps across an infinite-versus-finite depth are skipped.  The centre tap has
// e = 0 and weighs 9/64, so ws > 0; the prefilter's centre weighs 1/4, so den > 0.
RT_HD void vguided_pixel(const VGuidedLevel& L, const double* __restrict__ c, const double* __restrict__ v,
                         const float* g, int x, int y, double* cout, double* vout) {
    g = static_cast<const float*>(__builtin_assume_aligned(g, 16));
    const size_t p = (size_t)y * L.w + x;
    const double cp[3] = {c[3 * p], c[3 * p + 1], c[3 * p + 2]};
    const double vp[3] = {v[3 * p], v[3 * p + 1], v[3 * p + 2]};
    if (!vguided_finite(cp, vp)) {
        cout[0] = cp[0]; cout[1] = cp[1]; cout[2] = cp[2];
        vout[0] = vp[0]; vout[1] = vp[1]; vout[2] = vp[2];
        return;
    }
    // the variance prefilter: the 3 x 3 binomial mean of the channels' summed variance, at step 1 on every level
    double num = 0.0, den = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= L.h) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= L.w) continue;
            const size_t q = (size_t)qy * L.w + qx;
            const double cq[3] = {c[3 * q], c[3 * q + 1], c[3 * q + 2]};
            const double vq[3] = {v[3 * q], v[3 * q + 1], v[3 * q + 2]};
            if (!vguided_finite(cq, vq)) continue;
            const double k = vguided_tap3(dy) * vguided_tap3(dx);
            const double vs = (vguided_pos(vq[0]) + vguided_pos(vq[1])) + vguided_pos(vq[2]);
            num += k * vs;
            den += k;
        }
    }
    const double vb = num / den;
    const double ivb = 1.0 / (vb + RT_VGUIDED_EPS);
    double gp[7];
    for (int k = 0; k < 7; ++k) gp[k] = (double)g[8 * p + k];
    double acc[3] = {0.0, 0.0, 0.0}, vacc[3] = {0.0, 0.0, 0.0}, ws = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * L.step;
        if (qy < 0 || qy >= L.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * L.step;
            if (qx < 0 || qx >= L.w) continue;
            const size_t q = (size_t)qy * L.w + qx;
            const double cq[3] = {c[3 * q], c[3 * q + 1], c[3 * q + 2]};
            const double vq[3] = {v[3 * q], v[3 * q + 1], v[3 * q + 2]};
            if (!vguided_finite(cq, vq)) continue;
            const float* gq = g + 8 * q;
            const double zp = gp[6], zq = (double)gq[6];
            double ez = 0.0;
            if (!(zp == zq)) {
                if (fabs(zp) == (double)INFINITY || fabs(zq) == (double)INFINITY) continue;
                const double r = (zp - zq) / (L.sz * (zp + zq));
                ez = r * r;
            }
            const double t0 = cp[0] - cq[0], t1 = cp[1] - cq[1], t2 = cp[2] - cq[2];
            const double dc = (t0 * t0 + t1 * t1) + t2 * t2;
            const double ec = (dc * L.isv) * ivb;
            const double a0 = gp[0] - (double)gq[0], a1 = gp[1] - (double)gq[1], a2 = gp[2] - (double)gq[2];
            const double da = (a0 * a0 + a1 * a1) + a2 * a2;
            const double n0 = gp[3] - (double)gq[3], n1 = gp[4] - (double)gq[4], n2 = gp[5] - (double)gq[5];
            const double dn = (n0 * n0 + n1 * n1) + n2 * n2;
            const double e = ((ec + da * L.ia) + dn * L.in) + ez;
            const double wt = (guided_tap(dy) * guided_tap(dx)) * jsm::exp(-e);
            const double w2 = wt * wt;
            acc[0] += wt * cq[0];
            acc[1] += wt * cq[1];
            acc[2] += wt * cq[2];
            vacc[0] += w2 * vguided_pos(vq[0]);
            vacc[1] += w2 * vguided_pos(vq[1]);
            vacc[2] += w2 * vguided_pos(vq[2]);
            ws += wt;
        }
    }
    const double ws2 = ws * ws;
    cout[0] = acc[0] / ws; cout[1] = acc[1] / ws; cout[2] = acc[2] / ws;
    vout[0] = vacc[0] / ws2; vout[1] = vacc[1] / ws2; vout[2] = vacc[2] / ws2;
}

// ---- launch interface (pt_guided.hip) ----
// one level: (cout, vout) = vguided_pixel of every pixel of (cin, vin), never in place; vout may be nullptr
// (the last level of a caller that does not want the propagated variance)
hipError_t launch_vguided_level(const VGuidedLevel& L, const double* cin, const double* vin, const float* guides,
                                double* cout, double* vout, hipStream_t stream);

}  // namespace rt
