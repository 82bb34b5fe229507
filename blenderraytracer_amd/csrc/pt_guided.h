// pt_guided.h — the guided filter's per-pixel body: one level of the edge-avoiding à-trous wavelet filter
// (Dammertz et al. 2010) over the linear mean, guided by the feature buffers of aov_pixel
// (pt_path.h).  Host and device (RT_HD): tests/hostcheck compiles it for the CPU.  DESIGN.md §4 "Guided
// filter" is the definition; this is its arithmetic, operation for operation, always in binary64 and
// unfused (-ffp-contract=off), whatever the render's precision.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rt_hip.h"
#include "js_math.h"
#include "pt_path.h"

namespace rt {

// One level: step 2^l, ic = 1 / (sigma_color 2^-l)^2, ia = 1 / sigma_albedo^2, in = 1 / sigma_normal^2,
// sz = sigma_depth.  An infinite sigma gives the factor 0 (sz: the quotient 0): its term drops out.
struct GuidedLevel { int w, h, step, pad; double ic, ia, in, sz; };

inline GuidedLevel guided_level(int w, int h, const rt_guided_params& p, int level) {
    const double sc = p.sigma_color * (1.0 / (double)(1 << level));          // sigma_color 2^-l, exact scaling
    return GuidedLevel{w, h, 1 << level, 0, 1.0 / (sc * sc), 1.0 / (p.sigma_albedo * p.sigma_albedo),
                       1.0 / (p.sigma_normal * p.sigma_normal), p.sigma_depth};
}

// levels in 1..RT_GUIDED_MAX_LEVELS, every sigma > 0 (+inf allowed) and not NaN
inline bool guided_params_ok(const rt_guided_params* p) {
    if (!p || p->levels < 1 || p->levels > RT_GUIDED_MAX_LEVELS) return false;
    for (double s : {p->sigma_color, p->sigma_albedo, p->sigma_normal, p->sigma_depth})
        if (!(s > 0.0)) return false;
    return true;
}

RT_HD bool guided_finite3(const double* c) {
    return fabs(c[0]) < (double)INFINITY && fabs(c[1]) < (double)INFINITY && fabs(c[2]) < (double)INFINITY;   // NaN: false
}
// the compressive colour coordinate: the colour distance does not depend on exposure
RT_HD double guided_compress(double x) {
    const double m = x > 0.0 ? x : 0.0;
    return m / (1.0 + m);
}

// the B3-spline taps (1/16, 1/4, 3/8, 1/4, 1/16) at offset -2..2
RT_HD double guided_tap(int d) { return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625; }

// out[0..2] of pixel (x, y) (top-down row-major, like c: 3 doubles per pixel, and g: 8 floats per pixel).
// A pixel with a non-finite channel passes through; taps outside the image, taps with a non-finite channel
// and taps across an infinite-versus-finite depth are skipped.  The centre tap weighs 9/64, so ws > 0.
RT_HD void guided_pixel(const GuidedLevel& L, const double* __restrict__ c, const float* g, int x, int y,
                        double* out) {
    // g is 16-byte aligned (rt_guided_filter_device checks it): a guide record is two 16-byte loads
    g = static_cast<const float*>(__builtin_assume_aligned(g, 16));
    const size_t p = (size_t)y * L.w + x;
    const double cp[3] = {c[3 * p], c[3 * p + 1], c[3 * p + 2]};
    if (!guided_finite3(cp)) {
        out[0] = cp[0]; out[1] = cp[1]; out[2] = cp[2];
        return;
    }
    const double tp[3] = {guided_compress(cp[0]), guided_compress(cp[1]), guided_compress(cp[2])};
    double gp[7];
    for (int k = 0; k < 7; ++k) gp[k] = (double)g[8 * p + k];
    double acc[3] = {0.0, 0.0, 0.0}, ws = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * L.step;
        if (qy < 0 || qy >= L.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * L.step;
            if (qx < 0 || qx >= L.w) continue;
            const size_t q = (size_t)qy * L.w + qx;
            const double cq[3] = {c[3 * q], c[3 * q + 1], c[3 * q + 2]};
            if (!guided_finite3(cq)) continue;
            const float* gq = g + 8 * q;
            const double zp = gp[6], zq = (double)gq[6];
            double ez = 0.0;
            if (!(zp == zq)) {
                if (fabs(zp) == (double)INFINITY || fabs(zq) == (double)INFINITY) continue;
                const double r = (zp - zq) / (L.sz * (zp + zq));
                ez = r * r;
            }
            const double t0 = tp[0] - guided_compress(cq[0]), t1 = tp[1] - guided_compress(cq[1]),
                         t2 = tp[2] - guided_compress(cq[2]);
            const double dc = (t0 * t0 + t1 * t1) + t2 * t2;
            const double a0 = gp[0] - (double)gq[0], a1 = gp[1] - (double)gq[1], a2 = gp[2] - (double)gq[2];
            const double da = (a0 * a0 + a1 * a1) + a2 * a2;
            const double n0 = gp[3] - (double)gq[3], n1 = gp[4] - (double)gq[4], n2 = gp[5] - (double)gq[5];
            const double dn = (n0 * n0 + n1 * n1) + n2 * n2;
            const double e = ((dc * L.ic + da * L.ia) + dn * L.in) + ez;
            const double wt = (guided_tap(dy) * guided_tap(dx)) * jsm::exp(-e);
            acc[0] += wt * cq[0];
            acc[1] += wt * cq[1];
            acc[2] += wt * cq[2];
            ws += wt;
        }
    }
    out[0] = acc[0] / ws; out[1] = acc[1] / ws; out[2] = acc[2] / ws;
}

// ---- launch interface (pt_guided.hip) ----
// The frame whose pixels get feature buffers: the crop window (top-down rows) of a width x height image
struct AovFrame { int width, height, x0, y0, cw, ch; };
// aov_pixel of every crop pixel -> guides (8 floats per pixel, 16-byte aligned) and, where not nullptr, kind and
// idx as rt_closest_hits reports them.  The walk is launch_closest_hits' choice (kernel_select.h).
template <class R>
hipError_t launch_aovs(const SceneView<R>& sc, bool bvh, const AovFrame& f, float* guides, int* kind, int* idx,
                       hipStream_t stream);
// one level of the filter: out = guided_pixel of every pixel of `in` (never in place)
hipError_t launch_guided_level(const GuidedLevel& L, const double* in, const float* guides, double* out, hipStream_t stream);
// mean[k] = sum[k] / samples (finalize_kernel's division) for n values
hipError_t launch_mean(const double* sum, int samples, double* mean, size_t n, hipStream_t stream);

}  // namespace rt
