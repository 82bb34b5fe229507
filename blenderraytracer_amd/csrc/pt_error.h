// pt_error.h — the per-pixel error estimate from the sample pool's chunk partials (batch means; DESIGN.md §4
// "Error estimate").  A pixel's chunk partials S_c (one per chunk of n_c samples, Σn_c = N, K chunks, S = ΣS_c)
// are independent group sums, so B = Σ S_c²/n_c − S²/N has expectation (K − 1) σ² whatever the group sizes;
// B / (K − 1) estimates the per-sample variance and B / ((K − 1) N) the variance of the pixel's mean.
// Host and device (RT_HD): tests/hostcheck compiles the bodies for the CPU.  Always binary64 and unfused
// (-ffp-contract=off), whatever the render's precision: the partials and the sums are binary64 in both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_path.h"

namespace rt {

// samples of chunk c of a batch of `batch_samples` samples in chunks of `chunk` (the last may be short)
RT_HD int error_group_samples(int chunk, int batch_samples, int c) { return min(chunk, batch_samples - c * chunk); }

// one chunk's term of the second moment: q += S_c² / n_c
RT_HD double error_moment_add(double q, double s, int n) { return q + (s * s) / (double)n; }

RT_HD bool error_finite(double x) { return fabs(x) < (double)INFINITY; }   // NaN: false

// var_mean of one channel: max(0, q − S²/N) / ((K − 1) N), K >= 2
RT_HD double error_var_channel(double s, double q, int groups, int samples) {
    const double nn = (double)samples;
    const double b = q - (s * s) / nn;
    return (b > 0.0 ? b : 0.0) / ((double)(groups - 1) * nn);
}

// One pixel from its three sums s and moments q: v[0..2] = var_mean per channel (v may be nullptr) and the
// relative error e_p = sqrt(v_p) / (m_p + 0.03), v_p = (v0 + v1) + v2 the channels' var_mean and m_p = (s0/N +
// s1/N) + s2/N their means (the 0.03 keeps black pixels finite).  A non-finite sum or moment: NaN everywhere.
// The channels go one after the other (not unrolled): one binary64 division's registers at a time, so the
// kernel fits beside the trace waves.
RT_HD double error_pixel(const double* s, const double* q, int groups, int samples, double* v) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && error_finite(s[k]) && error_finite(q[k]);
    if (!ok) {
        if (v) v[0] = v[1] = v[2] = (double)NAN;
        return (double)NAN;
    }
    double vp = 0.0, mp = 0.0;                     // 0 + x is x: the sums start at the first channel
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        const double vk = error_var_channel(s[k], q[k], groups, samples);
        if (v) v[k] = vk;
        vp += vk;
        mp += s[k] / (double)samples;
    }
    return sqrt(vp) / (mp + 0.03);
}

// The fixed summation tree of 64 values (one per lane): levels off = 32, 16, .. 1, v[l] += v[l + off] for
// l < off.  The device runs every level's lanes at once (error_tile_kernel, error_frame_kernel), the host
// one after the other: the same additions in the same order, so the same bits.
RT_HD void error_tree_sum_level(double* v, int l, int off) { v[l] += v[l + off]; }
RT_HD void error_tree_max_level(double* v, int l, int off) { v[l] = v[l + off] > v[l] ? v[l + off] : v[l]; }

// What the frame reduction leaves per batch in mapped host memory (rt_capi.cpp: one slot per batch in flight)
struct ErrorWords {
    double frame_error, max_error;
    long long nonfinite, pixels;
    int32_t samples, groups, pad[2];
};

// the frame's figures from the totals over its pixels (host and device: the last step of the reduction)
RT_HD void error_frame_result(double sum_e, double max_e, long long bad, long long pixels, ErrorWords* w) {
    const long long good = pixels - bad;
    w->frame_error = good > 0 ? sum_e / (double)good : (double)NAN;
    w->max_error = good > 0 ? max_e : (double)NAN;
    w->nonfinite = bad;
    w->pixels = pixels;
}

// the threshold stop: a threshold is set, the frame's error is at or under it (NaN: never), and the estimate
// covers at least min_samples samples
RT_HD bool error_converged(double frame_error, double threshold, int samples, int min_samples) {
    return threshold > 0.0 && frame_error <= threshold && samples >= min_samples;
}

// ---- launch interface (pt_error.hip) ----
// q[3 pix + ch] += S_c² / n_c for the chunks of one batch in chunk order: the partials launch_reduce of the same
// `im` reads (samples [im.s_begin, im.s_end) in chunks of im.pool_chunk, 0: the pool's rule), under the same
// `skip` word (ReduceGate::skip, nullptr: always).  Right after the batch's reduce on its stream
hipError_t launch_error_moments(const ImageParams& im, double* q, const double* part, bool tri_bvh, const uint32_t* skip,
                                hipStream_t stream);
// the same for the partials of one pool launch: `chunks` chunks of `chunk` samples over `ns` samples
hipError_t launch_error_moments_chunks(const ImageParams& im, double* q, const double* part, int tiles, int chunks,
                                       int chunk, int ns, const uint32_t* skip, hipStream_t stream);
// per pixel var_mean (n x 3, may be nullptr) and rel_error (n floats, may be nullptr) from the sums and moments
// of `groups` >= 2 groups over `samples` samples; per tile (tile_part, 3 doubles per tile, may be nullptr) the sum
// and the maximum of e_p over the finite pixels and the non-finite count
hipError_t launch_error_estimate(const ImageParams& im, const double* sum, const double* q, int groups, int samples,
                                 double* var_mean, float* rel_error, double* tile_part, const uint32_t* skip,
                                 hipStream_t stream);
// One wave adds the tile partials (lane l: tiles l, l + 64, .. in tile order, then the fixed tree) and writes
// the frame's figures to `out` (mapped host memory) with plain stores; groups < 2: NaN figures, tile_part
// unread.  When error_converged, it sets the sticky `stop` word of the render's gates and `converged`.
struct ErrorFrame {
    int tiles, groups, samples, min_samples;
    long long pixels;
    double threshold;
    const double* tile_part;
    ErrorWords* out;
    uint32_t* stop;
    uint32_t* converged;
    const uint32_t* skip;
};
hipError_t launch_error_frame(const ErrorFrame& f, hipStream_t stream);

}  // namespace rt
