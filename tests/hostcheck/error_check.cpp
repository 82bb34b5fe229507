// error_check.cpp — TEST INFRASTRUCTURE: the error estimate's per-pixel bodies (pt_error.h) compiled for the CPU
// and driven in the kernels' order (pt_error.hip: one "lane" per pixel of an 8x8 tile, the fixed 64-value tree,
// then the tiles lane-strided), so CPU-only tests can compare them with a rational-arithmetic reference and
// the GPU tests the device with both.  Built host-only (tests/errcheck_binding.py); never part of librt_hip.so.
#include <vector>

#include "../../blenderraytracer_amd/csrc/pool_order.h"
#include "../../blenderraytracer_amd/csrc/pt_error.h"

using namespace rt;

namespace {
ImageParams frame(int cw, int ch) {
    ImageParams im{};
    im.width = im.cw = cw;
    im.height = im.ch = ch;
    return im;
}
int tiles_of(int cw, int ch) { return ((cw + 7) / 8) * ((ch + 7) / 8); }

void tree(double* se, double* sm, double* sb) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int m = 0; m < off; ++m) {
            error_tree_sum_level(se, m, off);
            error_tree_max_level(sm, m, off);
            error_tree_sum_level(sb, m, off);
        }
}
}  // namespace

// error_moments_kernel: q (cw*ch*3) += the moments of part[c][tile][ch][m] (chunks x tiles x 3 x 64 doubles),
// `chunks` chunks of `chunk` samples over `ns` samples
extern "C" int pte_moments(int cw, int ch, double* q, const double* part, int chunks, int chunk, int ns) {
    if (cw <= 0 || ch <= 0 || chunks <= 0 || chunk <= 0 || ns <= (chunks - 1) * chunk || ns > chunks * chunk) return -1;
    const ImageParams im = frame(cw, ch);
    const int tiles = tiles_of(cw, ch);
    const size_t stride = (size_t)tiles * 3 * 64;
    for (int tile = 0; tile < tiles; ++tile) {
        const Tile t = tile_of(im, tile);
        for (int m = 0; m < t.nv; ++m) {
            const size_t px = (size_t)(t.y0 + m / t.vw) * im.cw + (t.x0 + m % t.vw);
            for (int k = 0; k < 3; ++k) {
                const double* p = part + (size_t)tile * 3 * 64 + 64 * k + m;
                double a = q[3 * px + k];
                for (int c = 0; c < chunks; ++c, p += stride) a = error_moment_add(a, *p, error_group_samples(chunk, ns, c));
                q[3 * px + k] = a;
            }
        }
    }
    return 0;
}

// error_tile_kernel and error_frame_kernel: var_mean (cw*ch*3) and rel_error (cw*ch), either may be NULL, and
// the frame's figures (ErrorWords: frame_error, max_error, nonfinite, pixels, samples, groups); returns 1 when
// error_converged, 0 when not, < 0 on bad arguments
extern "C" int pte_estimate(int cw, int ch, const double* sum, const double* q, int groups, int samples, double* var_mean,
                            float* rel_error, double threshold, int min_samples, ErrorWords* out) {
    if (cw <= 0 || ch <= 0 || groups < 2 || samples <= 0 || !out) return -1;
    const ImageParams im = frame(cw, ch);
    const int tiles = tiles_of(cw, ch);
    std::vector<double> tile_part(3 * (size_t)tiles);
    for (int tile = 0; tile < tiles; ++tile) {
        const Tile t = tile_of(im, tile);
        double se[64], sm[64], sb[64];
        for (int m = 0; m < 64; ++m) {
            double e = 0.0, bad = 0.0;
            if (m < t.nv) {
                const size_t px = (size_t)(t.y0 + m / t.vw) * im.cw + (t.x0 + m % t.vw);
                const double r = error_pixel(sum + 3 * px, q + 3 * px, groups, samples, var_mean ? var_mean + 3 * px : nullptr);
                if (rel_error) rel_error[px] = (float)r;
                if (error_finite(r)) e = r;
                else bad = 1.0;
            }
            se[m] = e; sm[m] = e; sb[m] = bad;
        }
        tree(se, sm, sb);
        tile_part[3 * (size_t)tile] = se[0];
        tile_part[3 * (size_t)tile + 1] = sm[0];
        tile_part[3 * (size_t)tile + 2] = sb[0];
    }
    double se[64], sm[64], sb[64];
    for (int m = 0; m < 64; ++m) {
        double e = 0.0, mx = 0.0, bad = 0.0;
        for (int t = m; t < tiles; t += 64) {
            e += tile_part[3 * (size_t)t];
            const double x = tile_part[3 * (size_t)t + 1];
            mx = x > mx ? x : mx;
            bad += tile_part[3 * (size_t)t + 2];
        }
        se[m] = e; sm[m] = mx; sb[m] = bad;
    }
    tree(se, sm, sb);
    error_frame_result(se[0], sm[0], (long long)sb[0], (long long)cw * ch, out);
    out->samples = samples;
    out->groups = groups;
    return error_converged(out->frame_error, threshold, samples, min_samples) ? 1 : 0;
}

extern "C" int pte_words_size(void) { return (int)sizeof(ErrorWords); }
