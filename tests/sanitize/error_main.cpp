// error_main.cpp — TEST INFRASTRUCTURE: a stand-alone program over the error estimate's host build
// (tests/hostcheck/error_check.cpp: the bodies of csrc/pt_error.h in the kernels' order), linked with
// -fsanitize=address,undefined by tests/test_error_estimate.py.  Ragged frames, short last chunks, buffers of
// exactly the size the kernels index: an out-of-bounds index or undefined arithmetic ends the run.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../hostcheck/error_check.cpp"

int main() {
    const int frames[][2] = {{1, 1}, {8, 8}, {11, 9}, {65, 3}, {24, 20}, {7, 17}};
    unsigned long long state = 88172645463325252ull;
    auto next = [&] {                                   // xorshift64: values in [0, 4)
        state ^= state << 13; state ^= state >> 7; state ^= state << 17;
        return (double)(state >> 11) * (4.0 / 9007199254740992.0);
    };
    for (const auto& f : frames) {
        const int cw = f[0], ch = f[1], tiles = tiles_of(cw, ch);
        const size_t n = (size_t)cw * ch;
        std::vector<double> q(3 * n, 0.0), sum(3 * n, 0.0), var(3 * n);
        std::vector<float> rel(n);
        int groups = 0, samples = 0;
        const int batches[][3] = {{2, 4, 8}, {2, 4, 6}, {1, 5, 5}, {3, 3, 7}};    // chunks, chunk, samples
        for (const auto& b : batches) {
            std::vector<double> part((size_t)b[0] * tiles * 3 * 64);
            for (double& v : part) v = next();
            if (pte_moments(cw, ch, q.data(), part.data(), b[0], b[1], b[2]) != 0) return 1;
            const ImageParams im = frame(cw, ch);
            for (int tile = 0; tile < tiles; ++tile) {                            // reduce_kernel's additions
                const Tile t = tile_of(im, tile);
                for (int m = 0; m < t.nv; ++m) {
                    const size_t px = (size_t)(t.y0 + m / t.vw) * cw + (t.x0 + m % t.vw);
                    for (int c = 0; c < b[0]; ++c)
                        for (int k = 0; k < 3; ++k) sum[3 * px + k] += part[((size_t)c * tiles + tile) * 192 + 64 * k + m];
                }
            }
            groups += b[0];
            samples += b[2];
        }
        if (n > 2) sum[3] = NAN;                                                  // one non-finite pixel
        ErrorWords w;
        const int conv = pte_estimate(cw, ch, sum.data(), q.data(), groups, samples, var.data(), rel.data(), 1e9, 0, &w);
        if (conv != 1 || w.pixels != (long long)n || w.nonfinite != (n > 2 ? 1 : 0) || !(w.frame_error >= 0.0)) {
            fprintf(stderr, "%dx%d: converged %d, %lld pixels, %lld non-finite, frame error %g\n", cw, ch, conv, w.pixels,
                    w.nonfinite, w.frame_error);
            return 1;
        }
        printf("%dx%d ok: %d groups, %d samples, frame error %.6f\n", cw, ch, groups, samples, w.frame_error);
    }
    return 0;
}
