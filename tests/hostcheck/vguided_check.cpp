// vguided_check.cpp — TEST INFRASTRUCTURE: the variance-guided filter's code of the product header
// (pt_vguided.h vguided_pixel / vguided_level / vguided_sigma_ok) compiled for the CPU, so CPU-only tests can
// compare it with tests/vguided_ref.py bit for bit, and the GPU tests the device with it.
// Built host-only (tests/vguidedcheck_binding.py); never part of librt_hip.so.
#include <algorithm>
#include <vector>

#include "../../blenderraytracer_amd/csrc/pt_vguided.h"

using namespace rt;

extern "C" int ptv_sigma_ok(double sigma_variance) { return vguided_sigma_ok(sigma_variance) ? 1 : 0; }

// rt_guided_filter_variance_device on the CPU: every level through vguided_level / vguided_pixel, never in
// place; out and var_out: the last level's colour and variance
extern "C" int ptv_filter(int w, int h, const rt_guided_params* p, double sigma_variance, const double* color,
                          const double* var, const float* guides, double* out, double* var_out) {
    if (!guided_params_ok(p) || !vguided_sigma_ok(sigma_variance) || w <= 0 || h <= 0) return -1;
    const size_t n = (size_t)w * h;
    // vguided_pixel takes 16-byte aligned guide records
    std::vector<float4> g((8 * n + 3) / 4);
    float* gp = reinterpret_cast<float*>(g.data());
    std::copy(guides, guides + 8 * n, gp);
    std::vector<double> a(color, color + 3 * n), b(3 * n), va(var, var + 3 * n), vb(3 * n);
    for (int l = 0; l < p->levels; ++l) {
        const VGuidedLevel L = vguided_level(w, h, *p, sigma_variance, l);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t q = 3 * ((size_t)y * w + x);
                vguided_pixel(L, a.data(), va.data(), gp, x, y, &b[q], &vb[q]);
            }
        a.swap(b);
        va.swap(vb);
    }
    std::copy(a.begin(), a.end(), out);
    std::copy(va.begin(), va.end(), var_out);
    return 0;
}
