// filterx_check.cpp — TEST INFRASTRUCTURE: the expanded binary32 sphere filter (pt_core.h sphere_filter_x_pass,
// filter_x_k, make_filter_ray_x) and the binary64 lean grid kernel's walk with it (closest_hit_grid over
// copy_grid_lds<double, true>'s records) of the product headers compiled for the CPU.  Built host-only
// (tests/filterxcheck_binding.py); never part of librt_hip.so.
#include <cmath>
#include <cstring>
#include <random>

#include <string>
#include <vector>

#include "../../blenderraytracer_amd/csrc/pt_path.h"
#include "../../blenderraytracer_amd/csrc/scene_pack.h"
#include "../../blenderraytracer_amd/csrc/pool_order.h"
#include "../../blenderraytracer_amd/csrc/kernel_select.h"

using namespace rt;

// event counts of the kernel's code on the host (pt_core.h RT_HCOUNT; this file is built with -DRT_HOST_COUNTERS)
namespace rt { unsigned long long rt_host_count[16]; }

// The binary64 lean grid kernel's walk, as the device runs it, on the CPU over a crop: the scene staged as
// rt_scene_create stages it (pack_host, build_bvhs, choose_walk, make_records), the grid's LDS copy made by the
// kernel's own copy_grid_lds<double, true> (SphereLeaf::kx in r2p's place), and every pixel traced by
// trace_pixel<double, true, ACC_GRID_LDS_LEAN> (closest_hit_grid<double, true, 0>: make_filter_ray_x on the walk's
// rays, sphere_records_lds with the FilterRayX).  lean == 0: the walk the floor model's event counts have always
// run (pt_hostcheck.cpp ptc_work, ACC_GRID: the old filter on the records in memory).
// out[0..3] = segments, cells visited, sphere records visited, RNG draws; out[4..6] = the crop's summed radiance;
// out[7..22] = the RT_HCOUNT events (HostCount order) counted from the call's start, as ptc_work's callers count
// them: they include the scene set-up's own probe rays (choose_walk), whose share alone is out[23..38].  Returns -1
// if the scene does not walk the grid.
extern "C" int fxc_work(const rt_scene_desc* d, const rt_settings* s, int lean, double* out) {
    HostScene hs;
    HostRecords<double> rec;
    SceneView<double> v{};
    std::string err;
    for (int k = 0; k < 16; ++k) rt_host_count[k] = 0;
    if (!pack_host(*d, hs, err)) return -1;
    build_bvhs(hs);
    choose_walk(hs, *d);
    make_records(hs, *d, rec);
    v.runs = hs.runs.data();
    v.spheres = rec.spheres.data(); v.sphere_filter = rec.sphere_filter.data(); v.sphere_r = rec.sphere_r.data();
    v.sphere_inv_r = rec.sphere_inv_r.data(); v.planes = rec.planes.data();
    v.boxes = rec.boxes.data(); v.tris = rec.tris.data(); v.sphere_mat = hs.sphere_mat.data();
    v.plane_mat = hs.plane_mat.data(); v.box_mat = hs.box_mat.data(); v.tri_mat = hs.tri_mat.data();
    v.mats = rec.mats.data(); v.perm = rec.perm.data();
    v.plane_obj = hs.plane_obj.data(); v.box_obj = hs.box_obj.data();
    v.sphere_nodes = hs.sphere_bvh.data(); v.tri_nodes = hs.tri_bvh.data();
    v.bvh_sphere_leaf = rec.bvh_sphere_leaf.data(); v.bvh_tri_leaf = rec.bvh_tri_leaf.data();
    v.tri_filter = rec.tri_filter.data(); v.tri_exit = hs.tri_exit.data();
    v.big_spheres = rec.big_sphere_leaf.data();
    v.sphere_wide = hs.sphere_wide.data(); v.tri_wide = hs.tri_wide.data();
    v.grid_cell = hs.grid_cell.data(); v.grid_leaf = rec.grid_leaf.data();
    fill_view_constants(v, hs, *d);
    if (v.num_grid_cells <= 0 || v.num_tri_nodes != 0) return -1;
    std::vector<rt_u4> grec(grid_lds_rec_bytes(v) / 16 + 1);
    std::vector<int> gcell((size_t)v.num_grid_cells + 1);
    copy_grid_lds<double, true>(v, grec.data(), gcell.data(), 0, 1);
    ImageParams im{};
    im.width = s->width; im.height = s->height;
    im.x0 = s->crop_x0; im.y0 = s->crop_y0;
    im.cw = s->crop_w > 0 ? s->crop_w : s->width;
    im.ch = s->crop_h > 0 ? s->crop_h : s->height;
    im.samples = s->samples;
    im.s_begin = 0;
    im.s_end = s->samples;
    im.max_depth = s->max_depth;
    im.aa_mode = s->aa_mode;
    im.seedm = host_seed_mix(s->seed);
    int stack[64];
    BvhStack stk{stack, 1};
    stk.gcell = gcell.data();
    stk.grec = grec.data();
    for (int k = 0; k < 23; ++k) out[k] = 0;
    for (int k = 0; k < 16; ++k) out[23 + k] = (double)rt_host_count[k];
    for (int cy = 0; cy < im.ch; ++cy)
        for (int cx = 0; cx < im.cw; ++cx) {
            double acc[3] = {0, 0, 0};
            const PixelResult r = lean ? trace_pixel<double, true, ACC_GRID_LDS_LEAN>(v, im, cx, cy, im.s_end, acc, stk)
                                       : trace_pixel<double, true, ACC_GRID>(v, im, cx, cy, im.s_end, acc);
            out[0] += r.segments; out[1] += r.work.nodes; out[2] += r.work.spheres; out[3] += r.draws;
            for (int k = 0; k < 3; ++k) out[4 + k] += acc[k];
        }
    for (int k = 0; k < 16; ++k) out[7 + k] = (double)rt_host_count[k];
    return 0;
}

// Adversarial check of the expanded filter against the binary64 discriminant and the old filter, on the same
// cases.  mode 0: pt_hostcheck.cpp's ptc_sphere_filter_check generator (8 decades of scale, rays aimed at
// |p| = r (1 +- eps)); mode 1: the same with the centre moved out to |c| / r up to 10^6; mode 2: the origin
// on the sphere (a segment that leaves it), half of the directions tangent to within 10^-8.
// mutation 0: the product's record and ray; 1: k rounded DOWN by 64 ulps; 2: the ray's A with the wrong sign.
// out[0] violations of the new filter (rejected although disc64 >= 0), out[1] of the old one, out[2] worst
// |X' - Y - margin| / Q of the new one, out[3] / out[4] fraction of the sure misses the new / old rejects,
// out[5] the number of sure misses.
extern "C" int fxc_filter_check(long long n, unsigned seed, int mode, int mutation, double* out) {
    std::mt19937_64 gen(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    long long viol_new = 0, viol_old = 0, misses = 0, rej_new = 0, rej_old = 0;
    double worst = 0;
    for (long long it = 0; it < n; ++it) {
        const double scale = std::pow(10.0, 4.0 * U(gen) + 0.5);      // scene scale 10^-3.5 .. 10^4.5
        const double r = std::fabs(U(gen)) * scale * 0.5 + 1e-9;
        double c[3] = {U(gen) * scale, U(gen) * scale, U(gen) * scale};
        if (mode == 1) {
            const double cl = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + 1e-300;
            const double want = r * std::pow(10.0, 6.0 * std::fabs(U(gen)));
            for (int k = 0; k < 3; ++k) c[k] *= want / cl;
        }
        double dd[3] = {U(gen), U(gen), U(gen)};
        const double dl = std::pow(10.0, 3.0 * U(gen));                // |d| 10^-3 .. 10^3 (unnormalized)
        double w[3] = {U(gen), U(gen), U(gen)};
        const double d2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
        const double wd = (w[0] * dd[0] + w[1] * dd[1] + w[2] * dd[2]) / d2;
        for (int k = 0; k < 3; ++k) w[k] -= wd * dd[k];                // w perpendicular to d
        const double wn = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        const double eps = (it & 1 ? 1 : -1) * std::pow(10.0, -7.0 * std::fabs(U(gen)) - 1.0);
        const double back = U(gen) * 4 * scale;
        double o[3], d[3];
        for (int k = 0; k < 3; ++k) {
            if (mode == 2) {
                // o = c + r w/|w| on the sphere; d tangent (along dd, perpendicular to w) plus, for every
                // second case, a radial part of relative size eps
                o[k] = c[k] + w[k] / wn * r;
                d[k] = (dd[k] + ((it & 2) ? eps * 1e-1 * std::sqrt(d2) * w[k] / wn : U(gen) * w[k])) * dl;
            } else {
                d[k] = dd[k] * dl;
                o[k] = c[k] + w[k] / wn * r * (1 + eps) - dd[k] * back;
            }
        }
        const double ocx = o[0] - c[0], ocy = o[1] - c[1], ocz = o[2] - c[2];
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const double hb = ocx * d[0] + ocy * d[1] + ocz * d[2];
        const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r * r;
        const double disc64 = hb * hb - a * cc;
        const double kk = 2.0 * (c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + r * r;
        // the record as scene_pack.h make_records builds it
        const SphereFilter f{(float)c[0], (float)c[1], (float)c[2], (float)((r * r + filter_margin() * kk) * (1.0 + 0x1p-20))};
        SphereFilterX fx{f.cx, f.cy, f.cz, filter_x_k(f)};
        const FilterRay fr = make_filter_ray(V3<double>{o[0], o[1], o[2]}, V3<double>{d[0], d[1], d[2]});
        FilterRayX frx = make_filter_ray_x(fr);
        if (mutation == 1) for (int s = 0; s < 64; ++s) fx.k = nextafterf(fx.k, -INFINITY);
        if (mutation == 2) frx.A = -frx.A;
        const bool pass_old = sphere_filter_pass(f, fr), pass_new = sphere_filter_x_pass(fx, frx);
        if (disc64 >= 0 && !pass_new) ++viol_new;
        if (disc64 >= 0 && !pass_old) ++viol_old;
        if (disc64 < 0) { ++misses; rej_new += !pass_new; rej_old += !pass_old; }
        // observed |X' - Y - margin| / Q: X' as sphere_filter_x_pass evaluates it, Y = disc64 / |d|^2, margin =
        // r2p - r^2 + delta of the record and the ray (sphere_filter_bound)
        const float h = __builtin_fmaf(-fx.cx, frx.dx, __builtin_fmaf(-fx.cy, frx.dy, __builtin_fmaf(-fx.cz, frx.dz, frx.A)));
        const float e = __builtin_fmaf(frx.ox2, fx.cx, __builtin_fmaf(frx.oy2, fx.cy, __builtin_fmaf(frx.oz2, fx.cz, fx.k + frx.B)));
        const double X = (double)__builtin_fmaf(h, h, e);
        if ((X < 0) == pass_new && X == X) return -1;                 // the restatement above is the product's
        const double margin = ((double)f.r2p - r * r) + (double)fr.delta;
        double Q = r * r;
        for (int q = 0; q < 3; ++q) Q += (std::fabs(o[q]) + std::fabs(c[q])) * (std::fabs(o[q]) + std::fabs(c[q]));
        const double ratio = std::fabs(X - disc64 / a - margin) / Q;
        if (ratio > worst) worst = ratio;
    }
    out[0] = (double)viol_new; out[1] = (double)viol_old; out[2] = worst;
    out[3] = misses ? (double)rej_new / misses : 0; out[4] = misses ? (double)rej_old / misses : 0;
    out[5] = (double)misses;
    return 0;
}
