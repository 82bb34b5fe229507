// guided_check.cpp — TEST INFRASTRUCTURE: the feature-buffer and guided-filter code of the product headers
// (pt_path.h aov_pixel, pt_guided.h guided_pixel / guided_level / guided_params_ok) compiled for the CPU, so
// CPU-only tests can compare it with tests/guided_ref.py bit for bit, and the GPU tests the device with it.
// Built host-only (tests/guidedcheck_binding.py); never part of librt_hip.so.
#include <string>
#include <vector>

#include "../../blenderraytracer_amd/csrc/pt_guided.h"
#include "../../blenderraytracer_amd/csrc/scene_pack.h"

using namespace rt;

namespace {
// host-side scene staging as rt_scene_create builds it, in either precision, textures included
template <class R>
struct Packed {
    rt_scene_desc d;
    HostScene hs;
    HostRecords<R> rec;
    SceneView<R> v{};
    bool ok = false;
    explicit Packed(const rt_scene_desc* caller) {
        std::string err;
        if (!desc_as_filled(caller, d) || !validate_textures(d, err) || !validate_lights(d, err)) return;
        if (!pack_host(d, hs, err)) return;
        build_bvhs(hs);
        choose_walk(hs, d);
        make_records(hs, d, rec);
        v.runs = hs.runs.data();
        v.spheres = rec.spheres.data(); v.sphere_filter = rec.sphere_filter.data(); v.sphere_r = rec.sphere_r.data();
        v.sphere_inv_r = rec.sphere_inv_r.data();
        v.planes = rec.planes.data(); v.boxes = rec.boxes.data(); v.tris = rec.tris.data();
        v.sphere_mat = hs.sphere_mat.data(); v.plane_mat = hs.plane_mat.data(); v.box_mat = hs.box_mat.data();
        v.tri_mat = hs.tri_mat.data(); v.mats = rec.mats.data();
        v.plane_obj = hs.plane_obj.data(); v.box_obj = hs.box_obj.data();
        v.sphere_nodes = hs.sphere_bvh.data(); v.tri_nodes = hs.tri_bvh.data();
        v.bvh_sphere_leaf = rec.bvh_sphere_leaf.data(); v.bvh_tri_leaf = rec.bvh_tri_leaf.data();
        v.tri_filter = rec.tri_filter.data(); v.tri_exit = hs.tri_exit.data();
        v.big_spheres = rec.big_sphere_leaf.data();
        v.sphere_wide = hs.sphere_wide.data(); v.tri_wide = hs.tri_wide.data();
        v.grid_cell = hs.grid_cell.data(); v.grid_leaf = rec.grid_leaf.data();
        if (!rec.tex_recs.empty())
            rec.set_tex_view(TexView<R>{rec.tex_recs.data(), rec.tex_perms.data(), rec.mat_tex.data(),
                                        (int)rec.tex_recs.size(), (int)(rec.tex_perms.size() / 512)});
        v.perm = rec.perm.data();
        fill_view_constants(v, hs, d);
        ok = hs.bvh_depth <= 64;                     // the host walks use 64-entry stacks
    }
};

template <class R>
int aovs(const rt_scene_desc* caller, const rt_settings* s, float* guides, int* kind, int* idx) {
    Packed<R> p(caller);
    if (!p.ok) return -1;
    const int cw = s->crop_w > 0 ? s->crop_w : s->width, ch = s->crop_h > 0 ? s->crop_h : s->height;
    int stack[64];
    const BvhStack stk{stack, 1};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t q = (size_t)cy * cw + cx;
            const int i = s->crop_x0 + cx, j = s->height - 1 - (s->crop_y0 + cy);
            const AovHit h = s->accel == RT_ACCEL_BVH ? aov_pixel<R, ACC_BVH_STACK>(p.v, s->width, s->height, i, j, stk, guides + 8 * q)
                                                      : aov_pixel<R, ACC_BRUTE>(p.v, s->width, s->height, i, j, stk, guides + 8 * q);
            if (kind) kind[q] = h.kind;
            if (idx) idx[q] = h.idx;
        }
    return 0;
}

template <class R>
int closest_hits(const rt_scene_desc* caller, int accel, const double* rays, long long n, double* t, int* kind, int* idx) {
    Packed<R> p(caller);
    if (!p.ok) return -1;
    int stack[64];
    const BvhStack stk{stack, 1};
    for (long long r = 0; r < n; ++r) {
        const double* q = rays + 6 * r;
        const V3<R> o = mk<R>((R)q[0], (R)q[1], (R)q[2]), d = mk<R>((R)q[3], (R)q[4], (R)q[5]);
        Work w{};
        const Closest<R> c = accel == RT_ACCEL_BVH ? closest_hit_acc<R, ACC_BVH_STACK>(p.v, o, d, w, stk)
                                                   : closest_hit_acc<R, ACC_BRUTE>(p.v, o, d, w, stk);
        t[r] = c.kind == HIT_NONE ? (double)INFINITY : (double)c.t;
        kind[r] = c.kind;
        idx[r] = c.kind == HIT_NONE ? -1 : c.idx;
    }
    return 0;
}

// aov_texture_value of texture `tex` at n points (n x 3 doubles, rounded to R) -> rgb (n x 3 doubles)
template <class R>
int texture_values(const rt_scene_desc* caller, int tex, const double* pts, long long n, double* rgb) {
    Packed<R> p(caller);
    if (!p.ok || p.v.num_tex <= 0 || tex < 0 || tex >= p.v.num_tex) return -1;
    const TexView<R>* tv = tex_view(p.v);
    for (long long i = 0; i < n; ++i) {
        const V3<R> v = aov_texture_value<R>(tv, tex, mk<R>((R)pts[3 * i], (R)pts[3 * i + 1], (R)pts[3 * i + 2]));
        rgb[3 * i] = (double)v.x; rgb[3 * i + 1] = (double)v.y; rgb[3 * i + 2] = (double)v.z;
    }
    return 0;
}
}  // namespace

// the albedo buffer's texture function (pt_path.h aov_texture_value) on the CPU
extern "C" int ptg_texture_values(const rt_scene_desc* caller, int precision, int tex, const double* pts, long long n,
                                  double* rgb) {
    return precision == RT_PREC_F32 ? texture_values<float>(caller, tex, pts, n, rgb)
                                    : texture_values<double>(caller, tex, pts, n, rgb);
}

// rt_aovs of the settings' frame (precision, accel RT_ACCEL_BVH: the general ordered walk, else World order):
// guides n x 8 floats, kind and idx n ints (either may be NULL)
extern "C" int ptg_aovs(const rt_scene_desc* caller, const rt_settings* s, float* guides, int* kind, int* idx) {
    return s->precision == RT_PREC_F32 ? aovs<float>(caller, s, guides, kind, idx) : aovs<double>(caller, s, guides, kind, idx);
}

// rt_closest_hits on the CPU (the same outputs)
extern "C" int ptg_closest_hits(const rt_scene_desc* caller, int precision, int accel, const double* rays, long long n,
                                double* t, int* kind, int* idx) {
    return precision == RT_PREC_F32 ? closest_hits<float>(caller, accel, rays, n, t, kind, idx)
                                    : closest_hits<double>(caller, accel, rays, n, t, kind, idx);
}

extern "C" int ptg_params_ok(const rt_guided_params* p) { return guided_params_ok(p) ? 1 : 0; }

// rt_guided_filter_device on the CPU: every level through guided_level / guided_pixel, never in place
extern "C" int ptg_filter(int w, int h, const rt_guided_params* p, const double* color, const float* guides, double* out) {
    if (!guided_params_ok(p) || w <= 0 || h <= 0) return -1;
    const size_t n = (size_t)w * h;
    // guided_pixel takes 16-byte aligned guide records
    std::vector<float4> g((8 * n + 3) / 4);
    float* gp = reinterpret_cast<float*>(g.data());
    std::copy(guides, guides + 8 * n, gp);
    std::vector<double> a(color, color + 3 * n), b(3 * n);
    for (int l = 0; l < p->levels; ++l) {
        const GuidedLevel L = guided_level(w, h, *p, l);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) guided_pixel(L, a.data(), gp, x, y, &b[3 * ((size_t)y * w + x)]);
        a.swap(b);
    }
    std::copy(a.begin(), a.end(), out);
    return 0;
}
