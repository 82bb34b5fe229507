// light_check.cpp — TEST INFRASTRUCTURE: the direct-lighting code of the product headers (pt_core.h occluded /
// illuminate, pt_path.h shade_segment / trace_pixel with F_LIGHT, scene_pack.h's light records and validation)
// compiled for the CPU, so CPU-only tests can compare it with the reference's fixtures bit for bit.  Built
// host-only (tests/lightcheck_binding.py); never part of librt_hip.so.
#include <string>

#include "../../blenderraytracer_amd/csrc/pt_path.h"
#include "../../blenderraytracer_amd/csrc/scene_pack.h"

using namespace rt;

// the host validation rt_scene_create runs before it looks for a device: 0 = valid, else -1 and the message
extern "C" int ptl_validate(const rt_scene_desc* caller, char* err, int err_len) {
    std::string e;
    rt_scene_desc filled;
    if (!desc_as_filled(caller, filled)) e = "abi_version";
    else if (validate_textures(filled, e) && validate_lights(filled, e)) return 0;
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
    return -1;
}

// the descriptor's light count as the library reads it (0 unless extensions == RT_DESC_LIGHTS)
extern "C" int ptl_num_lights(const rt_scene_desc* caller) {
    rt_scene_desc filled;
    return desc_as_filled(caller, filled) ? filled.num_lights : -1;
}

// light.illuminate(point) for n points (n x 3 doubles) -> out n x 7 doubles: direction, colour, distance
extern "C" int ptl_illuminate(const rt_light_desc* l, const double* pts, long long n, double* out) {
    LightRec<double> r{};
    r.type = l->type;
    for (int k = 0; k < 3; ++k) { r.v[k] = l->v[k]; r.color[k] = l->color[k]; }
    r.intensity = l->intensity;
    for (long long i = 0; i < n; ++i) {
        const Illum<double> il = illuminate<double>(r, mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
        const double o[7] = {il.dir.x, il.dir.y, il.dir.z, il.col.x, il.col.y, il.col.z, il.dist};
        for (int k = 0; k < 7; ++k) out[7 * i + k] = o[k];
    }
    return 0;
}

namespace {
struct Packed {
    rt_scene_desc d;
    HostScene hs;
    HostRecords<double> rec;
    SceneView<double> v;
    bool ok = false;
    explicit Packed(const rt_scene_desc* caller) {
        std::string err;
        if (!desc_as_filled(caller, d) || !validate_textures(d, err) || !validate_lights(d, err)) return;
        if (!pack_host(d, hs, err)) return;
        build_bvhs(hs);
        choose_walk(hs, d);
        v = host_view(hs, d, rec);
        ok = hs.bvh_depth <= 64;
    }
};
}  // namespace

// occluded (World order, or accel == RT_ACCEL_BVH: the trees) and, beside it, closest hit t < tmax by the
// closest-hit query of the same walk, for n rays (n x 6 doubles) and limits
extern "C" int ptl_occluded(const rt_scene_desc* caller, int accel, const double* rays, const double* tmax, long long n,
                            uint8_t* out, uint8_t* by_closest) {
    Packed p(caller);
    if (!p.ok) return -1;
    int stack[64];
    const BvhStack stk{stack, 1};
    for (long long i = 0; i < n; ++i) {
        const double* q = rays + 6 * i;
        const V3<double> o = mk(q[0], q[1], q[2]), d = mk(q[3], q[4], q[5]);
        Work w{};
        Closest<double> c;
        if (accel == RT_ACCEL_BVH) {
            out[i] = occluded<double, ACC_BVH_STACK_LIT>(p.v, o, d, tmax[i], w, stk);
            c = closest_hit_acc<double, ACC_BVH_STACK>(p.v, o, d, w, stk);
        } else {
            out[i] = occluded<double, ACC_BRUTE_LIT>(p.v, o, d, tmax[i], w, stk);
            c = closest_hit_acc<double, ACC_BRUTE>(p.v, o, d, w, stk);
        }
        if (by_closest) by_closest[i] = c.kind != HIT_NONE && c.t < tmax[i];
    }
    return 0;
}

// The sample-order render (trace_pixel) through the lit modes when the descriptor carries lights, else as
// tex_check.cpp's ptx_render
extern "C" int ptl_render(const rt_scene_desc* caller, const rt_settings* s, double* sum, uint32_t* segs, uint32_t* draws) {
    Packed p(caller);
    if (!p.ok) return -1;
    const SceneView<double>& v = p.v;
    ImageParams im{};
    im.width = s->width; im.height = s->height;
    im.x0 = s->crop_x0; im.y0 = s->crop_y0;
    im.cw = s->crop_w > 0 ? s->crop_w : s->width;
    im.ch = s->crop_h > 0 ? s->crop_h : s->height;
    im.samples = s->samples;
    im.s_begin = s->sample_begin > 0 ? s->sample_begin : 0;
    im.s_end = s->sample_end > 0 ? s->sample_end : s->samples;
    im.max_depth = s->max_depth;
    im.aa_mode = s->aa_mode;
    im.seedm = host_seed_mix(s->seed);
    int stack[64];
    const BvhStack stk{stack, 1};
    const bool bvh = s->accel == RT_ACCEL_BVH, lit = v.num_lights > 0, tex = v.num_tex > 0;
    for (int cy = 0; cy < im.ch; ++cy)
        for (int cx = 0; cx < im.cw; ++cx) {
            const size_t q = (size_t)cy * im.cw + cx;
            PixelResult r{0, 0, {0, 0, 0}};
            double* acc = sum + 3 * q;
            if (im.max_depth > 0)
                r = lit ? (bvh ? trace_pixel<double, true, ACC_BVH_STACK_LIT>(v, im, cx, cy, im.s_end, acc, stk)
                               : trace_pixel<double, true, ACC_BRUTE_LIT>(v, im, cx, cy, im.s_end, acc, stk))
                  : tex ? (bvh ? trace_pixel<double, true, ACC_BVH_STACK_TEX>(v, im, cx, cy, im.s_end, acc, stk)
                               : trace_pixel<double, true, ACC_BRUTE_TEX>(v, im, cx, cy, im.s_end, acc))
                        : (bvh ? trace_pixel<double, true, ACC_BVH_STACK>(v, im, cx, cy, im.s_end, acc, stk)
                               : trace_pixel<double, true, ACC_BRUTE>(v, im, cx, cy, im.s_end, acc));
            segs[q] = r.segments;
            draws[q] = r.draws;
        }
    return 0;
}

// Shadow rays of the lit render of a crop (scripts/probe_lights.py): the paths of ptl_render traced once more
// with the unlit shading (same decisions: lighting draws nothing), counting at every scattering Lambertian hit
// the lights direct_light would query (cos > 0) and how many of those queries are occluded.
extern "C" int ptl_shadow_rays(const rt_scene_desc* caller, const rt_settings* s, unsigned long long* cast,
                               unsigned long long* blocked) {
    Packed p(caller);
    if (!p.ok || p.v.num_lights <= 0) return -1;
    const SceneView<double>& v = p.v;
    ImageParams im{};
    im.width = s->width; im.height = s->height;
    im.x0 = s->crop_x0; im.y0 = s->crop_y0;
    im.cw = s->crop_w > 0 ? s->crop_w : s->width;
    im.ch = s->crop_h > 0 ? s->crop_h : s->height;
    im.samples = s->samples;
    im.max_depth = s->max_depth;
    im.aa_mode = s->aa_mode;
    im.seedm = host_seed_mix(s->seed);
    int stack[64];
    const BvhStack stk{stack, 1};
    const LightView<double>* lv = light_view(v);
    *cast = *blocked = 0;
    for (int cy = 0; cy < im.ch; ++cy)
        for (int cx = 0; cx < im.cw; ++cx) {
            const int i = im.x0 + cx, row = im.y0 + cy, j = im.height - 1 - row;
            const uint32_t pkey = pixel_key(im.seedm, (uint32_t)row * (uint32_t)im.width + (uint32_t)i);
            for (int sm = 0; sm < s->samples; ++sm) {
                Rng<double> g;
                V3<double> o, d, T = mk<double>(1, 1, 1), L;
                int depth = im.max_depth;
                start_sample(v, im, i, j, pkey, sm, g, o, d);
                for (bool done = depth <= 0; !done;) {
                    Work w{};
                    const Closest<double> c = closest_hit_acc<double, ACC_BVH_STACK>(v, o, d, w, stk);
                    const V3<double> o0 = o, d0 = d;
                    const int depth0 = depth;
                    done = shade_segment<double, F_ALL | F_TEX>(v, c, o, d, T, depth, g, L);
                    if (depth == depth0 || v.mats[c.mat].type != 0) continue;      // no scatter, or not Lambertian
                    const Hit<double> h = hit_record<double>(v, o0, d0, c);
                    for (int k = 0; k < lv->num; ++k) {
                        const Illum<double> il = illuminate<double>(lv->recs[k], h.p);
                        if (!(dot(h.n, il.dir) > 0.0)) continue;
                        ++*cast;
                        if (occluded<double, ACC_BVH_STACK_LIT>(v, h.p, il.dir, il.dist, w, stk)) ++*blocked;
                    }
                }
            }
        }
    return 0;
}
