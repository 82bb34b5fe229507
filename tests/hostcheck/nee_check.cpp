// nee_check.cpp — TEST INFRASTRUCTURE: the emitter-sampling code of the product headers (scene_pack.h
// build_emitters, pt_core.h sample_emitter / emitter_query, pt_path.h emitter_light / emission_weight and
// shade_segment / trace_pixel with F_NEE, kernel_select.h) compiled for the CPU, so CPU-only tests can pin it
// against tests/nee_ref.py and check its statistics, and GPU tests can compare the device with it bit for bit.
// Built host-only (tests/neecheck_binding.py), once per RT_NEE_MUTATION; never part of librt_hip.so.
#include <string>

#include "../../blenderraytracer_amd/csrc/kernel_select.h"
#include "../../blenderraytracer_amd/csrc/pt_path.h"
#include "../../blenderraytracer_amd/csrc/scene_pack.h"

using namespace rt;

namespace {
struct Packed {
    rt_scene_desc d;
    HostScene hs;
    HostRecords<double> rec;
    SceneView<double> v;
    std::string err;
    bool ok = false;
    Packed(const rt_scene_desc* caller, bool emitters) {
        if (!desc_as_filled(caller, d) || !validate_textures(d, err) || !validate_lights(d, err)) return;
        if (!pack_host(d, hs, err)) return;
        if (!build_emitters(hs, d, emitters, err)) return;
        build_bvhs(hs);
        choose_walk(hs, d);
        v = host_view(hs, d, rec);
        ok = hs.bvh_depth <= 64;
    }
};
}  // namespace

// the emitter list as rt_scene_set_emitter_sampling(scene, 1) builds it: N, or -1; kind / idx: the first
// min(N, cap) entries; records (optional): 16 doubles each — g[12], le[3], area
extern "C" int ptn_emitters(const rt_scene_desc* caller, int* kind, int* idx, double* records, int cap) {
    Packed p(caller, true);
    if (!p.ok) return -1;
    const int n = (int)p.hs.emit_idx.size();
    for (int e = 0; e < n && e < cap; ++e) {
        kind[e] = p.hs.emit_kind[e];
        idx[e] = p.hs.emit_idx[e];
        if (records) {
            const EmitterRec<double>& r = p.rec.emitter_recs[e];
            for (int k = 0; k < 12; ++k) records[16 * e + k] = r.g[k];
            for (int k = 0; k < 3; ++k) records[16 * e + 12 + k] = r.le[k];
            records[16 * e + 15] = r.area;
        }
    }
    return n;
}

// build_emitters' own limit: a list of `count` identical emitters (0: accepted, -1: refused)
extern "C" int ptn_emitter_limit(long long count) {
    HostScene hs;
    rt_material_desc m{};
    m.type = RT_MAT_EMISSIVE;
    m.emission[0] = 1.0;
    rt_scene_desc d{};
    d.materials = &m;
    d.num_materials = 1;
    for (long long i = 0; i < count; ++i) {
        hs.spheres.insert(hs.spheres.end(), {0.0, 0.0, 0.0, 1.0});
        hs.sphere_mat.push_back(0);
        hs.sphere_obj.push_back((int)i);
    }
    std::string err;
    return build_emitters(hs, d, true, err) ? 0 : -1;
}

// emitter_query (World order, or accel == RT_ACCEL_BVH: the trees) for n queries (points n x 6: x, n; keys n),
// rt_emitter_samples' outputs, and beside them pO_sample = p_l N and pO_hit, the hit side's density
// (emitter_hit_pdf) for the ray (x, omega) and the sampled primitive at t_e (0 where there is no candidate)
extern "C" int ptn_samples(const rt_scene_desc* caller, int accel, const double* pts, const uint32_t* keys, long long n,
                           int32_t* emitter, double* omega, double* p_l, double* t_e, uint8_t* visible, double* pO_hit) {
    Packed p(caller, true);
    if (!p.ok || p.v.num_emitters <= 0) return -1;
    int stack[64];
    const BvhStack stk{stack, 1};
    const EmitterView<double>* ev = emitter_view(p.v);
    for (long long i = 0; i < n; ++i) {
        const double* q = pts + 6 * i;
        const V3<double> x = mk(q[0], q[1], q[2]), nn = mk(q[3], q[4], q[5]);
        Work w{};
        const EmitterQuery<double> s = accel == RT_ACCEL_BVH ? emitter_query<double, ACC_BVH_STACK_NEE>(p.v, x, nn, keys[i], w, stk)
                                                             : emitter_query<double, ACC_BRUTE_NEE>(p.v, x, nn, keys[i], w, stk);
        emitter[i] = s.e;
        omega[3 * i] = s.om.x; omega[3 * i + 1] = s.om.y; omega[3 * i + 2] = s.om.z;
        p_l[i] = s.p_l;
        t_e[i] = s.t_e;
        visible[i] = s.visible ? 1 : 0;
        if (pO_hit) {
            pO_hit[i] = 0.0;
            const EmitterRec<double>& er = ev->recs[s.e];
            double pO;
            if (s.t_e > 0.0 &&
                emitter_hit_pdf(p.v, Closest<double>{s.t_e, er.kind == EMIT_SPHERE ? HIT_SPHERE : HIT_TRI, er.idx, 0, 0}, x, s.om, pO))
                pO_hit[i] = pO;
        }
    }
    return 0;
}

// The sample-order render (trace_pixel) with emitter sampling `on`: through the F_NEE modes when the scene then
// lists emitters, else the kernels it always ran (light_check.cpp's ptl_render)
extern "C" int ptn_render(const rt_scene_desc* caller, const rt_settings* s, int on, double* sum, uint32_t* segs,
                          uint32_t* draws) {
    Packed p(caller, on != 0);
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
    const bool bvh = s->accel == RT_ACCEL_BVH, nee = v.num_emitters > 0, lit = v.num_lights > 0, tex = v.num_tex > 0;
    for (int cy = 0; cy < im.ch; ++cy)
        for (int cx = 0; cx < im.cw; ++cx) {
            const size_t q = (size_t)cy * im.cw + cx;
            PixelResult r{0, 0, {0, 0, 0}};
            double* acc = sum + 3 * q;
            if (im.max_depth > 0)
                r = nee ? (bvh ? trace_pixel<double, true, ACC_BVH_STACK_NEE>(v, im, cx, cy, im.s_end, acc, stk)
                               : trace_pixel<double, true, ACC_BRUTE_NEE>(v, im, cx, cy, im.s_end, acc, stk))
                  : lit ? (bvh ? trace_pixel<double, true, ACC_BVH_STACK_LIT>(v, im, cx, cy, im.s_end, acc, stk)
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

// select_kernel's mode for this scene with emitter sampling `on` (binary64), and the walk it reports
extern "C" int ptn_select(const rt_scene_desc* caller, int on, int bvh, int pool, int* walk) {
    Packed p(caller, on != 0);
    if (!p.ok) return -1;
    const KernelChoice k = select_kernel<double>(scene_facts(p.v), 0, bvh != 0, pool != 0, SelectKnobs{});
    if (walk) *walk = walk_report(k.acc);
    return (int)k.acc;
}

// Shadow queries of the emitter-sampling render of a crop (scripts/probe_emitters.py): per sample the occlusion
// queries emitter_light reaches, and how many of them are occluded — the paths traced once more with the plain
// shading (emitter sampling draws from its own stream: same decisions)
extern "C" int ptn_shadow_queries(const rt_scene_desc* caller, const rt_settings* s, unsigned long long* cast,
                                  unsigned long long* blocked) {
    Packed p(caller, true);
    if (!p.ok || p.v.num_emitters <= 0) return -1;
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
    const EmitterView<double>* ev = emitter_view(v);
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
                    if (depth == depth0 || v.mats[c.mat].type != 0 || depth0 <= 1) continue;
                    const Hit<double> h = hit_record<double>(v, o0, d0, c);
                    Rng<double> ge{lowbias32(g.key ^ lowbias32((uint32_t)(im.max_depth - depth0) + 0x4E454531u)), 0};
                    const EmitterDraw<double> e = sample_emitter(ev, v.num_emitters, h.p, ge);
                    double te;
                    if (!e.ok || !(dot(h.n, e.om) > 0.0) || !emitter_candidate(ev->recs[e.e], h.p, e.om, te)) continue;
                    ++*cast;
                    if (occluded<double, ACC_BVH_STACK_NEE>(v, h.p, e.om, te, w, stk)) ++*blocked;
                }
            }
        }
    return 0;
}
