// pt_path.h — the per-lane body of the megakernel: one pixel, samples [s_begin, s_end).
//
// The recursion of rayColor (js/ray-tracer.js:102-123) is flattened into one loop whose body is
// exactly one world.hit: when a path terminates (miss, emissive, absorption, depth cap) the lane
// adds its radiance to the pixel sum and immediately regenerates the camera ray of its next sample
// (path regeneration), so the lanes of a wave stay busy until their pixel is done.
// Radiance is carried as a forward throughput product T (att_0*att_1*...)*E instead of the
// recursion's att_0*(att_1*(...*E)): the same factors, rounded in a different order (<= a few ulp);
// every path DECISION is unaffected.
#pragma once
#include <type_traits>

#include "pt_core.h"

namespace rt {

struct ImageParams {
    int width, height;         // full image (pixel keys)
    int x0, y0, cw, ch;        // crop window (top-down rows)
    int samples;               // sampleCount (divisor of the mean)
    int s_begin, s_end;        // sample range of this launch
    int max_depth;
    int aa_mode;
    uint32_t seedm;            // seed_mix(seed)
    int pool_chunk;            // samples per sample-pool wave (0: pool_chunk's rule for this launch's samples)
    // fused batches (launch_trace_batches): the launch traces batches of batch_samples samples from
    // s_begin, batch_chunks chunks each, batch-major (chunk index c of the launch = batch c / batch_chunks);
    // 0: one batch
    int batch_samples, batch_chunks;
    // the whole-batch multi-device split (rt_capi.cpp): the launch's batches are every batch_ways-th batch
    // of the render (batch b starts batch_ways * batch_samples samples after batch b - 1, and raises the
    // flag batch_flag[b * batch_ways]); 0 or 1: consecutive batches
    int batch_ways;
    // pixel bands (rt_trace_device_bands, pool_order.h band_item): the launch's items band-major over `bands`
    // horizontal bands of whole tile rows, band_chunks chunks each; band b's items counted in
    // Counters::batch_count[b], its flag raised when all are done; 0: no bands
    int bands, band_chunks;
};

// Stochastic AA offsets (ray-tracer.js:136-141): sqrt, cos and sin in binary64 are long code that
// the default supersampling never runs, so they stay out of line (RT_COLD, pt_core.h).  Arguments and
// result by value: no local's address escapes into the call.
template <class R> struct AaUv { R u, v; };
template <class R>
RT_COLD_HD AaUv<R> stochastic_uv(uint32_t key, int i, int j, int width, int height) {
    Rng<R> g{key, 0};
    R r1 = g.next(), r2 = g.next();
    R ox = sqrt(r1) * js_cos<R>((R)2 * (R)3.141592653589793 * r2);       // ray-tracer.js:130-131, V8's Math.cos / sin
    R oy = sqrt(r1) * js_sin<R>((R)2 * (R)3.141592653589793 * r2);
    return AaUv<R>{((R)i + (R)0.5 + ox * (R)0.5) / (R)width, ((R)j + (R)0.5 + oy * (R)0.5) / (R)height};
}

#ifndef RT_OPAQUE_WH
#define RT_OPAQUE_WH 0
#endif
// The camera ray (camera.js:38-51) from the camera's 22 words at cp (SceneView: cam_o, cam_llc, cam_h,
// cam_v, cam_u, cam_vv, cam_w, lens_radius, contiguous)
template <class R, class P, int FEAT = F_ALL>
RT_HD void camera_ray(const SceneView<R>& sc, R u, R v, Rng<R>& g, V3<R>& o, V3<R>& d, P cp) {
    const V3<R> co = mk<R>(cp[0], cp[1], cp[2]);
    const V3<R> llc = mk<R>(cp[3], cp[4], cp[5]);
    const V3<R> hor = mk<R>(cp[6], cp[7], cp[8]);
    const V3<R> ver = mk<R>(cp[9], cp[10], cp[11]);
    const V3<R> cu = mk<R>(cp[12], cp[13], cp[14]);
    const V3<R> cv = mk<R>(cp[15], cp[16], cp[17]);
    V3<R> rd = random_in_unit_disk(g) * (R)cp[21];
    if ((FEAT & F_CAMALL) != 0 && sc.cam_ortho) {
        o = (co + cu * rd.x) + cv * rd.y;
        d = normalize((((llc + hor * u) + ver * v) - o) + mk<R>(cp[18], cp[19], cp[20]) * (R)-1);
    } else {
        o = co + (cu * rd.x + cv * rd.y);
        d = ((llc + hor * u) + ver * v) - o;
    }
}

// RELOAD (RT_CAM_RELOAD: the binary32 LDS pool kernel): the camera words read from the kernel-argument
// segment at every sample start (scalar loads through a pointer the compiler cannot hoist) instead of
// kept live in SGPRs across the segment loop, where the kernel's SGPR spills are reloaded by VALU
// v_readlane instructions: RTOW f32 +1.6 % (SGPR spills 61 -> 49).  In binary64 the freed SGPRs went to
// spills inside the walk instead (round 5: RTOW -0.3 %, mesh50k -9 %, Cornell -16 %; round 6's lean
// one-wave kernels: mesh50k -10 %), so binary32 and, with pt_core.h RT_SC_RELOAD, the binary64 lean
// grid kernel only.
#ifndef RT_CAM_RELOAD
#define RT_CAM_RELOAD 1
#endif
#ifndef RT_CAM_RELOAD_LEAN64
#define RT_CAM_RELOAD_LEAN64 1    // the binary64 lean grid kernel reloads too (round 6, with RT_SC_RELOAD)
#endif
// FEAT without F_CAMALL (the lean kernels): supersampling AA and the perspective camera only
template <class R, bool RELOAD = false, int FEAT = F_ALL>
RT_HD void start_sample(const SceneView<R>& sc, const ImageParams& im, int i, int j, uint32_t pkey, int s, Rng<R>& g,
                        V3<R>& o, V3<R>& d) {
    RT_HCOUNT(HC_SAMPLES, 1);
    g.key = sample_key(pkey, (uint32_t)s);
    g.k = 0;
    R u, v;                                                                   // ray-tracer.js:125-149
#if RT_OPAQUE_WH && defined(__HIP_DEVICE_COMPILE__)
    // (R)width / (R)height converted here from the kernel-argument SGPRs at every sample start instead of
    // hoisted out of the pool loop by the compiler (they then live in scratch): A/B
    int iw = im.width, ih = im.height;
    asm volatile("" : "+s"(iw), "+s"(ih));
    const R width = (R)iw, height = (R)ih;
#else
    const R width = (R)im.width, height = (R)im.height;
#endif
    if ((FEAT & F_CAMALL) == 0) {
        u = ((R)i + g.next()) / width;
        v = ((R)j + g.next()) / height;
    } else if (im.aa_mode == 1) {
        const AaUv<R> uv = stochastic_uv<R>(g.key, i, j, im.width, im.height);
        u = uv.u;
        v = uv.v;
        g.k = 2;
    } else if (im.aa_mode == 0) {
        u = ((R)i + g.next()) / width;
        v = ((R)j + g.next()) / height;
    } else {
        u = ((R)i + (R)0.5) / width;
        v = ((R)j + (R)0.5) / height;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (RELOAD && RT_CAM_RELOAD != 0) {
        // sc is the kernel's first argument's first member (the trace kernels take TraceArgs first,
        // pt_trace.hip): its camera words sit at offsetof(SceneView, cam_o) in the kernel-argument
        // segment.  (Taking &sc.cam_o instead makes the argument escape into a private copy.)
        typedef const __attribute__((address_space(4))) R* CamPtr;
        typedef const __attribute__((address_space(4))) char* ArgPtr;
        CamPtr cp = (CamPtr)((ArgPtr)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SceneView<R>, cam_o));
        asm volatile("" : "+s"(cp));
        camera_ray<R, CamPtr, FEAT>(sc, u, v, g, o, d, cp);
        return;
    }
#endif
    camera_ray<R, const R*, FEAT>(sc, u, v, g, o, d, &sc.cam_o[0]);
}

// x^5 for Schlick's approximation (materials.js:79-83, Math.pow(1 - cosine, 5)), correctly rounded —
// the fast path of schlick_reflects.  The reference's own Math.pow (V8 in Node 12, restated exactly in
// js_math.h) is not correctly rounded: it differs from RN(x^5) by 1 ulp in ~9.6 % of arguments
// (tests/test_js_host.py::test_pow5_vs_v8_math_pow).  The path only uses the value in
// `reflectance > Math.random()`, whose draws are multiples of 2^-24; schlick_reflects takes V8's own pow
// wherever the reflectance lies within 2^-40 of the draw, so the decision is V8's.  The device pow
// (ocml, <= 1 ulp) costs ~100 binary64 instructions.  Here x^2, x^4, x^5 are carried
// as unevaluated sums hi + lo (error-free products by FMA): the pair approximates x^5 to ~2^-100
// relative, so the single final rounding gives RN(x^5) unless x^5 lies within 2^-100 of a rounding
// midpoint.  10 binary64 ops; exact for x = 0 and x = 1.  Checked against exact rationals
// (tests/test_hostcheck.py::test_pow5_correctly_rounded) and against Node's own Math.pow(x, 5) on the
// same arguments (tests/test_js_host.py::test_pow5_vs_v8_math_pow, which reports the mismatch rate).
// Only for 0 <= x <= 2 (no overflow/underflow concerns: x is 0 or >= 2^-53).
template <class R>
RT_HD R pow5_rn(R x) {
    const R p = x * x, pe = fma(x, x, -p);                 // x^2 = p + pe exactly
    const R q = p * p, qe = fma(p, p, -q) + (R)2 * (p * pe); // x^4 ~ q + qe
    const R r = q * x, re = fma(q, x, -r) + qe * x;          // x^5 ~ r + re
    return r + re;
}

// V8's Math.pow(x, 5) itself (js_math.h): the rare exact path of schlick_reflects — inlined (config 3
// and Cornell unchanged; out of line, the call's register saves cost Cornell 4.4 %) or, in the lean
// triangle-tree kernel, out of line (inlined cost config 5 0.6 %, out of line nothing)
RT_HD double js_pow5_exact(double x) { return jsm::pow(x, 5.0); }
static RT_COLD_HD double js_pow5_exact_ool(double x) { return jsm::pow(x, 5.0); }

// Dielectric.scatter (materials.js:51-83) by value (RT_COLD_DIEL: out of line, so its registers leave the
// trace kernel's allocation — A/B): the new direction and the RNG's draw count
template <class R> struct DielOut { V3<R> nd; uint32_t k; };
#ifndef RT_COLD_DIEL
#define RT_COLD_DIEL 0
#endif
#if RT_COLD_DIEL && defined(__HIP_DEVICE_COMPILE__)
#define RT_DIEL_HD __host__ __device__ __attribute__((noinline))
#else
#define RT_DIEL_HD RT_HD
#endif
// Schlick's decision `reflectance(cosine, ratio) > Math.random()` (materials.js:64, 79-83) for the draw u.
// In binary64 the reference decides with V8's Math.pow (js_math.h), which lies within 1 ulp of the
// correctly rounded pow5_rn on every argument tested (9.6 % differ).  A difference can move the
// reflectance across the draw only when the two lie within a few ulps; within 2^-40 relative (4096 ulps)
// the reflectance is recomputed with V8's own pow — out of line, taken about once per 10^5 tests — so
// the decision is the reference's bit for bit (tests/test_js_host.py::test_schlick_decisions_are_v8s).
// OOL: the exact path out of line (js_pow5_exact_ool)
template <class R, bool OOL = false>
RT_HD bool schlick_reflects(R r0, R cos_t, R u) {
    R refl = r0 + ((R)1 - r0) * pow5_rn((R)1 - cos_t);
    if constexpr (sizeof(R) == 8)
        if (fabs(refl - u) <= refl * (R)0x1p-40)
            refl = r0 + ((R)1 - r0) * (OOL ? js_pow5_exact_ool((R)1 - cos_t) : js_pow5_exact((R)1 - cos_t));
    return refl > u;
}

template <class R, bool OOL = false>
RT_DIEL_HD DielOut<R> dielectric_scatter(R inv_ior, R ior, R r0f, R r0b, bool front, V3<R> n, V3<R> unit, uint32_t key,
                                         uint32_t k) {
    Rng<R> g{key, k};
    V3<R> nd;
    // 1 / ior and both faces' r0 come precomputed (scene_pack.h, the same roundings): two divisions fewer
    R ratio = front ? inv_ior : ior;
    R cos_t = js_min<R>(dot(unit * (R)-1, n), (R)1);
    R sin_t = sqrt((R)1 - cos_t * cos_t);
    bool reflect_it = ratio * sin_t > (R)1;
    if (!reflect_it) {                                                        // random drawn only if it can refract
        RT_HCOUNT(HC_DIELECTRIC_SCHLICK, 1);
        reflect_it = schlick_reflects<R, OOL>(front ? r0f : r0b, cos_t, g.next());
    }
    if (reflect_it) {
        nd = reflect(unit, n);
    } else {
        R ct = js_min<R>(dot(unit * (R)-1, n), (R)1);
        V3<R> perp = (unit + n * ct) * ratio;
        V3<R> par = n * (-sqrt(fabs((R)1 - dot(perp, perp))));
        nd = perp + par;
    }
    return DielOut<R>{nd, g.k};
}

// Scatter at a non-emissive hit (materials.js:20-83).  Returns false when Metal absorbs.
// The three materials share their common steps so that a wave holding several of them runs each step
// once (a branch runs for the union of its lanes): Lambertian and Metal draw one randomInUnitSphere
// and nothing else (Metal's reflect draws nothing), so that rejection loop runs before the material
// branch (RTOW +3.8 %), and the one normalize each material needs — Lambertian the unit-sphere point
// `p`, Metal and Dielectric the ray direction — arrives as `unit`, computed by shade_segment together
// with the missed rays' (skyGradient's) normalize (+1.6 %).
template <class R, bool OOL = false>
RT_HD bool scatter(const MatRec<R>& m, const Hit<R>& h, V3<R> unit, V3<R> p, Rng<R>& g, V3<R>& nd, V3<R>& att) {
    if (m.type <= 1) {
        att = mk(m.c[0], m.c[1], m.c[2]);
        if (m.type == 0) {                                                    // Lambertian :20-25
            RT_HCOUNT(HC_LAMBERT, 1);
            nd = h.n + unit;
            return true;
        }
        RT_HCOUNT(HC_METAL, 1);
        nd = reflect(unit, h.n) + p * m.p;                                    // Metal :36-41 (roughness)
        return dot(nd, h.n) > (R)0;
    }
    RT_HCOUNT(HC_DIELECTRIC, 1);
#ifdef RT_PROBE_NODIEL                                                        // timing probe only (inexact)
    nd = reflect(unit, h.n);
    att = mk<R>(1, 1, 1);
    return true;
#endif
    // Dielectric :51-83 (ior)
    const DielOut<R> r = dielectric_scatter<R, OOL>(m.c[0], m.p, m.c[1], m.c[2], h.front, h.n, unit, g.key, g.k);
    nd = r.nd;
    g.k = r.k;
    att = mk<R>(1, 1, 1);
    return true;
}

// RT_PROFILE=1 (A/B builds only): shader-clock cycles per lane spent in closest hit, shading and
// sample regeneration, reduced per wave (max) into Counters::totals[4..6]
#ifndef RT_PROFILE
#define RT_PROFILE 0
#endif
#if RT_PROFILE && defined(__HIP_DEVICE_COMPILE__)
#define RT_TICK() ((uint64_t)clock64())
#else
#define RT_TICK() ((uint64_t)0)
#endif

struct PixelResult { uint32_t segments, draws; Work work; uint64_t cyc[3]; };

// Direct lighting at a Lambertian / TexturedLambertian hit (F_LIGHT): for every scene light in scene order,
// light.illuminate(hit.point), the cosine against the stored (face-oriented) normal, a shadow ray from the
// hit point towards the light (occluded: World.hit(ray, 0.001, distance) !== null), and
// direct += (att * color) * cos per channel.  No random draw, no segment: path decisions are untouched.
// `direct` starts at +0 and only adds, so no component is ever -0.
template <class R, int ACC>
RT_HD V3<R> direct_light(const SceneView<R>& sc, const Hit<R>& h, V3<R> att, Work& w, BvhStack stk) {
    const LightView<R>* lv = light_view(sc);
    V3<R> direct = mk<R>(0, 0, 0);
    for (int i = 0; i < lv->num; ++i) {
        const Illum<R> il = illuminate<R>(lv->recs[i], h.p);
        const R cs = dot(h.n, il.dir);
        if (!(cs > (R)0)) continue;                                           // NaN and a zero direction too
        if (occluded<R, ACC>(sc, h.p, il.dir, il.dist, w, stk)) continue;
        direct = direct + mk((att.x * il.col.x) * cs, (att.y * il.col.y) * cs, (att.z * il.col.z) * cs);
    }
    return direct;
}

// Emitter sampling at a Lambertian / TexturedLambertian hit (F_NEE): one emitter drawn
// uniformly from the scene's list, one direction towards it (sample_emitter), the cosine against the facing
// normal, the sampled primitive's own candidate test and a shadow ray up to its t (occluded), weighted against
// the scattered ray's density cs / pi by the balance heuristic:
//   direct = (att (.) Le) * ((cs / pi) / (p_l + p_b)),  p_l = pO / N,  p_b = cs / pi.
// The draws come from a stream of their own, keyed by the sample's key and the bounce: the path's g.k, its
// decisions and its counters are the plain render's.
#ifndef RT_NEE_MUTATION
#define RT_NEE_MUTATION 0         // tests/hostcheck only: 1 = emission weight forced to 1, 2 = hit-side p_l without 1 / N
#endif
template <class R, int ACC>
RT_HD V3<R> emitter_light(const SceneView<R>& sc, const Hit<R>& h, V3<R> att, uint32_t key, int bounce, Work& w, BvhStack stk) {
    const V3<R> none = mk<R>(0, 0, 0);
    const EmitterView<R>* ev = emitter_view(sc);
    const int N = sc.num_emitters;
    if (N <= 0) return none;
    Rng<R> ge{lowbias32(key ^ lowbias32((uint32_t)bounce + 0x4E454531u)), 0};
    const EmitterDraw<R> s = sample_emitter(ev, N, h.p, ge);
    if (!s.ok) return none;
    const R cs = dot(h.n, s.om);
    if (!(cs > (R)0)) return none;
    const EmitterRec<R>& er = ev->recs[s.e];
    R te;
    if (!emitter_candidate(er, h.p, s.om, te)) return none;
    if (occluded<R, ACC>(sc, h.p, s.om, te, w, stk)) return none;
    const R pb = cs / (R)3.141592653589793;
    const R f = pb / (s.pO / (R)N + pb);
    return mk((att.x * er.le[0]) * f, (att.y * er.le[1]) * f, (att.z * er.le[2]) * f);
}

// The density sample_emitter has, per solid angle at o, for the direction d that reached the listed emitter at
// the closest hit c.  false: the primitive is not listed (boxes, planes, degenerate ones), or sampling from o
// skips it (o inside the sphere).
template <class R>
RT_HD bool emitter_hit_pdf(const SceneView<R>& sc, const Closest<R>& c, V3<R> o, V3<R> d, R& pO) {
    const EmitterView<R>* ev = emitter_view(sc);
    if (c.kind == HIT_SPHERE) {
        if (!ev->sphere_listed[c.idx]) return false;
        const SphereRec<R> s = sc.spheres[c.idx];
        const V3<R> w = mk(s.cx, s.cy, s.cz) - o;
        const R D2 = dot(w, w);
        if (!(D2 > s.r2)) return false;
        pO = cone_pdf(sphere_cone_omc(s.r2, D2));
        return true;
    }
    if (c.kind != HIT_TRI) return false;
    const R area = ev->tri_area[c.idx];
    if (!(area > (R)0)) return false;
    const TriRec<R> tr = sc.tris[c.idx];
    const R dd = dot(d, d);
    pO = tri_pdf((c.t * c.t) * dd, fabs(dot(mk(tr.nx, tr.ny, tr.nz), d)) / sqrt(dd), area);
    return true;
}
// The weight of the emission met by a scattered ray (o, d) at the closest hit c, whose direction a Lambertian
// scatter drew with density pb: pb / (pb + pO / N), the balance heuristic against emitter_light; 1 after a camera
// ray, a Metal or a Dielectric scatter (pb = 0; NaN too) and where emitter_hit_pdf has no density.
template <class R>
RT_HD R emission_weight(const SceneView<R>& sc, const Closest<R>& c, V3<R> o, V3<R> d, R pb) {
    if (!(pb > (R)0) || RT_NEE_MUTATION == 1) return (R)1;
    R pO;
    if (!emitter_hit_pdf(sc, c, o, d, pO)) return (R)1;
    return pb / (pb + (RT_NEE_MUTATION == 2 ? pO : pO / (R)sc.num_emitters));
}

// Shade the segment whose closest hit is c (rayColor's body after world.hit, ray-tracer.js:106-122):
// emission / scatter / background.  Returns true when the sample's path ended; its radiance L is
// then in `L`, otherwise (o, d, T, depth) describe the next segment.
// F_LIGHT (the lit kernels; ACC: their walk, for the shadow rays): a scattering Lambertian hit adds
// T (.) direct to lc->dsum, with T the throughput before this hit's attenuation (the forward form of
// emitted + direct + attenuation * rayColor(scattered)).
// LightCtx: what the lit kernels hand to shade_segment — the running sum, the work counters the shadow rays
// count in, and the lane's traversal stack (idle while a segment is shaded).  One pointer, nullptr elsewhere:
// further by-value parameters changed the register allocation of kernels that never use them.
template <class R> struct LightCtx { V3<R> dsum; Work* w; BvhStack stk; };
// F_NEE: the emitter-sampling kernels' context, handed on as its LightCtx — pb, the density of the direction the
// last scatter drew (0: none — a camera ray, Metal, Dielectric), and the render's depth (the bounce index keys
// the emitter draws).  A struct of its own: LightCtx with these two members changed the register allocation of
// the binary32 lane-per-pixel lit kernels (2 and 1 VGPR spills fewer), and every existing kernel stays as it was.
template <class R> struct NeeCtx : LightCtx<R> {
    R pb;
    int max_depth;
    RT_HD NeeCtx(V3<R> d, Work* w, BvhStack s) : LightCtx<R>{d, w, s}, pb((R)0), max_depth(0) {}
};
// the kernels' LightCtx variable: an empty object in the instantiations without F_LIGHT
struct NoLightCtx { template <class... A> RT_HD NoLightCtx(A&&...) {} };
template <class R, bool LIT, bool NEE = false>
using LightState = std::conditional_t<NEE, NeeCtx<R>, std::conditional_t<LIT, LightCtx<R>, NoLightCtx>>;
// RT_COOP_SPHERE (pt_core.h): random_in_unit_sphere for the lanes with `need`, its rejection rounds evaluated by
// every lane of the wave that reaches this call — requester or not: missed rays, Dielectric hits and lanes whose
// point is found help the lanes still looking.  The point and g.k afterwards are the sequential loop's (the first
// accepted round r >= 0 of draws k0+3r .. k0+3r+2, then k = k0 + 3 (r+1)); lanes without `need` get (0, 0, 0) and
// keep their k.  slots: the wave's 64 x {(key, k), result word} in LDS (kCoopSlotBytes each).  After each requester's
// own first round, a trip:
//   1. requester rho (its rank among the lanes that need, by mbcnt: holes in EXEC need no special case) writes
//      (key, k) and kCoopNone at slot rho;
//   2. helper h (its rank among the active lanes) reads slot q's stream, evaluates the round at offset j
//      (coop_assign) and, if that point is accepted, ds_min's coop_pack(j, x, y) into slot q's word;
//   3. the requester reads its word: coop_take.  The z draw is not handed over: the requester repeats it.
// The steps are ordered as pool_item orders its partials: a wave's LDS operations complete in program order, the
// wave-local fence and wave_barrier keep the compiler from moving them.  `while (N)` is wave-uniform, and every
// trip consumes at least one round of every requester, so the loop ends when the slowest sequential loop would.
constexpr int kCoopSlotBytes = 16;
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t coop_rank(uint64_t mask) {       // the active lanes of `mask` below this one
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}
template <class R>
__device__ __forceinline__ V3<R> unit_sphere_point(Rng<R>& g, bool need, unsigned long long* slots) {
    uint32_t ux = 1u << 23, uy = 1u << 23, uz = 1u << 23;             // (0, 0, 0)
    // the first round is the lane's own: half of the requesters end here, and the hand-off costs more than a round
    // (sharing the first trip too measured -0.3 % where this form gains 1.5 %)
    if (need) {
        need = !sphere_round(g.key, g.k, ux, uy, uz);
        g.k += 3;
    }
    uint64_t N = __ballot(need);
    while (N) {
        const uint64_t E = __ballot(true);
        const uint32_t n = (uint32_t)__popcll(N), H = (uint32_t)__popcll(E);
        const uint32_t rho = coop_rank(N);
        const float rn = coop_rcp(n);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (need) {
            slots[2 * rho] = ((unsigned long long)g.k << 32) | g.key;
            slots[2 * rho + 1] = kCoopNone;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const CoopShare a = coop_assign(coop_rank(E), n, rn);
        const unsigned long long stream = slots[2 * a.q];
        uint32_t hx, hy, hz;
        if (sphere_round((uint32_t)stream, (uint32_t)(stream >> 32) + 3 * a.j, hx, hy, hz))
            __hip_atomic_fetch_min(slots + 2 * a.q + 1, coop_pack(a.j, hx, hy), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (need && coop_take(slots[2 * rho + 1], coop_rounds(rho, H, n, rn), g.k, ux, uy)) {
            Rng<R> gz{g.key, g.k - 1};
            uz = gz.next_u24();
            need = false;
        }
        N = __ballot(need);
    }
    return mk((R)((int)ux - (1 << 23)) * (R)0x1p-23, (R)((int)uy - (1 << 23)) * (R)0x1p-23, (R)((int)uz - (1 << 23)) * (R)0x1p-23);
}
#endif
// where the cooperative form is compiled in: binary64 with the lean grid kernel's feature set (pool_item of
// trace_pool_lds_kernel<double, *, ACC_GRID_LDS_LEAN>, and rt_shade_segments' variant 2), on the device
template <class R, int FEAT>
constexpr bool coop_sphere() {
#if RT_COOP_SPHERE && defined(__HIP_DEVICE_COMPILE__)
    return sizeof(R) == 8 && FEAT == feat_of<ACC_GRID_LDS_LEAN>();
#else
    return false;
#endif
}
// coop: unit_sphere_point's LDS slots of this wave (nullptr, and every other instantiation: each lane's own loop)
template <class R, int FEAT = F_ALL, int ACC = ACC_BRUTE>
RT_HD bool shade_segment(const SceneView<R>& sc, const Closest<R>& c, V3<R>& o, V3<R>& d, V3<R>& T, int& depth,
                         Rng<R>& g, V3<R>& L, const MatRec<R>* mats = nullptr, LightCtx<R>* lc = nullptr,
                         unsigned long long* coop = nullptr) {
    bool done = true;
    L = mk<R>(0, 0, 0);
    const bool hit = c.kind != HIT_NONE;
    Hit<R> h{};
    MatRec<R> m{};
    V3<R> p = mk<R>(0, 0, 0);
    const bool shared = coop_sphere<R, FEAT>() && coop != nullptr;
    if (hit) {
        h = hit_record<R, FEAT>(sc, o, d, c);
        m = mats ? mats[h.mat] : sc.mats[h.mat];            // mats: an LDS copy (RT_MAT_LDS A/B)
        if (!shared && m.type <= 1) p = random_in_unit_sphere(g);            // Lambertian / Metal's only draws
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (coop_sphere<R, FEAT>()) {
        // ... drawn by the wave together: every lane here takes part (MatRec m{} has type 0 on a miss)
        if (shared) p = unit_sphere_point(g, hit && m.type <= 1, coop);
    }
#endif
    // one normalize for every lane (see scatter): Lambertian's p, else the ray direction (Metal,
    // Dielectric, and a missed ray's skyGradient)
    const V3<R> unit = normalize(hit && m.type == 0 ? p : d);
    if (hit) {
        if (m.type == 3) {                                                    // Emissive (materials.js:87-96)
            RT_HCOUNT(HC_EMISSIVE, 1);
            L = mk(T.x * m.c[0], T.y * m.c[1], T.z * m.c[2]);                 // emission
            if constexpr ((FEAT & F_NEE) != 0) {                              // ... MIS-weighted against emitter sampling
                const R wgt = emission_weight<R>(sc, c, o, d, static_cast<NeeCtx<R>*>(lc)->pb);
                if (wgt != (R)1) L = L * wgt;
            }
        } else {
            V3<R> nd, att;
            if (scatter<R, (FEAT & F_TRIS) != 0 && (FEAT & F_ALL) != F_ALL>(m, h, unit, p, g, nd, att)) {
                // TexturedLambertian / TexturedMetal (materials.js:99-126) draw what their plain forms draw;
                // only the attenuation differs: texture.value(u, v, rec.point).  (An absorbing TexturedMetal
                // skips the texture: it has no draws and no side effects.)
                if constexpr ((FEAT & F_TEX) != 0) {
                    if (m.type <= 1) {
                        const TexView<R>* tv = tex_view(sc);
                        const int tex = tv->mat_tex[h.mat];
                        if (tex >= 0) att = texture_value<R>(tv, tex, h.p);
                    }
                }
                if constexpr ((FEAT & F_LIGHT) != 0) {
                    if (m.type == 0) {
                        const V3<R> dl = direct_light<R, ACC>(sc, h, att, *lc->w, lc->stk);
                        lc->dsum = lc->dsum + mk(T.x * dl.x, T.y * dl.y, T.z * dl.z);
                    }
                }
                if constexpr ((FEAT & F_NEE) != 0) {
                    NeeCtx<R>* nc = static_cast<NeeCtx<R>*>(lc);
                    nc->pb = (R)0;
                    if (m.type == 0) {
                        // not at the last allowed bounce: its successor segment does not exist in the plain render
                        if (depth > 1) {
                            const V3<R> el = emitter_light<R, ACC>(sc, h, att, g.key, nc->max_depth - depth, *nc->w, nc->stk);
                            nc->dsum = nc->dsum + mk(T.x * el.x, T.y * el.y, T.z * el.z);
                        }
                        nc->pb = dot(h.n, nd) / (sqrt(dot(nd, nd)) * (R)3.141592653589793);
                    }
                }
                T = mk(T.x * att.x, T.y * att.y, T.z * att.z);
                o = h.p;
                d = nd;
                done = --depth <= 0;                                          // rayColor(.., 0) returns 0
            }
        }
    } else {
        RT_HCOUNT(HC_MISS, 1);
        const V3<R> bg = background<R, FEAT>(sc, d, unit);                    // world.background(ray)
        L = mk(T.x * bg.x, T.y * bg.y, T.z * bg.z);
    }
    return done;
}

// Trace samples [im.s_begin, s_end) of crop pixel (cx, cy), adding radiance into sum[0..2].
// In binary64 with maxBounces <= RT_REC_DEPTH, a sample's radiance is evaluated in the order of the
// reference's recursion (ray-tracer.js:102-121: emitted + attenuation * rayColor(scattered)): the
// attenuations are kept and multiplied onto the path's end value from the last bounce back, a0 * (a1 *
// (... * X)), where the sample pool carries the throughput forward, ((a0 * a1) * ...) * X.  emitted is
// zero for every material that scatters (an Emissive hit ends the path), so this is the recursion's
// value bit for bit; with the samples added in sample order (this function) the means are the
// reference's.  Deeper renders carry the throughput forward.
// Lit modes (F_LIGHT) keep one direct term per scattering bounce beside att[] — the last allowed bounce's
// too, whose recursive call returns 0 — and fold direct_k + att_k * (...) from the last bounce back: emitted
// is +0 there and direct is never -0, so (e + direct) + att * rec is that sum bit for bit.
#ifndef RT_REC_DEPTH
#define RT_REC_DEPTH 16
#endif
// trace_pixel for the lit modes (F_LIGHT): the same loop with the direct terms.  A twin, not `if constexpr`
// branches inside trace_pixel: the folded form (discarded branches, a one-element dir[], an empty LightState)
// is the same program for the unlit modes, yet it changed the register allocation of 21 existing
// lane-per-pixel trace_kernel instantiations — trace_kernel<float, *, ACC_BVH> from no scratch to 32-48 B
// and 7-10 spilled VGPRs, trace_kernel<double, false, ACC_BRUTE> from 592 to 608 B (compiler resource
// remarks, DESIGN.md §4 "Direct lighting") — and the feature must leave every existing kernel as it was.
template <class R, bool COUNT, int ACC>
RT_HD PixelResult trace_pixel_lit(const SceneView<R>& sc, const ImageParams& im, int cx, int cy, int s_end, double* sum,
                                  BvhStack stk) {
    const int i = im.x0 + cx, row = im.y0 + cy, j = im.height - 1 - row;
    const uint32_t pkey = pixel_key(im.seedm, (uint32_t)row * (uint32_t)im.width + (uint32_t)i);
    PixelResult res{0, 0, {0, 0, 0}, {0, 0, 0}};
    int s = im.s_begin;
    double sx = sum[0], sy = sum[1], sz = sum[2];
    Rng<R> g;
    V3<R> o, d, T = mk<R>(1, 1, 1);
    int depth = im.max_depth;
    const bool rec = sizeof(R) == 8 && im.max_depth <= RT_REC_DEPTH;
    V3<R> att[RT_REC_DEPTH];                   // rec: the sample's attenuations, bounce by bounce
    static_assert((feat_of<ACC>() & F_LIGHT) != 0, "a lit mode");
    V3<R> dir[RT_REC_DEPTH];                   // rec: the bounces' direct terms
    // dsum: the segment's (rec) or the sample's (forward) direct light
    constexpr bool NEE = (feat_of<ACC>() & F_NEE) != 0;     // emitter sampling: pb = 0 at every sample start
    LightState<R, true, NEE> lc{mk<R>(0, 0, 0), &res.work, stk};
    if constexpr (NEE) lc.max_depth = im.max_depth;
    int nb = 0;
    bool skip_tri = false;                     // tri_exit_bound (pt_core.h)
    if (s < s_end) start_sample(sc, im, i, j, pkey, s, g, o, d);
    while (s < s_end) {
        const uint64_t t0 = RT_TICK();
        const Closest<R> c = closest_hit_acc<R, ACC>(sc, o, d, res.work, stk, skip_tri);
        const uint64_t t1 = RT_TICK();
        if (RT_PROFILE) res.cyc[0] += t1 - t0;
        ++res.segments;
        V3<R> L;
        if (rec) T = mk<R>(1, 1, 1);           // then T = 1 * attenuation and L = 1 * X: exact
        const int depth0 = depth;
        if (rec) lc.dsum = mk<R>(0, 0, 0);
        const bool done = shade_segment<R, feat_of<ACC>(), ACC>(sc, c, o, d, T, depth, g, L, nullptr, &lc);
        if (rec && done && depth != depth0) {       // the last allowed bounce scattered: direct + att * 0
            att[nb] = T;
            dir[nb++] = lc.dsum;
        }
        if (rec && !done) dir[nb] = lc.dsum;
        if constexpr (sizeof(R) == 8 && (walk_of<ACC>() == ACC_BVH || walk_of<ACC>() == ACC_BVH_STACK || ACC == ACC_BVH_STACK_LEAN))
            skip_tri = !done && c.kind == HIT_TRI && leaves_tri_hull(sc, c.idx, o, d);
        const uint64_t t2 = RT_TICK();
        if (RT_PROFILE) res.cyc[1] += t2 - t1;
        if (rec && !done) att[nb++] = T;
        if (done) {
            if (rec) {
                for (int k = nb - 1; k >= 0; --k)
                    L = mk(dir[k].x + att[k].x * L.x, dir[k].y + att[k].y * L.y, dir[k].z + att[k].z * L.z);
                nb = 0;
            } else {
                L = L + lc.dsum;
                lc.dsum = mk<R>(0, 0, 0);
            }
            sx += (double)L.x; sy += (double)L.y; sz += (double)L.z;
            if (COUNT) res.draws += g.k;
            ++s;
            T = mk<R>(1, 1, 1);
            depth = im.max_depth;
            if constexpr (NEE) lc.pb = (R)0;
            if (s < s_end) start_sample(sc, im, i, j, pkey, s, g, o, d);
        }
        if (RT_PROFILE) res.cyc[2] += RT_TICK() - t2;
    }
    sum[0] = sx; sum[1] = sy; sum[2] = sz;
    return res;
}

template <class R, bool COUNT, int ACC = ACC_BRUTE>
RT_HD PixelResult trace_pixel(const SceneView<R>& sc, const ImageParams& im, int cx, int cy, int s_end, double* sum,
                              BvhStack stk = BvhStack{nullptr, 0}) {
    // the lit modes: the twin above (this function's text is kept as it was, so that the kernels without
    // F_LIGHT compile to what they were)
    if constexpr ((feat_of<ACC>() & F_LIGHT) != 0) return trace_pixel_lit<R, COUNT, ACC>(sc, im, cx, cy, s_end, sum, stk);
    else {
    const int i = im.x0 + cx, row = im.y0 + cy, j = im.height - 1 - row;
    const uint32_t pkey = pixel_key(im.seedm, (uint32_t)row * (uint32_t)im.width + (uint32_t)i);
    PixelResult res{0, 0, {0, 0, 0}, {0, 0, 0}};
    int s = im.s_begin;
    double sx = sum[0], sy = sum[1], sz = sum[2];
    Rng<R> g;
    V3<R> o, d, T = mk<R>(1, 1, 1);
    int depth = im.max_depth;
    const bool rec = sizeof(R) == 8 && im.max_depth <= RT_REC_DEPTH;
    V3<R> att[RT_REC_DEPTH];                   // rec: the sample's attenuations, bounce by bounce
    int nb = 0;
    bool skip_tri = false;                     // tri_exit_bound (pt_core.h)
    if (s < s_end) start_sample(sc, im, i, j, pkey, s, g, o, d);
    while (s < s_end) {
        const uint64_t t0 = RT_TICK();
        const Closest<R> c = closest_hit_acc<R, ACC>(sc, o, d, res.work, stk, skip_tri);
        const uint64_t t1 = RT_TICK();
        if (RT_PROFILE) res.cyc[0] += t1 - t0;
        ++res.segments;
        V3<R> L;
        if (rec) T = mk<R>(1, 1, 1);           // then T = 1 * attenuation and L = 1 * X: exact
        const bool done = shade_segment<R, F_ALL | (feat_of<ACC>() & F_TEX)>(sc, c, o, d, T, depth, g, L);
        if constexpr (sizeof(R) == 8 && (walk_of<ACC>() == ACC_BVH || walk_of<ACC>() == ACC_BVH_STACK || ACC == ACC_BVH_STACK_LEAN))
            skip_tri = !done && c.kind == HIT_TRI && leaves_tri_hull(sc, c.idx, o, d);
        const uint64_t t2 = RT_TICK();
        if (RT_PROFILE) res.cyc[1] += t2 - t1;
        if (rec && !done) att[nb++] = T;
        if (done) {
            if (rec) {
                for (int k = nb - 1; k >= 0; --k) L = mk(att[k].x * L.x, att[k].y * L.y, att[k].z * L.z);
                nb = 0;
            }
            sx += (double)L.x; sy += (double)L.y; sz += (double)L.z;
            if (COUNT) res.draws += g.k;
            ++s;
            T = mk<R>(1, 1, 1);
            depth = im.max_depth;
            if (s < s_end) start_sample(sc, im, i, j, pkey, s, g, o, d);
        }
        if (RT_PROFILE) res.cyc[2] += RT_TICK() - t2;
    }
    sum[0] = sx; sum[1] = sy; sum[2] = sz;
    return res;
    }
}

// ---- feature buffers (AOVs) of the primary hit: the guides of the guided filter (pt_guided.h) ----
// One ray through the centre of pixel (i, j) (j bottom-up; the RT_AA_CENTER formula) from a pinhole — camera_ray
// with the lens offset exactly zero, so no random number is drawn: perspective o = cam_o, d = ((llc + hor u) +
// ver v) - o, not normalized; orthographic as camera_ray normalizes it.  The closest hit is the trace kernels'
// own query and record.  g[0..2] albedo: the Lambertian / Metal albedo (a textured material: texture_value at
// the hit point; binary32: aov_texture_value's pinned sine), (1, 1, 1) for a Dielectric, min(emission, 1) per channel for an Emissive; g[3..5] the record's
// normal (facing the ray); g[6] = t |d| in R; g[7] = 0.  A miss: zeros and depth +inf.  Everything is computed
// in R and stored as binary32.
struct AovHit { int kind, idx; };
// Texture.value for the albedo buffer.  Binary64: texture_value itself (pt_core.h), the trace kernels' function.
// Binary32: the same operations with one difference — texture_value<float> takes the platform's sinf (the
// binary32 fast mode keeps the device's own, pt_core.h js_sin), which differs in the last bit between the
// device's library and a host's C library; a feature buffer is an output, so here the sine is V8's binary64
// Math.sin (js_math.h: plain binary64 arithmetic, the same bits everywhere) of the widened argument, rounded to
// binary32.  The buffer is then the same bits on the GPU and in the CPU build, and within an ulp or two of
// the value the binary32 trace kernels attenuate with.  (|argument| > 2^19 pi/2: jsm::sin falls back to the
// platform's function, not bit-pinned; no scene here gets near it.)
RT_HD float aov_sin(float x) { return (float)jsm::sin((double)x); }
template <class R>
__host__ __device__ RT_COLD V3<R> aov_texture_value(const TexView<R>* tv, int tex, V3<R> p) {
    if constexpr (sizeof(R) == 8) return texture_value<R>(tv, tex, p);
    else {
        const TexRec<R> t = tv->recs[tex];
        const R s = t.scale;
        if (t.type == TEX_CHECKER) {                                                  // textures.js:32-35
            const R sines = (aov_sin(s * p.x) * aov_sin(s * p.y)) * aov_sin(s * p.z);
            return sines < (R)0 ? mk(t.odd[0], t.odd[1], t.odd[2]) : mk(t.even[0], t.even[1], t.even[2]);
        }
        if (t.type == TEX_NOISE) return texture_value<R>(tv, tex, p);                 // no sine
        const int* perm = tv->perms + 512 * t.perm;
        if (t.type == TEX_MARBLE) {                                                   // :60-64
            const R n = turbulence<R>(perm, p * s, 7);
            const R m = (R)0.5 * ((R)1 + aov_sin(s * p.z + (R)10 * n)), w = (R)1 - m;
            return mk<R>((R)0.9 * m + (R)0.6 * w, (R)0.8 * m + (R)0.4 * w, (R)0.7 * m + (R)0.3 * w);
        }
        const R k = s * (R)20;                                                        // wood :75-80
        const R grain = perlin<R>(perm, p.x * k, p.y * k, p.z * k);
        const R rings = aov_sin(s * sqrt(p.x * p.x + p.z * p.z) + grain * (R)10);
        const R m = (R)0.5 * ((R)1 + rings), w = (R)1 - m;
        return mk<R>((R)0.8 * m + (R)0.4 * w, (R)0.5 * m + (R)0.2 * w, (R)0.2 * m + (R)0.1 * w);
    }
}
template <class R, int ACC>
RT_HD AovHit aov_pixel(const SceneView<R>& sc, int width, int height, int i, int j, BvhStack stk, float* g) {
    const R u = ((R)i + (R)0.5) / (R)width, v = ((R)j + (R)0.5) / (R)height;
    const V3<R> o = mk<R>(sc.cam_o[0], sc.cam_o[1], sc.cam_o[2]);
    const V3<R> llc = mk<R>(sc.cam_llc[0], sc.cam_llc[1], sc.cam_llc[2]);
    const V3<R> hor = mk<R>(sc.cam_h[0], sc.cam_h[1], sc.cam_h[2]), ver = mk<R>(sc.cam_v[0], sc.cam_v[1], sc.cam_v[2]);
    V3<R> d = ((llc + hor * u) + ver * v) - o;
    if (sc.cam_ortho) d = normalize(d + mk<R>(sc.cam_w[0], sc.cam_w[1], sc.cam_w[2]) * (R)-1);
    Work w{0, 0, 0, 0, 0, 0};
    const Closest<R> c = closest_hit_acc<R, ACC>(sc, o, d, w, stk);
    for (int k = 0; k < 8; ++k) g[k] = 0.0f;
    if (c.kind == HIT_NONE) {
        g[6] = INFINITY;
        return AovHit{HIT_NONE, -1};
    }
    const Hit<R> h = hit_record<R>(sc, o, d, c);
    const MatRec<R> m = sc.mats[h.mat];
    V3<R> alb = mk<R>(1, 1, 1);                                               // Dielectric
    if (m.type <= 1) {
        alb = mk(m.c[0], m.c[1], m.c[2]);
        if (sc.num_tex > 0) {
            const TexView<R>* tv = tex_view(sc);
            const int tex = tv->mat_tex[h.mat];
            if (tex >= 0) alb = aov_texture_value<R>(tv, tex, h.p);
        }
    } else if (m.type == 3) {
        alb = mk(m.c[0] > (R)1 ? (R)1 : m.c[0], m.c[1] > (R)1 ? (R)1 : m.c[1], m.c[2] > (R)1 ? (R)1 : m.c[2]);
    }
    g[0] = (float)alb.x; g[1] = (float)alb.y; g[2] = (float)alb.z;
    g[3] = (float)h.n.x; g[4] = (float)h.n.y; g[5] = (float)h.n.z;
    g[6] = (float)(c.t * sqrt(dot(d, d)));
    return AovHit{c.kind, c.idx};
}

}  // namespace rt
