// rt_capi.cpp — extern "C" ABI of librt_hip.so (include/rt_hip.h).
//
// Replaces RayTracer.render (js/ray-tracer.js:166-281): the host hands over the packed World /
// Camera once (rt_scene_create uploads it to HBM), then each render traces sample batches on the
// GPU, runs the epilogue on the GPU and copies back only the per-pixel outputs.
// There is no CPU fallback anywhere in this library: without a HIP device every call fails with
// RT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_hip.h"
#include "pt_launch.h"
#include "pt_guided.h"
#include "pt_vguided.h"
#include "pt_error.h"
#include "pool_order.h"
#include "render_plan.h"
#include "scene_pack.h"

using namespace rt;

namespace {

thread_local std::string g_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

}  // namespace

namespace rt {
int set_error(int code, const char* msg) {   // for the other translation units (scene_json.cpp)
    g_error = msg;
    return code;
}
}  // namespace rt

namespace {

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = std::max<size_t>(count, 1);
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

template <class T>
hipError_t upload(DevBuf<T>& b, const std::vector<T>& v) {
    hipError_t e = b.ensure(v.size());
    if (e != hipSuccess) return e;
    if (!v.empty()) e = hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// Scene arrays of one precision, resident in HBM.
template <class R>
struct DeviceScene {
    DevBuf<Run> runs;
    DevBuf<SphereRec<R>> spheres;
    DevBuf<SphereFilter> sphere_filter;
    DevBuf<R> sphere_r, sphere_inv_r;
    DevBuf<PlaneRec<R>> planes;
    DevBuf<BoxRec<R>> boxes;
    DevBuf<TriRec<R>> tris;
    DevBuf<int> sphere_mat, plane_mat, box_mat, tri_mat, perm;
    DevBuf<MatRec<R>> mats;
    DevBuf<int> plane_obj, box_obj;
    DevBuf<BvhNode> sphere_nodes, tri_nodes;
    DevBuf<SphereLeaf<R>> bvh_sphere_leaf;
    DevBuf<TriLeaf<R>> bvh_tri_leaf;
    DevBuf<TriFilter> tri_filter;
    DevBuf<double> tri_exit;
    DevBuf<SphereLeaf<R>> big_sphere_leaf;
    DevBuf<Bvh2Node> sphere_wide, tri_wide;
    DevBuf<int> grid_cell;
    DevBuf<SphereLeaf<R>> grid_leaf;
    // procedural textures (scene_textured only): records, tables, texture per material; the TexView over
    // them is uploaded behind the world's table in `perm` (pt_core.h tex_view)
    DevBuf<TexRec<R>> tex_recs;
    DevBuf<int> tex_perms, mat_tex;
    DevBuf<LightRec<R>> light_recs;      // scene lights (lit scenes only): the LightView follows the TexView
    DevBuf<EmitterRec<R>> emitter_recs;  // emitter sampling: the EmitterView follows the LightView
    DevBuf<int> sphere_listed;
    DevBuf<R> tri_area;
    SceneView<R> view{};
    void release() {
        runs.release(); spheres.release(); sphere_filter.release(); sphere_r.release(); sphere_inv_r.release(); planes.release(); boxes.release(); tris.release();
        sphere_mat.release(); plane_mat.release(); box_mat.release(); tri_mat.release(); perm.release(); mats.release();
        plane_obj.release(); box_obj.release(); sphere_nodes.release(); tri_nodes.release(); bvh_sphere_leaf.release();
        bvh_tri_leaf.release(); tri_filter.release(); tri_exit.release(); big_sphere_leaf.release();
        sphere_wide.release(); tri_wide.release(); grid_cell.release(); grid_leaf.release();
        tex_recs.release(); tex_perms.release(); mat_tex.release(); light_recs.release();
        emitter_recs.release(); sphere_listed.release(); tri_area.release();
    }
};

template <class R>
int build_device(DeviceScene<R>& ds, const HostScene& hs, const rt_scene_desc& d) {
    HostRecords<R> rec;
    make_records(hs, d, rec);
    hipError_t e = hipSuccess;
#define UP(buf, vec) if (e == hipSuccess) e = upload(ds.buf, vec)
    UP(runs, hs.runs); UP(spheres, rec.spheres); UP(sphere_filter, rec.sphere_filter); UP(sphere_r, rec.sphere_r); UP(sphere_inv_r, rec.sphere_inv_r); UP(planes, rec.planes);
    UP(boxes, rec.boxes); UP(tris, rec.tris); UP(sphere_mat, hs.sphere_mat); UP(plane_mat, hs.plane_mat);
    UP(box_mat, hs.box_mat); UP(tri_mat, hs.tri_mat); UP(mats, rec.mats);
    const bool textured = !rec.tex_recs.empty(), lit = !rec.light_recs.empty(), nee = !rec.emitter_recs.empty();
    if (textured || lit || nee) {   // the TexView over the uploaded arrays goes behind the world's table (tex_view)
        UP(tex_recs, rec.tex_recs); UP(tex_perms, rec.tex_perms); UP(mat_tex, rec.mat_tex);
        rec.set_tex_view(TexView<R>{ds.tex_recs.p, ds.tex_perms.p, ds.mat_tex.p, (int)rec.tex_recs.size(),
                                    (int)(rec.tex_perms.size() / 512)});
    }
    if (lit) {               // ... and the LightView behind it (light_view)
        UP(light_recs, rec.light_recs);
        rec.set_light_view(LightView<R>{ds.light_recs.p, (int)rec.light_recs.size(), 0});
    }
    if (nee) {               // ... and the EmitterView behind that (emitter_view)
        UP(emitter_recs, rec.emitter_recs); UP(sphere_listed, rec.sphere_listed); UP(tri_area, rec.tri_area);
        rec.set_emitter_view(EmitterView<R>{ds.emitter_recs.p, ds.sphere_listed.p, ds.tri_area.p,
                                            (int)rec.emitter_recs.size(), 0});
    }
    UP(perm, rec.perm);
    UP(plane_obj, hs.plane_obj); UP(box_obj, hs.box_obj); UP(sphere_nodes, hs.sphere_bvh); UP(tri_nodes, hs.tri_bvh);
    UP(bvh_sphere_leaf, rec.bvh_sphere_leaf); UP(bvh_tri_leaf, rec.bvh_tri_leaf); UP(tri_filter, rec.tri_filter); UP(big_sphere_leaf, rec.big_sphere_leaf); UP(sphere_wide, hs.sphere_wide); UP(tri_wide, hs.tri_wide);
    UP(grid_cell, hs.grid_cell); UP(grid_leaf, rec.grid_leaf); UP(tri_exit, hs.tri_exit);
#undef UP
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "scene upload: %s", hipGetErrorString(e));
    SceneView<R>& v = ds.view;
    v.runs = ds.runs.p;
    v.spheres = ds.spheres.p; v.sphere_filter = ds.sphere_filter.p; v.sphere_r = ds.sphere_r.p; v.sphere_inv_r = ds.sphere_inv_r.p; v.planes = ds.planes.p; v.boxes = ds.boxes.p;
    v.tris = ds.tris.p; v.sphere_mat = ds.sphere_mat.p; v.plane_mat = ds.plane_mat.p; v.box_mat = ds.box_mat.p;
    v.tri_mat = ds.tri_mat.p; v.mats = ds.mats.p; v.perm = ds.perm.p;
    v.plane_obj = ds.plane_obj.p; v.box_obj = ds.box_obj.p; v.sphere_nodes = ds.sphere_nodes.p; v.tri_nodes = ds.tri_nodes.p;
    v.bvh_sphere_leaf = ds.bvh_sphere_leaf.p; v.bvh_tri_leaf = ds.bvh_tri_leaf.p; v.tri_filter = ds.tri_filter.p;
    v.tri_exit = ds.tri_exit.p;
    v.big_spheres = ds.big_sphere_leaf.p;
    v.sphere_wide = ds.sphere_wide.p; v.tri_wide = ds.tri_wide.p;
    v.grid_cell = ds.grid_cell.p; v.grid_leaf = ds.grid_leaf.p;
    fill_view_constants(v, hs, d);
    return RT_OK;
}

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// The render's control words (rt_scene::ctl, mapped coherent host memory, read and written by the host
// and by the kernels of every device): the cancel word, the sticky stop word and the samples the sums
// hold (ReduceGate), and one `aborted` word per batch slot of the ring.
// kCtlCancel: kCancelCopies copies of the cancel word, one per 128-B line (pt_launch.h).
constexpr int kCtlStop = 1, kCtlDone = 2, kCtlAborted = 4;
constexpr int kCtlCancel = 128;
// fused batches (render_impl): per batch, the flag its last item raises; two `aborted` words (the gates'
// stand-in, never written; the skipping waves', never read)
constexpr int kCtlFlag = kCtlCancel + kCancelCopies * kCancelStride;
constexpr int kCtlFusedAborted = kCtlFlag + kMaxFused;
// the error estimate (pt_error.h): the sticky `converged` word of the threshold stop, and one ErrorWords per
// batch in flight (slot kb % ring, like the `aborted` words), 8-byte aligned
constexpr int kCtlConverged = kCtlFusedAborted + 2;
constexpr int kCtlErr = (kCtlConverged + 1 + 31) & ~31;
constexpr int kErrSlots = kSlots * RT_MAX_DEVICES + kSlots;
constexpr int kErrSlotWords = (int)(sizeof(ErrorWords) / sizeof(uint32_t));
static_assert(sizeof(ErrorWords) % sizeof(uint32_t) == 0 && kErrSlotWords % 2 == 0, "ErrorWords slots stay 8-byte aligned");
constexpr int kCtlWords = kCtlErr + kErrSlots * kErrSlotWords;
static_assert(kCtlAborted + kSlots * RT_MAX_DEVICES + kSlots <= kCtlCancel, "one aborted word per ring slot");
inline uint32_t ctl_load(const uint32_t* ctl, int k) { return __atomic_load_n(ctl + k, __ATOMIC_SEQ_CST); }
inline void ctl_store(uint32_t* ctl, int k, uint32_t v) { __atomic_store_n(ctl + k, v, __ATOMIC_SEQ_CST); }
inline void ctl_cancel(uint32_t* ctl, uint32_t v) {
    for (int k = 0; k < kCancelCopies; ++k) ctl_store(ctl, kCtlCancel + k * kCancelStride, v);
}

// Everything one device holds for a scene: the scene arrays in its HBM, a stream, the running sums
// and counters of the samples it traces, the pool's chunk partials and the work totals (scratch).
struct DeviceState {
    int device = 0;
    DeviceScene<double> s64;
    DeviceScene<float> s32;
    hipStream_t stream = nullptr;      // accumulation stream: zeroing, reduces, merges, epilogue
    hipEvent_t ev[2] = {};             // trace timing
    DevBuf<double> sum;
    DevBuf<uint32_t> segs, draws;
    DevBuf<unsigned long long> total;
    DevBuf<double> part;               // sample-pool chunk partials (ensure_partials; overlapped batches: slot 0)
    DevBuf<uint32_t> gate_skip;        // ReduceGate::skip of the reduces on this device's stream
    hipEvent_t scratch_ev = nullptr;   // recorded after every use of part / total (order_scratch)
    hipStream_t scratch_stream = nullptr;
    bool scratch_used = false;
    hipEvent_t copy_ev = nullptr;      // a replica's batch sums copied out to the home device (merge_shards)
    // overlapped batches (render_impl): batch k traces on tstream[k % kSlots] into its own partials
    // (slot 0: `part`), so the next batches' waves fill the CUs while this one drains; its reduce runs on
    // `stream` in batch order
    hipStream_t tstream[kSlots] = {};
    DevBuf<double> part_more[kSlots - 1];   // partials of slots 1 ..
    hipEvent_t traced[kSlots] = {}, reduced[kSlots] = {}, setup_ev = nullptr;
    DevBuf<double>& slot_part(int j) { return j == 0 ? part : part_more[j - 1]; }
    // fused batches (render_impl): every batch's chunk partials, the items done per batch, and the
    // event recorded after the one launch on tstream[0]
    DevBuf<double> fused_part;
    DevBuf<uint32_t> fused_count;
    hipEvent_t fused_done = nullptr;
    // the one-wave pool kernel's cancel word in device memory (Counters::cancel_dev), zeroed once; each
    // render matches its own generation
    DevBuf<uint32_t> cancel_word;

    int init(int dev, const HostScene& hs, const rt_scene_desc& d) {
        device = dev;
        hipError_t e = hipSetDevice(dev);
        if (e != hipSuccess) return fail(RT_ERR_DEVICE, "hipSetDevice(%d): %s", dev, hipGetErrorString(e));
        int rc;
        if ((rc = build_device(s64, hs, d)) || (rc = build_device(s32, hs, d))) return rc;
        // the accumulation stream at the device's highest priority: a batch's reduce (and preview frame)
        // would otherwise wait for free wave slots behind the next batch's trace waves — measured: a
        // 0.1-ms reduce took 7.8 ms, and the batch after next started late
        int least = 0, greatest = 0;
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, greatest);
        for (int k = 0; k < kSlots && e == hipSuccess; ++k) e = hipStreamCreateWithFlags(&tstream[k], hipStreamNonBlocking);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
        for (int k = 0; k < kSlots && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&traced[k], hipEventDisableTiming);
        for (int k = 0; k < kSlots && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&reduced[k], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&setup_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&fused_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&scratch_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&copy_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = cancel_word.ensure((size_t)kDevCancelCopies * kCancelStride);
        if (e == hipSuccess) e = hipMemset(cancel_word.p, 0, (size_t)kDevCancelCopies * kCancelStride * sizeof(uint32_t));
        if (e != hipSuccess) return fail(RT_ERR_DEVICE, "stream/event create: %s", hipGetErrorString(e));
        return RT_OK;
    }
    void sync_all() {                  // every stream of this device (error paths, release)
        (void)hipSetDevice(device);
        for (hipStream_t s : tstream)
            if (s) (void)hipStreamSynchronize(s);
        if (stream) (void)hipStreamSynchronize(stream);
    }
    void release() {
        sync_all();
        s64.release();
        s32.release();
        sum.release(); segs.release(); draws.release(); total.release(); part.release(); gate_skip.release();
        fused_part.release(); fused_count.release(); cancel_word.release();
        for (DevBuf<double>& b : part_more) b.release();
        for (hipEvent_t e : {ev[0], ev[1], setup_ev, scratch_ev, copy_ev, fused_done})
            if (e) (void)hipEventDestroy(e);
        for (int k = 0; k < kSlots; ++k) {
            if (traced[k]) (void)hipEventDestroy(traced[k]);
            if (reduced[k]) (void)hipEventDestroy(reduced[k]);
            if (tstream[k]) (void)hipStreamDestroy(tstream[k]);
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// A deep copy of the scene descriptor, so replicas can be uploaded to more devices later.
struct DescCopy {
    rt_scene_desc d{};
    std::vector<rt_object_desc> objects;
    std::vector<rt_material_desc> materials;
    std::vector<double> triangles;
    std::vector<rt_texture_desc> textures;
    std::vector<int32_t> material_texture, texture_perms;
    std::vector<rt_light_desc> lights;
    void set(const rt_scene_desc& src) {
        d = src;
        lights.assign(src.lights, src.lights + std::max(0, src.num_lights));
        d.lights = lights.data();
        textures.assign(src.textures, src.textures + std::max(0, src.num_textures));
        if (src.material_texture) material_texture.assign(src.material_texture, src.material_texture + std::max(0, src.num_materials));
        texture_perms.assign(src.texture_perms, src.texture_perms + 512 * (size_t)std::max(0, src.num_texture_perms));
        d.textures = textures.data();
        d.material_texture = src.material_texture ? material_texture.data() : nullptr;
        d.texture_perms = texture_perms.data();
        objects.assign(src.objects, src.objects + std::max(0, src.num_objects));
        materials.assign(src.materials, src.materials + std::max(0, src.num_materials));
        triangles.assign(src.triangles, src.triangles + 12 * (size_t)std::max(0, src.num_triangles));
        d.objects = objects.data();
        d.materials = materials.data();
        d.triangles = triangles.data();
    }
};

}  // namespace

// The RGBA8 threshold table of one gamma (launch_gamma_thresholds) on the scene's device.  A table is
// built once and then only read: an asynchronous epilogue on any stream reads its own gamma's table, so
// a later call with another gamma can never overwrite the bytes an earlier one is still reading (ADVICE
// r5).  `used` is recorded after every kernel that reads the table; a slot is rebuilt for another gamma
// (the least recently used one, when kGammaSlots gammas are in use) only after it has completed.
struct GammaSlot {
    DevBuf<unsigned char> buf;
    double gamma = NAN;
    bool ok = false;                 // no exception overflow: the table may be used
    hipEvent_t used = nullptr;
    bool used_recorded = false;
    uint64_t tick = 0;               // last use (LRU)
    const GammaTable* table() const { return reinterpret_cast<const GammaTable*>(buf.p); }
    void release() {
        buf.release();
        if (used) (void)hipEventDestroy(used);
        used = nullptr;
    }
};
constexpr int kGammaSlots = 8;

// What a resident checkpoint's sums are sums of: a resume from the sums left on the device
// (rt_render_resume with sums NULL) must name the same frame, crop window, first sample, precision, seed,
// anti-aliasing mode and depth, not only the same pixel count.
struct CkptKey {
    int32_t width, height, x0, y0, cw, ch, sample_begin, precision, aa_mode, max_depth;
    uint64_t seed;
    bool operator==(const CkptKey& o) const {
        return width == o.width && height == o.height && x0 == o.x0 && y0 == o.y0 && cw == o.cw && ch == o.ch &&
               sample_begin == o.sample_begin && precision == o.precision && aa_mode == o.aa_mode &&
               max_depth == o.max_depth && seed == o.seed;
    }
};
inline CkptKey ckpt_key(const rt_settings* s, int cw, int ch) {
    return CkptKey{s->width, s->height, s->crop_x0, s->crop_y0, cw, ch, std::max(0, s->sample_begin), s->precision,
                   s->aa_mode, s->max_depth, (uint64_t)s->seed};
}

// A shard's staging buffers on the home device and the events that free them (merge_shards,
// trace_replica).
struct MergeSlot {
    DevBuf<double> sum;
    DevBuf<uint32_t> segs, draws;
    hipEvent_t added = nullptr;     // recorded on the home stream after this slot's adds
    bool pending = false;           // `added` has been recorded
    // whole-batch split (trace_replica): the chunk partials of the replica's batch in its partial slot j
    // land in stage[j] on the home device, reduced there in batch order; stage_free[j] is recorded on the
    // home stream after that reduce
    DevBuf<double> stage[kSlots];
    hipEvent_t stage_free[kSlots] = {};
    bool stage_used[kSlots] = {};
    void release() {
        sum.release(); segs.release(); draws.release();
        for (DevBuf<double>& b : stage) b.release();
        if (added) (void)hipEventDestroy(added);
        for (hipEvent_t e : stage_free)
            if (e) (void)hipEventDestroy(e);
    }
};

struct rt_scene {
    DeviceState home;               // the device of rt_scene_create: epilogue, outputs, checkpoint
    std::vector<DeviceState*> replicas;   // rt_settings.devices[k] for k >= 1 (created on first use)
    HostScene hs;
    DescCopy desc;
    int num_prims = 0;
    int bvh_prims = 0;              // spheres + triangles (the primitives the BVHs cover)
    bool bvh_ok = true;             // both trees fit the traversal stack (depth <= RT_BVH_STACK)
    bool tri_bvh = false;           // the scene has a triangle BVH (pool chunk choice)
    double record_bytes = 0;
    hipEvent_t ev[2] = {};          // epilogue timing
    DevBuf<double> mean;
    std::vector<MergeSlot> merge;   // per shard (index in the render's device list): its staging on home
    DevBuf<float> post, post_raw;   // post_raw: pre-denoise floatData
    DevBuf<uint8_t> rgba;
    // rt_output.preview_rgba8: the running frame of each batch in flight, in mapped pinned host memory
    std::vector<uint8_t*> preview_host;
    std::vector<uint8_t*> preview_dev;    // the same buffers' device addresses
    size_t preview_host_n = 0;
    std::vector<hipEvent_t> batch_done;   // home stream: batch k's reduce, merges and preview done (slot k % ring)
    // preview frames / RGBA8-only epilogues: the gamma tables (launch_gamma_thresholds), one per gamma,
    // never rebuilt while a kernel may read them (gamma_table)
    std::vector<GammaSlot> gamma_slots;
    uint64_t gamma_tick = 0;
    std::atomic<int> cancel{0};
    uint32_t render_gen = 0;        // generation of the current render (device cancel words)
    uint32_t* ctl = nullptr;        // the render's control words (kCtl*), host address
    uint32_t* ctl_dev = nullptr;    // ... their device address (portable mapping: valid on every device)
    // the guided filter (rt_scene_set_guided): while on, epilogue() filters the mean along the frame's feature
    // buffers.  g_mean: sum / samples; guides: aov_kernel's records; g_ping / g_pong: the levels' frames
    // (rt_guided_filter_device uses g_ping beside the caller's d_out).  g_used is recorded after every use of
    // these buffers and waited for before the next, on whichever streams
    bool emitter_sampling = false;  // rt_scene_set_emitter_sampling (the list itself: hs.emit_kind / emit_idx)
    bool guided_on = false;
    rt_guided_params guided{};
    DevBuf<double> g_mean, g_ping, g_pong;
    DevBuf<float> guides;
    hipEvent_t g_used = nullptr;
    bool g_used_recorded = false;
    // the variance-guided form (rt_scene_set_guided_variance, pt_vguided.h): gvar_sigma > 0 is on.  gv_var: the
    // error estimate's var_mean of the frame; gv_ping / gv_pong: the levels' variance frames, gv_pong the last
    // level's (rt_guided_filtered_variance: gv_pixels pixels, 0 = none); gv_aux: rt_guided_filter_variance_device's
    // second scratch frame (it leaves gv_pong alone).  Under the g_used protocol like the colour frames
    double gvar_sigma = 0.0;
    DevBuf<double> gv_var, gv_ping, gv_pong, gv_aux;
    size_t gv_pixels = 0;
    // the error estimate (rt_scene_set_error_estimate, pt_error.h).  err_q: the pixels' second moments of the
    // samples home.sum holds (err_valid), err_groups chunk partials each; err_tile: the frame reduction's tile
    // partials; err_var / err_rel: rt_error_estimate's staging.  err_stats: the figures complete_batch read last
    bool err_on = false, err_valid = false;
    double err_threshold = 0.0;
    int err_min_samples = 0, err_groups = 0, err_samples = 0;
    DevBuf<double> err_q, err_tile, err_var;
    DevBuf<float> err_rel;
    CkptKey err_key{};              // the frame err_q is of (its crop: the estimate kernels' indexing)
    rt_error_stats err_stats{};
    size_t ckpt_pixels = 0;         // progressive state of the last rt_render / rt_render_resume:
    int ckpt_done = 0;              // `home.sum` holds samples [sample_begin, ckpt_done) of ckpt_pixels pixels
    CkptKey ckpt_key{};             // ... of this frame, crop, first sample, precision and seed
};

namespace {

int check_settings(const rt_settings* s, int* cw, int* ch) {
    if (!s) return fail(RT_ERR_INVALID, "settings is NULL");
    if (s->width <= 0 || s->height <= 0) return fail(RT_ERR_INVALID, "image %dx%d", s->width, s->height);
    if ((long long)s->width * s->height > 0xFFFFFFFFLL) return fail(RT_ERR_INVALID, "image too large for 32-bit pixel keys");
    *cw = s->crop_w > 0 ? s->crop_w : s->width;
    *ch = s->crop_h > 0 ? s->crop_h : s->height;
    if (s->crop_x0 < 0 || s->crop_y0 < 0 || s->crop_x0 + *cw > s->width || s->crop_y0 + *ch > s->height)
        return fail(RT_ERR_INVALID, "crop [%d,%d %dx%d] outside %dx%d", s->crop_x0, s->crop_y0, *cw, *ch, s->width,
                    s->height);
    if (s->samples < 0) return fail(RT_ERR_INVALID, "samples %d", s->samples);
    if (s->precision != RT_PREC_F64 && s->precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", s->precision);
    if (s->aa_mode < 0 || s->aa_mode > 2) return fail(RT_ERR_INVALID, "aa_mode %d", s->aa_mode);
    if (s->accel < RT_ACCEL_AUTO || s->accel > RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "accel %d", s->accel);
    if (s->denoise && (*cw != s->width || *ch != s->height))
        return fail(RT_ERR_INVALID, "denoise needs the full frame (PostProcessor.denoise clamps to the image edge)");
    if (s->device_count < 0 || s->device_count > RT_MAX_DEVICES)
        return fail(RT_ERR_INVALID, "device_count %d (at most %d)", s->device_count, RT_MAX_DEVICES);
    if (s->device_count > 1) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible");
        for (int k = 0; k < s->device_count; ++k)
            if (s->devices[k] < 0 || s->devices[k] >= ndev) return fail(RT_ERR_INVALID, "devices[%d] = %d of %d", k, s->devices[k], ndev);
    }
    return RT_OK;
}

// The gamma table of `gamma` on the scene's device (current), or nullptr when previews must take
// finalize_kernel.  A new gamma's table is built on the scene's own stream (`home.stream`, waited for:
// its exception count is read back) into a slot no kernel is reading: a free one, else the least
// recently used slot once its last reader has completed.  The caller's stream is never synchronized.
GammaSlot* gamma_table(rt_scene* sc, double gamma) {
    if (!preview_thresholds_ok(gamma)) return nullptr;
    GammaSlot* g = nullptr;
    for (GammaSlot& x : sc->gamma_slots)
        if (x.gamma == gamma) g = &x;
    if (!g) {
        sc->gamma_slots.reserve(kGammaSlots);      // never reallocated: a render keeps its slot's address
        if ((int)sc->gamma_slots.size() < kGammaSlots) {
            sc->gamma_slots.emplace_back();
            g = &sc->gamma_slots.back();
        } else {
            g = &sc->gamma_slots[0];
            for (GammaSlot& x : sc->gamma_slots)
                if (x.tick < g->tick) g = &x;
        }
        hipError_t e = g->used_recorded ? hipEventSynchronize(g->used) : hipSuccess;
        g->gamma = NAN;
        g->used_recorded = false;
        uint32_t words[2] = {0, 1};
        hipStream_t st = sc->home.stream;
        if (e == hipSuccess && !g->used) e = hipEventCreateWithFlags(&g->used, hipEventDisableTiming);
        if (e == hipSuccess) e = g->buf.ensure(sizeof(GammaTable));
        GammaTable* t = reinterpret_cast<GammaTable*>(g->buf.p);
        if (e == hipSuccess) e = launch_gamma_thresholds(gamma, t, st);
        if (e == hipSuccess) e = hipMemcpyAsync(words, &t->n_exc, sizeof words, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        g->gamma = gamma;
        g->ok = words[1] == 0;
    }
    g->tick = ++sc->gamma_tick;
    return g->ok ? g : nullptr;
}

// after a kernel reading g's table was enqueued on `st`
hipError_t gamma_used(GammaSlot* g, hipStream_t st) {
    const hipError_t e = hipEventRecord(g->used, st);
    if (e == hipSuccess) g->used_recorded = true;
    return e;
}

// RT_ACCEL_AUTO: the BVH unless the scene has almost no spheres/triangles (measured faster from 10
// primitives (Cornell) to 50k (mesh50k), DESIGN.md "BVH")
constexpr int kAutoBvhPrims = 8;

bool use_bvh(const rt_scene* sc, const rt_settings* s) {
    if (!sc->bvh_ok) return false;
    return s->accel == RT_ACCEL_BVH || (s->accel == RT_ACCEL_AUTO && sc->bvh_prims >= kAutoBvhPrims);
}

// f(the device scene's view in this precision)
template <class F>
auto with_view(const DeviceState& ds, int32_t precision, F&& f) {
    return precision == RT_PREC_F32 ? f(ds.s32.view) : f(ds.s64.view);
}

// the scene's guided-filter buffers on `st`: after their last use (on any stream), and marked used again
hipError_t guided_scratch_begin(rt_scene* sc, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (!sc->g_used) e = hipEventCreateWithFlags(&sc->g_used, hipEventDisableTiming);
    if (e == hipSuccess && sc->g_used_recorded) e = hipStreamWaitEvent(st, sc->g_used, 0);
    return e;
}
hipError_t guided_scratch_end(rt_scene* sc, hipStream_t st) {
    const hipError_t e = hipEventRecord(sc->g_used, st);
    if (e == hipSuccess) sc->g_used_recorded = true;
    return e;
}
// (a buffer that must grow is freed only once its last reader has finished)
template <class T>
hipError_t guided_ensure(rt_scene* sc, DevBuf<T>& b, size_t count) {
    if (count <= b.n && b.p) return hipSuccess;
    if (sc->g_used_recorded)
        if (const hipError_t e = hipEventSynchronize(sc->g_used)) return e;
    return b.ensure(count);
}

// The feature buffers of the settings' crop window into `guides` (8 floats per pixel) on `st`
hipError_t aovs_on(const rt_scene* sc, const rt_settings* s, int cw, int ch, float* guides, int* kind, int* idx,
                   hipStream_t st) {
    const AovFrame f{s->width, s->height, s->crop_x0, s->crop_y0, cw, ch};
    const bool bvh = use_bvh(sc, s);
    return with_view(sc->home, s->precision, [&](const auto& v) { return launch_aovs(v, bvh, f, guides, kind, idx, st); });
}

// The levels of the filter: color -> ... -> out, level l into `out` when an even number of levels follow it,
// else into `tmp`, so that no level runs in place (color, out and tmp are distinct frames)
hipError_t guided_levels(int w, int h, const rt_guided_params& p, const double* color, const float* guides, double* out,
                         double* tmp, hipStream_t st) {
    const double* src = color;
    for (int l = 0; l < p.levels; ++l) {
        double* dst = (p.levels - 1 - l) % 2 == 0 ? out : tmp;
        if (const hipError_t e = launch_guided_level(guided_level(w, h, p, l), src, guides, dst, st)) return e;
        src = dst;
    }
    return hipSuccess;
}

// The levels of the variance-guided form: (color, var) -> ... -> (out, vout) with (tmp, vtmp) in between, by
// guided_levels' rule.  keep_var false: the last level writes no variance (vout is then only a scratch frame,
// unused with one level)
hipError_t vguided_levels(int w, int h, const rt_guided_params& p, double sigma_variance, const double* color,
                          const double* var, const float* guides, double* out, double* vout, double* tmp, double* vtmp,
                          bool keep_var, hipStream_t st) {
    const double *src = color, *vsrc = var;
    for (int l = 0; l < p.levels; ++l) {
        const bool to_out = (p.levels - 1 - l) % 2 == 0;
        double* dst = to_out ? out : tmp;
        double* vdst = l == p.levels - 1 && !keep_var ? nullptr : to_out ? vout : vtmp;
        if (const hipError_t e = launch_vguided_level(vguided_level(w, h, p, sigma_variance, l), src, vsrc, guides, dst, vdst, st))
            return e;
        src = dst;
        vsrc = vdst;
    }
    return hipSuccess;
}

// mean, toneMap, gammaCorrect (+ PostProcessor.denoise), RGBA8 on `st` (ray-tracer.js:208-276).
// thresholds: an RGBA8-only epilogue through the gamma table (preview_kernel: the same bytes, 29 VGPRs
// instead of finalize_kernel's 80)
// While the guided filter is set (rt_scene_set_guided; full frames only, check_guided): the mean sum / samples,
// the frame's feature buffers, the filter, then the same kernels on the filtered mean with samples = 1 (x / 1
// is x: `mean` is the filtered mean).  `sum` is only read.
// With the variance form on (rt_scene_set_guided_variance; render_impl has checked that the render commits an
// estimate of at least 2 groups over the scene's own sums): var_mean of the committed samples and groups into
// gv_var, then the variance levels instead of the plain ones; gv_pong keeps the propagated variance.
hipError_t epilogue(rt_scene* sc, const rt_settings* s, int cw, int ch, const double* sum, double* mean, float* post,
                    uint8_t* rgba, hipStream_t st, bool thresholds = false) {
    FinalizeParams fp{cw * ch, s->samples, s->tone_map, s->exposure, s->gamma};
    bool guided = false;
    if (sc->guided_on) {
        const size_t n = (size_t)cw * ch;
        hipError_t e = guided_ensure(sc, sc->g_mean, 3 * n);
        if (e == hipSuccess) e = guided_ensure(sc, sc->g_ping, 3 * n);
        if (e == hipSuccess) e = guided_ensure(sc, sc->g_pong, 3 * n);
        if (e == hipSuccess) e = guided_ensure(sc, sc->guides, 8 * n);
        const bool variance = sc->gvar_sigma > 0.0;
        if (variance) {
            if (sum != sc->home.sum.p || !sc->err_on || !sc->err_valid || sc->err_groups < 2 || sc->err_samples <= 0)
                return hipErrorInvalidValue;
            sc->gv_pixels = 0;
            if (e == hipSuccess) e = guided_ensure(sc, sc->gv_var, 3 * n);
            if (e == hipSuccess) e = guided_ensure(sc, sc->gv_ping, 3 * n);
            if (e == hipSuccess) e = guided_ensure(sc, sc->gv_pong, 3 * n);
        }
        if (e == hipSuccess) e = guided_scratch_begin(sc, st);
        if (e == hipSuccess) e = launch_mean(sum, s->samples, sc->g_mean.p, 3 * n, st);
        if (e == hipSuccess && variance) {
            ImageParams im{};
            im.cw = cw;
            im.ch = ch;
            e = launch_error_estimate(im, sum, sc->err_q.p, sc->err_groups, sc->err_samples, sc->gv_var.p, nullptr, nullptr,
                                      nullptr, st);
        }
        if (e == hipSuccess) e = aovs_on(sc, s, cw, ch, sc->guides.p, nullptr, nullptr, st);
        if (e == hipSuccess && !variance)
            e = guided_levels(cw, ch, sc->guided, sc->g_mean.p, sc->guides.p, sc->g_pong.p, sc->g_ping.p, st);
        if (e == hipSuccess && variance) {
            e = vguided_levels(cw, ch, sc->guided, sc->gvar_sigma, sc->g_mean.p, sc->gv_var.p, sc->guides.p, sc->g_pong.p,
                               sc->gv_pong.p, sc->g_ping.p, sc->gv_ping.p, true, st);
            if (e == hipSuccess) sc->gv_pixels = n;
        }
        if (e != hipSuccess) return e;
        sum = sc->g_pong.p;
        fp.samples = 1;
        thresholds = false;
        guided = true;
    }
    hipError_t e = hipSuccess;
    if (thresholds && !s->denoise && !mean && !post && rgba)
        if (GammaSlot* g = gamma_table(sc, s->gamma)) {
            e = launch_finalize(fp, sum, nullptr, nullptr, rgba, st, g->table());
            return e == hipSuccess ? gamma_used(g, st) : e;
        }
    if (!s->denoise) e = launch_finalize(fp, sum, mean, post, rgba, st);
    else {
        e = sc->post_raw.ensure(4 * (size_t)cw * ch);
        if (e == hipSuccess) e = launch_finalize(fp, sum, mean, sc->post_raw.p, nullptr, st);
        if (e == hipSuccess) e = launch_denoise(cw, ch, s->denoise_weights[0], s->denoise_weights[1], sc->post_raw.p, post, rgba, st);
    }
    if (e == hipSuccess && guided) e = guided_scratch_end(sc, st);
    return e;
}

// the guided filter reads every pixel's 5 x 5 x 2^l neighbourhood: the full frame, as `denoise`
int check_guided(const rt_scene* sc, const rt_settings* s, int cw, int ch) {
    if (sc->guided_on && (cw != s->width || ch != s->height))
        return fail(RT_ERR_INVALID, "the guided filter needs the full frame (its taps reach across the image)");
    return RT_OK;
}

// the variance form's needs that do not depend on the batches: the guided filter set (check_guided: the full
// frame) and the error estimate on
int check_guided_variance(const rt_scene* sc) {
    if (!(sc->gvar_sigma > 0.0)) return RT_OK;
    if (!sc->guided_on) return fail(RT_ERR_INVALID, "the variance-guided form needs the guided filter set (rt_scene_set_guided)");
    if (!sc->err_on) return fail(RT_ERR_INVALID, "the variance-guided form needs the error estimate on (rt_scene_set_error_estimate)");
    return RT_OK;
}

ImageParams image_params(const rt_settings* s, int cw, int ch) {
    ImageParams im{};
    im.width = s->width; im.height = s->height;
    im.x0 = s->crop_x0; im.y0 = s->crop_y0; im.cw = cw; im.ch = ch;
    im.samples = s->samples;
    im.s_begin = std::max(0, s->sample_begin);
    im.s_end = s->sample_end > 0 ? std::min(s->sample_end, s->samples) : s->samples;
    im.max_depth = s->max_depth;
    im.aa_mode = s->aa_mode;
    im.seedm = host_seed_mix(s->seed);
    return im;
}

int check_accel(const rt_scene* sc, const rt_settings* s) {
    if (s->accel == RT_ACCEL_BVH && !sc->bvh_ok)
        return fail(RT_ERR_INVALID, "BVH deeper than the %d-entry traversal stack (too many primitives): use "
                    "RT_ACCEL_AUTO or RT_ACCEL_BRUTE", RT_BVH_STACK);
    return RT_OK;
}

// rt_settings.sum_order: the sample pool unless the caller asks for sample order (or RT_SAMPLE_POOL=0)
bool use_pool(const rt_settings* s) { return s->sum_order == RT_SUM_POOL && trace_uses_pool(); }

hipError_t trace(const rt_scene* sc, const DeviceState& ds, const rt_settings* s, const ImageParams& im,
                 const Counters& c, hipStream_t st, double* err_q = nullptr) {
    if (im.max_depth <= 0) return hipSuccess;   // rayColor(ray, depth<=0) is 0: nothing to trace
    const bool bvh = use_bvh(sc, s), pool = use_pool(s);
    return with_view(ds, s->precision, [&](const auto& v) { return launch_trace(v, im, c, bvh, pool, st, err_q); });
}

// The error estimate's launches after a batch's reduce, on the reduce's (home) stream and under its gate
// (render_impl; pt_error.h): the chunk moments of the partials just added (part == nullptr: launch_trace added
// them), then the frame's figures over the `samples` samples and `groups` chunk partials the sums hold once this
// batch is in, written to the batch's ErrorWords slot — and, with a threshold, the stop of every later batch.
// Before whatever lets the partials be overwritten (the slot's `reduced` event, the stage's `stage_free`).
struct ErrorBatch { int groups, samples, slot; };
hipError_t error_after_reduce(rt_scene* sc, const ErrorBatch& eb, const ImageParams& im, const double* part,
                              const ReduceGate* gate, hipStream_t st) {
    const uint32_t* skip = gate ? gate->skip : nullptr;
    hipError_t e = hipSuccess;
    if (part) e = launch_error_moments(im, sc->err_q.p, part, sc->tri_bvh, skip, st);
    if (e == hipSuccess && eb.groups >= 2)
        e = launch_error_estimate(im, sc->home.sum.p, sc->err_q.p, eb.groups, eb.samples, nullptr, nullptr, sc->err_tile.p,
                                  skip, st);
    if (e != hipSuccess) return e;
    ErrorFrame f{};
    f.tiles = crop_tiles(im.cw, im.ch);
    f.groups = eb.groups;
    f.samples = eb.samples;
    f.min_samples = sc->err_min_samples;
    f.pixels = (long long)im.cw * im.ch;
    f.threshold = gate ? sc->err_threshold : 0.0;      // only a gated render can stop
    f.tile_part = sc->err_tile.p;
    f.out = reinterpret_cast<ErrorWords*>(sc->ctl_dev + kCtlErr + eb.slot * kErrSlotWords);
    f.stop = sc->ctl_dev + kCtlStop;
    f.converged = sc->ctl_dev + kCtlConverged;
    f.skip = skip;
    return launch_error_frame(f, st);
}

// One overlapped batch on one device: the pool kernel writes the batch's chunk partials into slot `j`
// on tstream[j] (after the reduce that last read slot j), and `stream` adds them to the sums in chunk
// order once the trace is done.  Sums see the same additions in the same order as trace() of the batch
// (bit-identical), while the trace of batch k+1 may already run beside batch k's draining waves.
hipError_t trace_overlapped(rt_scene* sc, DeviceState& ds, const rt_settings* s, const ImageParams& im,
                            const Counters& c, int j, bool slot_used, const ReduceGate* gate,
                            const ErrorBatch* eb = nullptr) {
    if (im.max_depth <= 0 || im.s_end <= im.s_begin) return hipSuccess;
    const bool bvh = use_bvh(sc, s);
    DevBuf<double>& part = ds.slot_part(j);
    hipStream_t ts = ds.tstream[j];
    hipError_t e = hipSuccess;
    if (slot_used) e = hipStreamWaitEvent(ts, ds.reduced[j], 0);
    if (e == hipSuccess)
        e = with_view(ds, s->precision, [&](const auto& v) {
            return launch_trace_partials(v, im, c, bvh, part.p, part.n * sizeof(double), ts);
        });
    if (e == hipSuccess) e = hipEventRecord(ds.traced[j], ts);
    if (e == hipSuccess) e = hipStreamWaitEvent(ds.stream, ds.traced[j], 0);
    if (e == hipSuccess) e = launch_reduce(im, c.sum, part.p, sc->tri_bvh, ds.stream, gate);
    if (e == hipSuccess && eb) e = error_after_reduce(sc, *eb, im, part.p, gate, ds.stream);
    if (e == hipSuccess) e = hipEventRecord(ds.reduced[j], ds.stream);
    return e;
}

// A ReduceGate over the scene's control words: the `aborted` word's index, the samples the sums hold once the
// batch is committed, and (flag >= 0) the completion flag of a fused launch's batch or band
ReduceGate reduce_gate(const rt_scene* sc, int aborted_word, int32_t done_value, uint32_t* skip, int flag = -1) {
    ReduceGate g;
    g.aborted = sc->ctl_dev + aborted_word;
    g.stop = sc->ctl_dev + kCtlStop;
    g.done = reinterpret_cast<int32_t*>(sc->ctl_dev + kCtlDone);
    g.done_value = done_value;
    g.skip = skip;
    if (flag >= 0) g.complete = sc->ctl_dev + kCtlFlag + flag;
    return g;
}

// The chunk partials `src` (`bytes`) of a replica's batch into slot j of its staging on the home device
// (`doubles` large), over the replica's stream `st` once `before` has enqueued on it what produces them and
// the home stream's last reduce of that slot is done; then `reduce` of the staged partials on the home
// stream, after which the slot is free again.
template <class Before, class Reduce>
int stage_and_reduce(rt_scene* sc, DeviceState& ds, MergeSlot& m, int j, hipStream_t st, const double* src, size_t bytes,
                     size_t doubles, Before&& before, Reduce&& reduce) {
    DeviceState& h = sc->home;
    HIP_TRY(hipSetDevice(h.device));
    HIP_TRY(m.stage[j].ensure(doubles));
    if (!m.stage_free[j]) HIP_TRY(hipEventCreateWithFlags(&m.stage_free[j], hipEventDisableTiming));
    HIP_TRY(hipSetDevice(ds.device));
    HIP_TRY(before());
    if (m.stage_used[j]) HIP_TRY(hipStreamWaitEvent(st, m.stage_free[j], 0));
    HIP_TRY(hipMemcpyPeerAsync(m.stage[j].p, h.device, src, ds.device, bytes, st));
    HIP_TRY(hipEventRecord(ds.traced[j], st));              // its partials copied out
    HIP_TRY(hipSetDevice(h.device));
    HIP_TRY(hipStreamWaitEvent(h.stream, ds.traced[j], 0));
    HIP_TRY(reduce(m.stage[j].p));
    HIP_TRY(hipEventRecord(m.stage_free[j], h.stream));
    m.stage_used[j] = true;
    return RT_OK;
}

// One whole batch on a replica (the whole-batch split of render_impl): the pool kernel writes the
// batch's chunk partials into the replica's slot j on its tstream[j]; the same stream then copies them
// into the home device's staging slot j (once the home stream's last reduce of that slot is done), and
// the home stream adds them to the home sums in chunk order after the copy — exactly the reduce that
// trace_overlapped runs for a batch traced on the home device, in the same (batch) order, so the sums
// are bit-identical to the same batches on one device.  The replica's next trace into slot j follows
// the copy on the same stream.
int trace_replica(rt_scene* sc, DeviceState& ds, MergeSlot& m, const rt_settings* s, const ImageParams& im,
                  const Counters& c, int j, const ReduceGate* gate, const ErrorBatch* eb = nullptr) {
    if (im.max_depth <= 0 || im.s_end <= im.s_begin) return RT_OK;
    DeviceState& h = sc->home;
    const size_t bytes = pool_plan(im.cw, im.ch, im.s_end - im.s_begin, sc->tri_bvh, im.pool_chunk).part_bytes;
    const bool bvh = use_bvh(sc, s);
    DevBuf<double>& part = ds.slot_part(j);
    hipStream_t ts = ds.tstream[j];
    return stage_and_reduce(
        sc, ds, m, j, ts, part.p, bytes, bytes / sizeof(double),
        [&] {
            return with_view(ds, s->precision, [&](const auto& v) {
                return launch_trace_partials(v, im, c, bvh, part.p, part.n * sizeof(double), ts);
            });
        },
        [&](const double* staged) {
            hipError_t e = launch_reduce(im, h.sum.p, staged, sc->tri_bvh, h.stream, gate);
            if (e == hipSuccess && eb) e = error_after_reduce(sc, *eb, im, staged, gate, h.stream);
            return e;
        });
}

// The per-pixel counters (segments, draws) of the replicas of a whole-batch split, added into the home
// device's once all their batches are traced (integer sums: any order).  The replica's accumulation
// stream first waits for its trace streams.
int merge_counters(rt_scene* sc, const std::vector<DeviceState*>& states, size_t n, bool segs, bool draws) {
    DeviceState& h = sc->home;
    for (size_t k = 0; k < states.size(); ++k) {
        DeviceState* ds = states[k];
        if (ds == &h || !(segs || draws)) continue;
        MergeSlot& m = sc->merge[k];
        HIP_TRY(hipSetDevice(h.device));
        if (segs) HIP_TRY(m.segs.ensure(n));
        if (draws) HIP_TRY(m.draws.ensure(n));
        HIP_TRY(hipSetDevice(ds->device));
        if (segs) HIP_TRY(hipMemcpyPeerAsync(m.segs.p, h.device, ds->segs.p, ds->device, n * sizeof(uint32_t), ds->stream));
        if (draws) HIP_TRY(hipMemcpyPeerAsync(m.draws.p, h.device, ds->draws.p, ds->device, n * sizeof(uint32_t), ds->stream));
        HIP_TRY(hipEventRecord(ds->copy_ev, ds->stream));
        HIP_TRY(hipSetDevice(h.device));
        HIP_TRY(hipStreamWaitEvent(h.stream, ds->copy_ev, 0));
        if (segs) HIP_TRY(launch_add<uint32_t>(h.segs.p, m.segs.p, n, h.stream));
        if (draws) HIP_TRY(launch_add<uint32_t>(h.draws.p, m.draws.p, n, h.stream));
    }
    return RT_OK;
}

// Peer access between the scene's device and a replica's (hipMemcpyPeerAsync then runs over xGMI
// directly instead of a staged copy).  Without a peer path (PCIe-only topologies, device subsets across
// root complexes) the copies still work — HIP stages them through host memory — so that is not an
// error: it is reported once on stderr and the render goes on.  Only an unexpected failure of
// hipDeviceEnablePeerAccess fails the render.
int enable_peer(int a, int b) {
    if (a == b) return RT_OK;
    for (int k = 0; k < 2; ++k) {
        const int from = k ? b : a, to = k ? a : b;
        int can = 0;
        HIP_TRY(hipDeviceCanAccessPeer(&can, from, to));
        if (!can) {
            static std::atomic<bool> told{false};
            if (!told.exchange(true))
                fprintf(stderr, "[rt_hip] device %d has no peer access to device %d: the sample split's copies are "
                        "staged through host memory\n", from, to);
            continue;
        }
        HIP_TRY(hipSetDevice(from));
        const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
        if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        else if (e != hipSuccess) return fail(RT_ERR_DEVICE, "hipDeviceEnablePeerAccess(%d -> %d): %s", from, to, hipGetErrorString(e));
    }
    return RT_OK;
}

// Sample-pool chunk partials (pool_partial_bytes, pt_trace.hip): all of a launch's chunks when they fit
// the budget (RT_PART_MB, default 2 GiB, at most 10 % of the free device memory), else as many
// chunks as fit (launch_trace then splits the samples over several launches).  RTOW 1080p x 512 spp
// needs 0.3 GB; a launch with a single chunk needs none.  Kept by the device state between renders.
size_t part_budget() {
    static const size_t budget = [] {
        const char* e = getenv("RT_PART_MB");
        return (size_t)(e ? std::max(1LL, atoll(e)) : 2048LL) << 20;
    }();
    return budget;
}

// A device state's scratch may still be read by an asynchronous call on another stream (rt_trace_device):
// wait for its last user before freeing or reallocating it (hipFree's implicit device synchronization is
// not relied upon).
hipError_t scratch_idle(DeviceState& ds) {
    return ds.scratch_used ? hipEventSynchronize(ds.scratch_ev) : hipSuccess;
}

// single: a launch of one chunk gets its partials too (the error estimate reads them, launch_trace's err_q)
int ensure_partials(const rt_scene* sc, DeviceState& ds, int cw, int ch, int samples, bool pool, Counters& c,
                    int chunk = 0, bool single = false) {
    if (!pool || samples <= 0 || cw <= 0 || ch <= 0) return RT_OK;
    const size_t per_chunk = (size_t)crop_tiles(cw, ch) * kPartialBytesPerTile;
    size_t want_all = pool_partial_bytes(cw, ch, samples, sc->tri_bvh, chunk);
    if (want_all == 0 && single) want_all = per_chunk;
    if (want_all == 0) return RT_OK;
    size_t want = want_all;
    if (want > ds.part.n * sizeof(double)) {
        HIP_TRY(scratch_idle(ds));
        size_t free_b = 0, total_b = 0, cap = part_budget();
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) cap = std::min(cap, (free_b + ds.part.n * sizeof(double)) / 10);
        want = std::min(want, std::max<size_t>(cap / per_chunk, 1) * per_chunk);
        while (want > ds.part.n * sizeof(double)) {
            if (ds.part.ensure(want / sizeof(double)) == hipSuccess) break;
            (void)hipGetLastError();
            if (want == per_chunk) return fail(RT_ERR_DEVICE, "sample pool: cannot allocate %zu bytes", per_chunk);
            want = std::max<size_t>(want / per_chunk / 2, 1) * per_chunk;
        }
    }
    c.part = ds.part.p;
    c.part_bytes = ds.part.n * sizeof(double);
    return RT_OK;
}

// Both partial slots of the overlapped batches, `bytes` each (one batch's chunks: pool_plan).  False
// (no error) when they do not fit the budget: the render then runs its batches one after the other.
bool ensure_overlap_partials(DeviceState& ds, size_t bytes) {
    bool have = true;
    size_t held = 0;
    for (int j = 0; j < kSlots; ++j) {
        have = have && ds.slot_part(j).p && ds.slot_part(j).n * sizeof(double) >= bytes;
        held += ds.slot_part(j).n * sizeof(double);
    }
    if (bytes == 0 || have) return true;
    if (scratch_idle(ds) != hipSuccess) return false;
    size_t free_b = 0, total_b = 0, cap = part_budget();
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) cap = std::min(cap, (free_b + held) / 10);
    if (kSlots * bytes > cap) return false;
    for (int j = 0; j < kSlots; ++j)
        if (ds.slot_part(j).ensure(bytes / sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    return true;
}

// Fused batches: the chunk partials of all `nb` batches of a render (`doubles` each) and their item
// counters.  The partials budget is RT_FUSED_MB (default 8 GiB, at most 10 % of the free device
// memory; config 3 in 16 batches needs 0.8 GB); false (no error) when they do not fit: the render then
// launches its batches one by one.
bool ensure_fused(DeviceState& ds, size_t doubles, int nb) {
    const size_t bytes = doubles * (size_t)nb * sizeof(double);
    if (bytes == 0) return false;
    if (ds.fused_part.n * sizeof(double) < bytes) {
        static const size_t budget = [] {   // thread-safe initialization (concurrent renders of other scenes)
            const char* e = getenv("RT_FUSED_MB");
            return (size_t)(e ? std::max(0LL, atoll(e)) : 8192LL) << 20;
        }();
        size_t free_b = 0, total_b = 0, cap = budget;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) cap = std::min(cap, (free_b + ds.fused_part.n * sizeof(double)) / 10);
        if (bytes > cap) return false;
        ds.fused_part.release();
        if (ds.fused_part.ensure(bytes / sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    }
    if (ds.fused_count.ensure((size_t)nb) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

// A device state's scratch buffers (chunk partials, work totals) are shared by every call on it.  A
// call on stream `st` first waits for the previous user of the scratch (possibly another stream:
// rt_trace_device on a caller's stream, rt_render on the scene's own) and records the event again
// when it has enqueued its last use, so asynchronous calls on different streams never overlap on it.
hipError_t order_scratch(DeviceState& ds, hipStream_t st) {
    if (!ds.scratch_used || ds.scratch_stream == st) return hipSuccess;
    return hipStreamWaitEvent(st, ds.scratch_ev, 0);
}
hipError_t release_scratch(DeviceState& ds, hipStream_t st) {
    ds.scratch_stream = st;
    ds.scratch_used = true;
    return hipEventRecord(ds.scratch_ev, st);
}

// totals = [segments, BVH nodes, sphere tests, triangle tests] of the launches
void fill_stats(rt_stats* st, const rt_scene* sc, const rt_settings* s, const unsigned long long* totals, size_t n,
                const ImageParams& im) {
    st->samples = (uint64_t)n * (uint64_t)std::max(0, im.s_end - im.s_begin);
    st->segments = totals[0];
    if (use_bvh(sc, s)) {
        const uint64_t brute = (uint64_t)sc->home.s64.view.num_planes + sc->home.s64.view.num_boxes;
        st->node_visits = totals[1];
        st->sphere_tests = totals[2];
        st->tri_tests = totals[3];
        st->prim_tests = totals[2] + totals[3] + totals[0] * brute;
        // a walk step reads a 64-B two-child node, or a grid cell's 8-B record range (node_visits then
        // counts cells)
        const bool grid = with_view(sc->home, s->precision, [](const auto& v) { return trace_walks_grid(v); });
        st->algorithmic_bytes = (grid ? 8.0 : 64.0) * totals[1] + 16.0 * totals[2] + 36.0 * totals[3] +
                                24.0 * totals[0] * brute + 12.0 * (double)n;
    } else {
        st->node_visits = st->sphere_tests = st->tri_tests = 0;
        st->prim_tests = totals[0] * (uint64_t)sc->num_prims;
        st->algorithmic_bytes = (double)totals[0] * sc->record_bytes + 12.0 * (double)n;
    }
}

// the statistics of a trace on the home device alone (rt_trace_device, _bands), once its stream has been waited for
int trace_stats(rt_stats* st, const rt_scene* sc, const rt_settings* s, const DeviceState& ds, const unsigned long long* totals,
                size_t n, const ImageParams& im, double t_start) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ds.ev[0], ds.ev[1]));
    st->kernel_ms = ms;
    st->finalize_ms = 0;
    fill_stats(st, sc, s, totals, n, im);
    st->wall_ms = now_ms() - t_start;
    return RT_OK;
}

// The device states of a render: shard k of rt_settings.devices (k = 0: the scene's own device when
// it is listed first, else a replica), created and uploaded on first use.
int shard_states(rt_scene* sc, const rt_settings* s, std::vector<DeviceState*>& out) {
    out.clear();
    const int n = s->device_count > 1 ? s->device_count : 1;
    if (n == 1) {
        out.push_back(&sc->home);
        return RT_OK;
    }
    for (int k = 0; k < n; ++k) {
        const int dev = s->devices[k];
        if (k == 0 && dev == sc->home.device) {
            out.push_back(&sc->home);
            continue;
        }
        const size_t slot = (size_t)k;                     // replica of shard k
        if (sc->replicas.size() <= slot) sc->replicas.resize(slot + 1, nullptr);
        DeviceState*& r = sc->replicas[slot];
        if (r && r->device != dev) {                       // the device list changed: re-create
            r->release();
            delete r;
            r = nullptr;
        }
        if (!r) {
            int rc = enable_peer(sc->home.device, dev);
            if (rc) return rc;
            r = new DeviceState();
            rc = r->init(dev, sc->hs, sc->desc.d);
            if (rc) {
                r->release();
                delete r;
                r = nullptr;
                return rc;
            }
        }
        out.push_back(r);
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

const char* rt_last_error(void) { return g_error.c_str(); }

int rt_device_count(int* count) {
    if (!count) return fail(RT_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        *count = 0;
        return fail(RT_ERR_NO_DEVICE, "no HIP device: %s", hipGetErrorString(e));
    }
    *count = n;
    return RT_OK;
}

int rt_scene_create(const rt_scene_desc* caller_desc, int device, rt_scene** out) {
    if (!caller_desc || !out) return fail(RT_ERR_INVALID, "NULL argument");
    *out = nullptr;
    rt_scene_desc filled;                 // the texture fields only where the caller says it filled them
    if (!desc_as_filled(caller_desc, filled))
        return fail(RT_ERR_INVALID, "abi_version %d != %d", caller_desc->abi_version, RT_ABI_VERSION);
    const rt_scene_desc* desc = &filled;
    if (desc->num_objects < 0 || (desc->num_objects > 0 && !desc->objects)) return fail(RT_ERR_INVALID, "objects");
    if (desc->num_materials < 0 || (desc->num_materials > 0 && !desc->materials)) return fail(RT_ERR_INVALID, "materials");
    if (desc->num_triangles < 0 || (desc->num_triangles > 0 && !desc->triangles)) return fail(RT_ERR_INVALID, "triangles");
    if (desc->background < 0 || desc->background > RT_BG_NAN) return fail(RT_ERR_INVALID, "background %d", desc->background);
    for (int i = 0; i < 512; ++i)
        if (desc->perm[i] < 0 || desc->perm[i] > 255) return fail(RT_ERR_INVALID, "perm[%d] = %d", i, desc->perm[i]);
    for (int i = 0; i < desc->num_materials; ++i)
        if (desc->materials[i].type < 0 || desc->materials[i].type > RT_MAT_EMISSIVE)
            return fail(RT_ERR_INVALID, "material %d: type %d", i, desc->materials[i].type);
    {
        std::string terr;                      // host-only checks first: a bad descriptor is RT_ERR_INVALID
        if (!validate_textures(*desc, terr)) return fail(RT_ERR_INVALID, "%s", terr.c_str());   // with or without a device
        if (!validate_lights(*desc, terr)) return fail(RT_ERR_INVALID, "%s", terr.c_str());
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID, "device %d of %d", device, ndev);
    rt_scene* sc = new rt_scene();
    std::string err;
    if (!pack_host(*desc, sc->hs, err)) {
        delete sc;
        return fail(RT_ERR_INVALID, "%s", err.c_str());
    }
    build_bvhs(sc->hs);
    choose_walk(sc->hs, *desc);
    sc->desc.set(*desc);
    sc->num_prims = sc->hs.num_prims;
    sc->bvh_prims = (int)(sc->hs.sphere_r.size() + sc->hs.tri_mat.size());
    sc->bvh_ok = sc->hs.bvh_depth <= RT_BVH_STACK;
    sc->tri_bvh = !sc->hs.tri_wide.empty();
    sc->record_bytes = sc->hs.record_bytes;
    int rc = sc->home.init(device, sc->hs, sc->desc.d);
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && !rc && e == hipSuccess; ++k) e = hipEventCreate(&sc->ev[k]);
    if (!rc && e == hipSuccess)
        e = hipHostMalloc((void**)&sc->ctl, kCtlWords * sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
    if (!rc && e == hipSuccess) {
        memset(sc->ctl, 0, kCtlWords * sizeof(uint32_t));
        e = hipHostGetDevicePointer((void**)&sc->ctl_dev, sc->ctl, 0);
    }
    if (!rc && e != hipSuccess) rc = fail(RT_ERR_DEVICE, "event create: %s", hipGetErrorString(e));
    if (rc) {
        rt_scene_destroy(sc);
        return rc;
    }
    *out = sc;
    return RT_OK;
}

void rt_scene_destroy(rt_scene* sc) {
    if (!sc) return;
    for (DeviceState* r : sc->replicas)
        if (r) {
            r->release();
            delete r;
        }
    sc->home.release();
    (void)hipSetDevice(sc->home.device);
    sc->mean.release(); sc->post.release(); sc->post_raw.release();
    sc->g_mean.release(); sc->g_ping.release(); sc->g_pong.release(); sc->guides.release();
    sc->gv_var.release(); sc->gv_ping.release(); sc->gv_pong.release(); sc->gv_aux.release();
    sc->err_q.release(); sc->err_tile.release(); sc->err_var.release(); sc->err_rel.release();
    if (sc->g_used) (void)hipEventDestroy(sc->g_used);
    for (MergeSlot& m : sc->merge) m.release();
    sc->rgba.release();
    for (GammaSlot& g : sc->gamma_slots) g.release();
    for (uint8_t* p : sc->preview_host)
        if (p) (void)hipHostFree(p);
    if (sc->ctl) (void)hipHostFree(sc->ctl);
    for (hipEvent_t e : {sc->ev[0], sc->ev[1]})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : sc->batch_done)
        if (e) (void)hipEventDestroy(e);
    delete sc;
}

int rt_cancel(rt_scene* sc) {
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    sc->cancel.store(1);
    if (sc->ctl) {
        ctl_cancel(sc->ctl, 1);             // the one-wave pool kernels skip their items from here on
        (void)cancel_pool_launches(sc->ctl_dev + kCtlCancel);   // the LDS pool launches' queues end
    }
    return RT_OK;
}

}  // extern "C"

namespace {

// Adds the replicas' sums (and counters) of the batch just traced into the home device's, in shard
// order, without a host wait: each replica copies its batch sums over xGMI into its own staging slot on
// the home device from its own stream (the copies of all replicas run at once, one link each) and then
// zeroes them for its next batch; the home stream waits for each copy and adds the slots in shard
// order, then records that the slot is free (the replica's next copy waits for that).  The home
// device's own trace of the next batch follows the adds on its stream, so the running sums see the same
// sequence of additions as a merge after every batch done synchronously: a checkpoint holds exactly
// the merged batches and a resumed render is bit-identical.
int merge_shards(rt_scene* sc, const std::vector<DeviceState*>& states, size_t n, bool segs, bool draws) {
    DeviceState& h = sc->home;
    if (sc->merge.size() < states.size()) sc->merge.resize(states.size());
    for (size_t k = 0; k < states.size(); ++k) {
        DeviceState* ds = states[k];
        if (ds == &h) continue;
        MergeSlot& m = sc->merge[k];
        HIP_TRY(hipSetDevice(h.device));
        HIP_TRY(m.sum.ensure(3 * n));
        if (segs) HIP_TRY(m.segs.ensure(n));
        if (draws) HIP_TRY(m.draws.ensure(n));
        if (!m.added) HIP_TRY(hipEventCreateWithFlags(&m.added, hipEventDisableTiming));
        HIP_TRY(hipSetDevice(ds->device));
        if (m.pending) HIP_TRY(hipStreamWaitEvent(ds->stream, m.added, 0));    // the slot's last adds are done
        HIP_TRY(hipMemcpyPeerAsync(m.sum.p, h.device, ds->sum.p, ds->device, 3 * n * sizeof(double), ds->stream));
        if (segs) HIP_TRY(hipMemcpyPeerAsync(m.segs.p, h.device, ds->segs.p, ds->device, n * sizeof(uint32_t), ds->stream));
        if (draws) HIP_TRY(hipMemcpyPeerAsync(m.draws.p, h.device, ds->draws.p, ds->device, n * sizeof(uint32_t), ds->stream));
        HIP_TRY(hipEventRecord(ds->copy_ev, ds->stream));
        HIP_TRY(hipMemsetAsync(ds->sum.p, 0, 3 * n * sizeof(double), ds->stream));
        if (segs) HIP_TRY(hipMemsetAsync(ds->segs.p, 0, n * sizeof(uint32_t), ds->stream));
        if (draws) HIP_TRY(hipMemsetAsync(ds->draws.p, 0, n * sizeof(uint32_t), ds->stream));
        HIP_TRY(hipSetDevice(h.device));
        HIP_TRY(hipStreamWaitEvent(h.stream, ds->copy_ev, 0));
        HIP_TRY(launch_add<double>(h.sum.p, m.sum.p, 3 * n, h.stream));
        if (segs) HIP_TRY(launch_add<uint32_t>(h.segs.p, m.segs.p, n, h.stream));
        if (draws) HIP_TRY(launch_add<uint32_t>(h.draws.p, m.draws.p, n, h.stream));
        HIP_TRY(hipEventRecord(m.added, h.stream));
        m.pending = true;
    }
    return RT_OK;
}

// ---- rt_render and rt_render_resume: render_impl and its stages (the decisions: render_plan.h) ----

// Batch kb of a run as its launches see it
struct Batch {
    int kb, b, be;                    // samples [b, be)
    ReduceGate gate;                  // gated runs: the batch's cancel and commit words (gp: &gate, else NULL)
    const ReduceGate* gp = nullptr;
    ErrorBatch eb{};                  // the error estimate's launches follow the batch's reduce, under its gate
    const ErrorBatch* ebp = nullptr;  // (error_after_reduce)
    bool previewed = false;           // the reduce wrote the running frame too (RT_FUSED_PREVIEW)
};

// the refusals that need neither the devices nor the plan
int check_render(const rt_scene* sc, const rt_settings* s, const double* sums_in, int* cw, int* ch) {
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    int rc = check_settings(s, cw, ch);
    if (!rc) rc = check_accel(sc, s);
    if (!rc) rc = check_guided(sc, s, *cw, *ch);
    if (!rc) rc = check_guided_variance(sc);
    if (!rc && sc->gvar_sigma > 0.0 && sums_in)
        rc = fail(RT_ERR_INVALID, "the variance-guided form needs the error estimate: a resume from host sums leaves none");
    if (rc) return rc;
    // the error estimate reads the sample pool's chunk partials: renders without them are refused while it is on
    if (sc->err_on) {
        if (s->sum_order != RT_SUM_POOL)
            return fail(RT_ERR_INVALID, "the error estimate needs the sample pool (RT_SUM_SAMPLE_ORDER has no chunk partials)");
        if (!use_pool(s)) return fail(RT_ERR_INVALID, "the error estimate needs the sample pool (it is switched off)");
        if (s->max_depth <= 0) return fail(RT_ERR_INVALID, "the error estimate needs max_depth > 0 (nothing is traced)");
    } else if (sc->err_threshold > 0.0)
        return fail(RT_ERR_INVALID, "a noise threshold needs the error estimate on");
    return RT_OK;
}

// One render between its stages: what the stage functions of render_impl share.
struct RenderRun {
    rt_scene* const sc;
    DeviceState& h;                   // the scene's home state
    rt_settings settings;             // the caller's settings (a threshold stop: `samples` as committed, for the epilogue)
    const rt_settings* const s = &settings;
    const rt_output* const out;
    const double* const sums_in;      // the sums to start from (NULL: zeros, or `resident`: the scene's checkpoint)
    const bool resident;
    const int cw, ch;
    const size_t n = (size_t)cw * ch;
    const bool want_segs = out && out->segments, want_draws = out && out->draws;
    bool err_active = false;          // this render starts or continues the scene's error estimate
    RenderPlan p;
    ImageParams im{};                 // samples [p.s0, p.s1)
    std::vector<DeviceState*> states;
    std::vector<Counters> cs;         // per state
    int enqueued = 0;                 // batches [0, enqueued) are queued on the GPU
    std::vector<unsigned> slots_used; // whole-batch split: the partial slots each device traced into
    bool fused_launched = false;
    GammaSlot* thresholds = nullptr;  // the running frames' RGBA8 thresholds for this gamma (preview_kernel)
    bool stopped = false;             // the noise threshold ended the render early

    RenderRun(rt_scene* sc, const rt_settings& st, const rt_output* out, const double* sums_in, bool resident, int cw, int ch)
        : sc(sc), h(sc->home), settings(st), out(out), sums_in(sums_in), resident(resident), cw(cw), ch(ch) {}
    RenderRun(const RenderRun&) = delete;

    // The run's plan (render_plan.h; its fit questions allocate the buffers asked about), the refusals that
    // depend on it, and the scene's error-estimate state for this render
    int make_plan(int first) {
        cs.resize(states.size());
        slots_used.assign(states.size(), 0);
        for (DeviceState* ds : states) {
            HIP_TRY(hipSetDevice(ds->device));
            HIP_TRY(ds->sum.ensure(3 * n));
            HIP_TRY(ds->total.ensure(kTotalSlots));
        }
        // The error estimate of this render (pt_error.h): rt_render starts it, a resident resume of a render that
        // has one continues it; a resume from host sums (or from sums without moments) leaves none
        err_active = sc->err_on && !sums_in && (!resident || (sc->err_valid && sc->err_key == ckpt_key(s, cw, ch)));
        RenderPlanIn in{};
        in.cw = cw; in.ch = ch;
        in.sample_begin = s->sample_begin; in.sample_end = s->sample_end; in.samples = s->samples;
        in.batch_samples = s->batch_samples; in.max_depth = s->max_depth;
        in.pool = use_pool(s);
        in.first = first;
        in.tri_bvh = sc->tri_bvh;
        in.shards = (int)states.size();
        in.home_first = states[0] == &h;
        in.want_segs = want_segs; in.want_draws = want_draws;
        in.want_preview = out && out->preview_rgba8;
        in.err_active = err_active;
        in.err_groups = resident ? sc->err_groups : 0;
        in.knobs = render_knobs();
        hipError_t fit_error = hipSuccess;
        p = plan_render(in, [&](const FitAsk& a) {
            DeviceState& ds = *states[a.shard];
            if (fit_error == hipSuccess) fit_error = hipSetDevice(ds.device);
            if (fit_error != hipSuccess) return false;
            return a.kind == FitAsk::Fused ? ensure_fused(ds, a.doubles, a.batches) : ensure_overlap_partials(ds, a.bytes);
        });
        HIP_TRY(fit_error);
        im = image_params(s, cw, ch);
        im.s_begin = p.s0;
        if (p.whole() && sc->merge.size() < states.size()) sc->merge.resize(states.size());
        if (p.gated) {
            HIP_TRY(hipSetDevice(h.device));
            HIP_TRY(h.gate_skip.ensure(1));
        }
        if (sc->err_on) {
            if (p.devices == DeviceMode::Split)
                return fail(RT_ERR_INVALID, "the error estimate needs whole batches per device (this render splits every "
                            "batch's samples over the devices)");
            if (sc->err_threshold > 0.0 && p.nb > 1 && !p.gated)
                return fail(RT_ERR_INVALID, "the noise threshold needs overlapped batches (their commit gates stop the render)");
            if (!resident) sc->err_groups = sc->err_samples = 0;
            sc->err_valid = err_active && resident;
            if (!err_active || !resident) sc->err_stats = rt_error_stats{};
            ctl_store(sc->ctl, kCtlConverged, 0);
        }
        if (err_active) {
            HIP_TRY(hipSetDevice(h.device));
            HIP_TRY(sc->err_q.ensure(3 * n));
            HIP_TRY(sc->err_tile.ensure(3 * (size_t)crop_tiles(cw, ch)));
            sc->err_key = ckpt_key(s, cw, ch);
            if (p.nb > 0) sc->err_stats.chunk_samples = p.err_chunk;
            else p.err_chunk = sc->err_stats.chunk_samples;
        }
        // the variance-guided epilogue reads var_mean: refused here, before anything is traced, unless the finished
        // render holds an estimate of at least 2 groups (a noise-threshold stop never comes before 2 groups)
        if (sc->gvar_sigma > 0.0 && p.final_groups < 2)
            return fail(RT_ERR_INVALID, "the variance-guided form needs an estimate of at least 2 groups: this render would "
                        "commit %d (more batches, or a resident resume of a render with an estimate)", p.final_groups);
        return RT_OK;
    }

    // A state's sums and per-pixel counters as the render starts, on its stream: the sums zeroed — on the home
    // state copied from the caller's sums, or left as they are (the resident checkpoint) — and the counters
    // zeroed.  c: a state that traces (its work totals zeroed too, and its counters wired into c)
    int start_sums(DeviceState& ds, Counters* c) {
        const bool home = &ds == &sc->home;
        if (resident && home) {
            // the scene's checkpoint is already in place
        } else if (sums_in && home)
            HIP_TRY(hipMemcpyAsync(ds.sum.p, sums_in, 3 * n * sizeof(double), hipMemcpyHostToDevice, ds.stream));
        else
            HIP_TRY(hipMemsetAsync(ds.sum.p, 0, 3 * n * sizeof(double), ds.stream));
        if (c) HIP_TRY(hipMemsetAsync(ds.total.p, 0, kTotalSlots * sizeof(unsigned long long), ds.stream));
        if (want_segs) {
            HIP_TRY(ds.segs.ensure(n));
            HIP_TRY(hipMemsetAsync(ds.segs.p, 0, n * sizeof(uint32_t), ds.stream));
            if (c) c->segs = ds.segs.p;
        }
        if (want_draws) {
            HIP_TRY(ds.draws.ensure(n));
            HIP_TRY(hipMemsetAsync(ds.draws.p, 0, n * sizeof(uint32_t), ds.stream));
            if (c) c->draws = ds.draws.p;
        }
        return RT_OK;
    }

    // Every device's buffers and streams at the start of the batches, the completion events and preview frames
    // of the ring, and the checkpoint state from which a failing render leaves a consistent checkpoint
    int prepare_devices() {
        int rc;
        for (size_t k = 0; k < states.size(); ++k) {
            DeviceState& ds = *states[k];
            HIP_TRY(hipSetDevice(ds.device));
            Counters& c = cs[k];
            c = Counters{ds.sum.p, nullptr, nullptr, ds.total.p};
            c.cancel_dev = ds.cancel_word.p;
            c.cancel_gen = sc->render_gen;
            const int ns = p.first_share((int)k);
            if (!p.overlap() && s->max_depth > 0 &&
                (rc = ensure_partials(sc, ds, cw, ch, ns, use_pool(s), c, p.batch_chunk((int)k, ns), err_active)))
                return rc;
            HIP_TRY(order_scratch(ds, ds.stream));
            if ((rc = start_sums(ds, &c))) return rc;
            HIP_TRY(hipEventRecord(ds.ev[0], ds.stream));
            if (p.overlap()) {                        // the trace streams start after this set-up
                HIP_TRY(hipEventRecord(ds.setup_ev, ds.stream));
                for (hipStream_t t : ds.tstream) HIP_TRY(hipStreamWaitEvent(t, ds.setup_ev, 0));
            }
        }
        if (states[0] != &h) {                      // the home device only merges: its buffers start here
            HIP_TRY(hipSetDevice(h.device));
            HIP_TRY(h.sum.ensure(3 * n));
            if ((rc = start_sums(h, nullptr))) return rc;
        }
        HIP_TRY(hipSetDevice(h.device));
        if (err_active && !resident) HIP_TRY(hipMemsetAsync(sc->err_q.p, 0, 3 * n * sizeof(double), h.stream));
        if ((int)sc->batch_done.size() < p.ring) sc->batch_done.resize(p.ring, nullptr);
        for (hipEvent_t& e : sc->batch_done)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (p.preview && (sc->preview_host_n < 4 * n || (int)sc->preview_host.size() < p.ring)) {
            for (uint8_t*& q : sc->preview_host) {
                if (q) (void)hipHostFree(q);
                q = nullptr;
            }
            sc->preview_host_n = 0;
            sc->preview_host.assign(p.ring, nullptr);
            sc->preview_dev.assign(p.ring, nullptr);
            for (int k = 0; k < p.ring; ++k) {
                HIP_TRY(hipHostMalloc((void**)&sc->preview_host[k], 4 * n, hipHostMallocMapped));
                HIP_TRY(hipHostGetDevicePointer((void**)&sc->preview_dev[k], sc->preview_host[k], 0));
            }
            sc->preview_host_n = 4 * n;
        }
        // the running frames' RGBA8 thresholds for this gamma (exact bytes without a binary64 pow: preview_kernel)
        if (p.preview) {
            HIP_TRY(hipSetDevice(h.device));
            thresholds = gamma_table(sc, s->gamma);
        }
        sc->ckpt_pixels = n;
        sc->ckpt_done = p.s0;
        sc->ckpt_key = ckpt_key(s, cw, ch);
        ctl_store(sc->ctl, kCtlStop, 0);
        ctl_store(sc->ctl, kCtlDone, (uint32_t)p.s0);
        return RT_OK;
    }

    // the running frame's epilogue parameters once the sums hold samples [base, done)
    FinalizeParams frame_params(int done) {
        return FinalizeParams{(int)n, done - p.base, s->tone_map, s->exposure, s->gamma};
    }

    // a trace launch's counters with the run's cancel word and the batch's `aborted` word (gated runs)
    Counters with_cancel(const Batch& bt, Counters c) {
        if (p.gated) {
            if (render_knobs().item_cancel) c.cancel = sc->ctl_dev + kCtlCancel;
            c.aborted = const_cast<uint32_t*>(bt.gate.aborted);
        }
        return c;
    }

    // batch kb's samples, gate and error-estimate figures
    Batch begin_batch(int kb) {
        Batch bt{kb, p.batch_begin(kb), p.batch_end(kb)};
        if (p.gated) {
            // fused: the batch's flag commits it (a word no kernel writes stands in for `aborted`)
            const int w = p.fused() ? kCtlFusedAborted : kCtlAborted + kb % p.ring;
            if (!p.fused()) ctl_store(sc->ctl, w, 0);   // batch kb - ring, the slot's last user, has completed
            bt.gate = reduce_gate(sc, w, bt.be, sc->home.gate_skip.p, p.fused() ? kb : -1);
        }
        bt.eb = ErrorBatch{err_active ? p.groups_after[kb] : 0, bt.be - p.base, kb % p.ring};
        return bt;
    }

    // a fused batch's reduce (and the estimate's launches) of the partials `src` on the home stream
    hipError_t reduce_fused(Batch& bt, const ImageParams& bi, const double* src) {
        // fused batches with running frames: RT_FUSED_PREVIEW=1 (A/B) the batch's reduce and its frame in one
        // kernel (reduce_preview_kernel) — measured slower: mesh50k 22 batches with running frames 77.6 vs
        // 76.1 ms kernel time for the two kernels (config 3: 96.0 vs 95.9), DESIGN.md §4
        const bool fuse_prev = render_knobs().fused_preview && p.preview && bt.be < p.s1 && thresholds;
        hipError_t e;
        if (!fuse_prev) e = launch_reduce(bi, h.sum.p, src, sc->tri_bvh, h.stream, bt.gp);
        else {
            e = launch_reduce_preview(bi, h.sum.p, src, sc->tri_bvh, h.stream, bt.gp, frame_params(bt.be),
                                      thresholds->table(), sc->preview_dev[bt.kb % p.ring]);
            if (e == hipSuccess) e = gamma_used(thresholds, h.stream);
            bt.previewed = e == hipSuccess;
        }
        if (e == hipSuccess && bt.ebp) e = error_after_reduce(sc, bt.eb, bi, src, bt.gp, h.stream);
        return e;
    }

    // Fused batches: every device's one launch of all its batches (device e: batches e, e + nsh, ...; all of
    // them when nsh = 1), before batch 0's reduce
    int launch_fused(const Batch& bt) {
        const int nsh = p.shards;
        const bool bvh = use_bvh(sc, s);
        for (int k = 0; k < p.nb; ++k) ctl_store(sc->ctl, kCtlFlag + k, 0);
        ctl_store(sc->ctl, kCtlFusedAborted, 0);
        ctl_store(sc->ctl, kCtlFusedAborted + 1, 0);
        for (int e = 0; e < nsh; ++e) {
            DeviceState& de = *states[e];
            HIP_TRY(hipSetDevice(de.device));
            const int nbe = (p.nb - e + nsh - 1) / nsh;
            HIP_TRY(hipMemsetAsync(de.fused_count.p, 0, nbe * sizeof(uint32_t), de.tstream[0]));
            Counters c = with_cancel(bt, cs[e]);
            c.aborted = sc->ctl_dev + kCtlFusedAborted + 1;   // written by skipping waves, read by no gate
            c.batch_count = de.fused_count.p;
            c.batch_flag = sc->ctl_dev + kCtlFlag + e;          // batch k = e + lb * nsh
            ImageParams fi = im;
            fi.s_begin = p.s0 + e * p.batch;
            fi.s_end = p.s1;
            fi.pool_chunk = p.fchunk;
            fi.batch_ways = nsh;
            const size_t fb = de.fused_part.n * sizeof(double);
            HIP_TRY(with_view(de, s->precision, [&](const auto& v) {
                return launch_trace_batches(v, fi, c, bvh, p.batch, de.fused_part.p, fb, de.tstream[0]);
            }));
            HIP_TRY(hipEventRecord(de.fused_done, de.tstream[0]));
        }
        fused_launched = true;
        return RT_OK;
    }

    // Fused batches: batch kb's reduce on the home stream once its flag is up — from the device's own fused
    // partials, or for a replica's batch from their copy on the home device
    int enqueue_fused(Batch& bt) {
        const int kb = bt.kb;
        if (kb == 0)
            if (int rc = launch_fused(bt)) return rc;
        const int d = kb % p.shards, lb = kb / p.shards;
        DeviceState& ds = *states[d];
        // the host waits for batch kb's flag; without it (a cancel: its items stay untraced) the
        // consumer stream waits for the device's launch to end, so the gate reads the final words
        for (;;) {
            if (ctl_load(sc->ctl, kCtlFlag + kb)) break;
            if (sc->cancel.load()) {          // (launches registered after rt_cancel's call, too)
                (void)cancel_pool_launches(sc->ctl_dev + kCtlCancel);
                break;
            }
            const hipError_t q = hipEventQuery(ds.fused_done);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) {      // a device fault, not a cancel: fail with the HIP error
                (void)hipGetLastError();
                return fail(RT_ERR_DEVICE, "fused batch %d: %s", kb, hipGetErrorString(q));
            }
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        const bool flagged = ctl_load(sc->ctl, kCtlFlag + kb) != 0;
        ImageParams bi = im;
        bi.s_begin = bt.b;
        bi.s_end = bt.be;
        bi.pool_chunk = p.fchunk;
        const double* src = ds.fused_part.p + (size_t)lb * p.fdoubles;
        if (&ds == &h) {
            HIP_TRY(hipSetDevice(h.device));
            if (!flagged) HIP_TRY(hipStreamWaitEvent(h.stream, h.fused_done, 0));
            HIP_TRY(reduce_fused(bt, bi, src));
            return RT_OK;
        }
        const size_t bytes = pool_plan(cw, ch, bt.be - bt.b, sc->tri_bvh, p.fchunk).part_bytes;
        return stage_and_reduce(
            sc, ds, sc->merge[d], lb % kSlots, ds.stream, src, bytes, p.fdoubles,
            [&] { return flagged ? hipSuccess : hipStreamWaitEvent(ds.stream, ds.fused_done, 0); },
            [&](const double* staged) { return reduce_fused(bt, bi, staged); });
    }

    // The whole batch on one device, reduced on the home device
    int enqueue_whole(const Batch& bt) {
        const RenderPlan::Piece q = p.piece(bt.kb, 0);
        const int k = q.shard, lj = bt.kb / p.shards, j = lj % kSlots;
        DeviceState& ds = *states[k];
        ImageParams bi = im;
        bi.s_begin = q.begin;
        bi.s_end = q.end;
        bi.pool_chunk = q.chunk;
        HIP_TRY(hipSetDevice(ds.device));
        slots_used[k] |= 1u << j;
        if (&ds == &sc->home) HIP_TRY(trace_overlapped(sc, ds, s, bi, with_cancel(bt, cs[k]), j, lj >= kSlots, bt.gp, bt.ebp));
        else return trace_replica(sc, ds, sc->merge[k], s, bi, with_cancel(bt, cs[k]), j, bt.gp, bt.ebp);
        return RT_OK;
    }

    // One device, or every batch split over the devices: every shard's launches first (the devices run
    // together), then the merge of the shards into the home device
    int enqueue_split(const Batch& bt) {
        const int kb = bt.kb;
        for (int k = 0; k < p.pieces(); ++k) {
            const RenderPlan::Piece q = p.piece(kb, k);
            DeviceState& ds = *states[k];
            ImageParams bi = im;
            bi.s_begin = q.begin;
            bi.s_end = q.end;
            bi.pool_chunk = q.chunk;
            HIP_TRY(hipSetDevice(ds.device));
            if (p.overlap())
                HIP_TRY(trace_overlapped(sc, ds, s, bi, with_cancel(bt, cs[k]), kb % kSlots, kb >= kSlots, bt.gp, bt.ebp));
            else {                                    // (the estimate: one device, launch_trace adds the chunk moments)
                HIP_TRY(trace(sc, ds, s, bi, cs[k], ds.stream, bt.ebp ? sc->err_q.p : nullptr));
                if (bt.ebp) HIP_TRY(error_after_reduce(sc, bt.eb, bi, nullptr, nullptr, ds.stream));
            }
        }
        return p.shards > 1 ? merge_shards(sc, states, n, want_segs, want_draws) : RT_OK;
    }

    // The running frame of the sums' first `done` samples (their mean) into ring slot `slot` on the home stream:
    // written by the epilogue kernel straight into pinned host memory (over PCIe): a hipMemcpyAsync here is a
    // blit kernel that waits for wave slots behind the trace waves (measured 7-15 ms per 8-MB frame while
    // batches overlap)
    int preview_frame(int done, int slot, bool by_thresholds) {
        const GammaTable* table = by_thresholds && thresholds ? thresholds->table() : nullptr;
        HIP_TRY(launch_finalize(frame_params(done), h.sum.p, nullptr, nullptr, sc->preview_dev[slot], h.stream, table));
        if (table) HIP_TRY(gamma_used(thresholds, h.stream));
        return RT_OK;
    }

    // enqueue batch kb (no host wait): every shard's trace, the merge of the shards into the home device,
    // the preview frame, then batch_done[kb % ring] on the home stream
    int enqueue_batch(int kb) {
        Batch bt = begin_batch(kb);
        bt.gp = p.gated ? &bt.gate : nullptr;
        bt.ebp = err_active ? &bt.eb : nullptr;
        int rc = p.fused() ? enqueue_fused(bt) : p.whole() ? enqueue_whole(bt) : enqueue_split(bt);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(sc->home.device));
        if (p.preview && bt.be < p.s1 && !bt.previewed && (rc = preview_frame(bt.be, kb % p.ring, true))) return rc;
        HIP_TRY(hipEventRecord(sc->batch_done[kb % p.ring], sc->home.stream));
        return RT_OK;
    }

    // enqueue batches [enqueued, upto).  The host keeps up to p.ahead batches queued beyond the one it waits
    // for (their ordering on the partial slots is device-side: trace_overlapped), so neither the host's progress
    // call nor a preview frame ever delays the start of a batch
    int fill_queue(int upto) {
        for (; enqueued < std::min(upto, p.nb) && !sc->cancel.load(); ++enqueued)
            if (int rc = enqueue_batch(enqueued)) return rc;
        return RT_OK;
    }

    // the error figures of committed batch kb, from its slot of the control words
    void commit_error_stats(int kb) {
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
        ErrorWords w;
        memcpy(&w, sc->ctl + kCtlErr + (kb % p.ring) * kErrSlotWords, sizeof w);
        rt_error_stats& st = sc->err_stats;
        st.samples = w.samples;
        st.groups = w.groups;
        st.chunk_samples = p.err_chunk;
        st.converged = ctl_load(sc->ctl, kCtlConverged) ? 1 : 0;
        st.pixels = w.pixels;
        st.nonfinite_pixels = w.nonfinite;
        st.frame_error = w.frame_error;
        st.max_error = w.max_error;
        sc->err_groups = w.groups;
        sc->err_samples = w.samples;
        sc->err_valid = true;
    }

    // host side of batch kb once batch_done: checkpoint state and the preview frame.  merged: the batch
    // is in the sums (gated renders: not if a cancel left it unfinished)
    int complete_batch(int kb, bool& merged) {
        HIP_TRY(hipEventSynchronize(sc->batch_done[kb % p.ring]));
        const int be = p.batch_end(kb);
        merged = !p.gated || (int)ctl_load(sc->ctl, kCtlDone) >= be;
        if (!merged) return RT_OK;
        sc->ckpt_done = be;
        if (err_active) commit_error_stats(kb);
        // the running frame, unless the next batch has finished too (its frame supersedes this one: the
        // host does not fall further behind the GPU copying frames nobody will see)
        if (p.preview && be < p.s1 &&
            !(kb + 1 < enqueued && hipEventQuery(sc->batch_done[(kb + 1) % p.ring]) == hipSuccess)) {
            memcpy(out->preview_rgba8, sc->preview_host[kb % p.ring], 4 * n);
            if (out->preview_samples) *out->preview_samples = be - p.base;
        }
        return RT_OK;
    }

    // A cancel, or the noise threshold's stop (conv), seen after batch kb: what the queued batches still do,
    // the checkpoint they leave and its frame.  status: RT_OK (the render completed after all, or stopped at
    // the threshold) or RT_ERR_CANCELLED; the return value: a HIP failure on the way
    int stop_render(int kb, bool conv, int& status) {
        if (p.gated) {
            // the queued batches stop at their next item and are not reduced; once every stream has
            // drained, the sums hold exactly the batches the gates committed
            ctl_cancel(sc->ctl, 1);
            (void)cancel_pool_launches(sc->ctl_dev + kCtlCancel);
            for (DeviceState* ds : states) ds->sync_all();
            h.sync_all();
            sc->ckpt_done = (int)ctl_load(sc->ctl, kCtlDone);
            if (err_active && sc->ckpt_done > p.s0) commit_error_stats((sc->ckpt_done - p.s0 + p.batch - 1) / p.batch - 1);
            if (p.preview && sc->ckpt_done > p.base && sc->ckpt_done < p.s1) {   // the checkpoint's frame
                HIP_TRY(hipSetDevice(h.device));
                if (int rc = preview_frame(sc->ckpt_done, 0, false)) return rc;
                HIP_TRY(hipStreamSynchronize(h.stream));
                memcpy(out->preview_rgba8, sc->preview_host[0], 4 * n);
                if (out->preview_samples) *out->preview_samples = sc->ckpt_done - p.base;
            }
        } else {
            // the batches in flight finish (and if the last one was among them, the render completed)
            bool merged = true;
            for (int k = kb + 1; k < enqueued && status == RT_OK; ++k) status = complete_batch(k, merged);
        }
        if (status == RT_OK && sc->ckpt_done < p.s1) {
            if (conv && !sc->cancel.load() && sc->ckpt_done > p.base) stopped = true;   // RT_OK over the samples done
            else status = fail(RT_ERR_CANCELLED, "render cancelled after %d samples", sc->ckpt_done);
        }
        return RT_OK;
    }

    // a HIP error inside the pipeline: drain every stream; the checkpoint keeps the last batch whose
    // merge is known to be complete (complete_batch ran for it), and the scratch is released
    void drain_after_error() {
        const std::string err = g_error;
        for (DeviceState* ds : states) {
            ds->sync_all();
            (void)release_scratch(*ds, ds->stream);
        }
        sc->home.sync_all();
        (void)hipGetLastError();
        g_error = err;
    }

    // After the batches (all of them, or those a cancel or the threshold left): the counters' merge, the work
    // totals, then — unless cancelled (status) — the epilogue, the outputs' copies and the statistics
    int finish_render(int status, rt_stats* stats, double t_start) {
        if (fused_launched)                         // every launch's last waves (counters, work totals) first
            for (DeviceState* ds : states) {
                HIP_TRY(hipSetDevice(ds->device));
                HIP_TRY(hipStreamWaitEvent(ds->stream, ds->fused_done, 0));
            }
        if (p.whole()) {   // every device's accumulation stream after its trace streams; the replicas' counters
            for (size_t k = 0; k < states.size(); ++k) {
                DeviceState* ds = states[k];
                HIP_TRY(hipSetDevice(ds->device));
                for (int j = 0; j < kSlots; ++j)
                    if (slots_used[k] & (1u << j)) HIP_TRY(hipStreamWaitEvent(ds->stream, ds->traced[j], 0));
            }
            if (int rc = merge_counters(sc, states, n, want_segs, want_draws)) return rc;
        }
        unsigned long long totals[kTotalSlots] = {};
        float kernel_ms = 0;
        for (DeviceState* ds : states) {
            unsigned long long t[kTotalSlots] = {};
            HIP_TRY(hipSetDevice(ds->device));
            HIP_TRY(hipEventRecord(ds->ev[1], ds->stream));
            HIP_TRY(hipMemcpyAsync(t, ds->total.p, sizeof t, hipMemcpyDeviceToHost, ds->stream));
            HIP_TRY(release_scratch(*ds, ds->stream));
            HIP_TRY(hipStreamSynchronize(ds->stream));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ds->ev[0], ds->ev[1]));
            kernel_ms = std::max(kernel_ms, ms);
            for (int k = 0; k < kTotalSlots; ++k) totals[k] += t[k];
        }
        HIP_TRY(hipSetDevice(h.device));
        HIP_TRY(hipStreamSynchronize(h.stream));          // the merges of the last batch (checkpoint state)
        if (status != RT_OK) return status;
        if (stopped) {                              // the epilogue and the statistics over the samples committed
            settings.samples = sc->ckpt_done - p.base;
            im.s_end = sc->ckpt_done;
        }
        const bool want_mean = out && out->mean, want_post = out && out->post, want_rgba = out && out->rgba8;
        if (want_mean) HIP_TRY(sc->mean.ensure(3 * n));
        if (want_post) HIP_TRY(sc->post.ensure(4 * n));
        if (want_rgba) HIP_TRY(sc->rgba.ensure(4 * n));
        HIP_TRY(hipEventRecord(sc->ev[0], h.stream));
        HIP_TRY(epilogue(sc, s, cw, ch, h.sum.p, want_mean ? sc->mean.p : nullptr, want_post ? sc->post.p : nullptr,
                         want_rgba ? sc->rgba.p : nullptr, h.stream));
        HIP_TRY(hipEventRecord(sc->ev[1], h.stream));
        if (want_mean) HIP_TRY(hipMemcpyAsync(out->mean, sc->mean.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, h.stream));
        if (want_post) HIP_TRY(hipMemcpyAsync(out->post, sc->post.p, 4 * n * sizeof(float), hipMemcpyDeviceToHost, h.stream));
        if (want_rgba) HIP_TRY(hipMemcpyAsync(out->rgba8, sc->rgba.p, 4 * n, hipMemcpyDeviceToHost, h.stream));
        if (want_segs) HIP_TRY(hipMemcpyAsync(out->segments, h.segs.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h.stream));
        if (want_draws) HIP_TRY(hipMemcpyAsync(out->draws, h.draws.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h.stream));
        HIP_TRY(hipStreamSynchronize(h.stream));
        if (stats) {
            float fms = 0;
            HIP_TRY(hipEventElapsedTime(&fms, sc->ev[0], sc->ev[1]));
            stats->kernel_ms = kernel_ms;
            stats->finalize_ms = fms;
            fill_stats(stats, sc, s, totals, n, im);
            stats->wall_ms = now_ms() - t_start;
        }
#if RT_PROFILE
        const double cyc = (double)(totals[4] + totals[5] + totals[6]);
        fprintf(stderr, "[rt_profile] wave-max cycles: closest hit %.3f, shading %.3f, regeneration %.3f (%.3e total); "
                "walk iterations: %.3e per lane, %.3e per wave, lane efficiency %.3f, wave-uniform inner-node share %.3f\n",
                totals[4] / cyc, totals[5] / cyc, totals[6] / cyc, cyc, (double)totals[7], (double)totals[8],
                totals[8] ? (double)totals[7] / (64.0 * (double)totals[8]) : 0.0,
                totals[8] ? (double)totals[9] / (double)totals[8] : 0.0);
        fprintf(stderr, "[rt_profile] wave walk iterations with <= 8 lanes walking %.3f, <= 16 %.3f\n",
                totals[8] ? (double)totals[10] / (double)totals[8] : 0.0, totals[8] ? (double)totals[11] / (double)totals[8] : 0.0);
#endif
        return RT_OK;
    }
};

// rt_render and rt_render_resume: trace samples [first, sample_end) on top of `sums_in` (render_plan.h)
int render_impl(rt_scene* sc, const rt_settings* s_in, const rt_output* out, rt_progress_fn progress, void* user,
                rt_stats* stats, const double* sums_in, int first, bool resident = false) {
    const double t_start = now_ms();
    int cw, ch;
    int rc = check_render(sc, s_in, sums_in, &cw, &ch);
    if (rc) return rc;
    RenderRun r(sc, *s_in, out, sums_in, resident, cw, ch);
    if ((rc = shard_states(sc, r.s, r.states))) return rc;
    // no checkpoint from here until the new sums are consistent (set by prepare_devices, with the samples
    // they hold): a render that fails in between leaves none, rather than old metadata over overwritten sums
    sc->ckpt_pixels = 0;
    sc->cancel.store(0);
    ctl_cancel(sc->ctl, 0);
    // this render's LDS pool launches are registered under its cancel word until it returns
    struct LaunchScope {
        const uint32_t* word;
        ~LaunchScope() { forget_pool_launches(word); }
    } launch_scope{sc->ctl_dev + kCtlCancel};
    if (++sc->render_gen == 0) sc->render_gen = 1;   // 0 is the words' initial value
    for (DeviceState* ds : r.states) register_cancel_word(sc->ctl_dev + kCtlCancel, ds->device, ds->cancel_word.p, sc->render_gen);
    if ((rc = r.make_plan(first)) || (rc = r.prepare_devices())) return rc;
    const RenderPlan& p = r.p;
    int status = RT_OK;
    for (int kb = 0; kb < p.nb && status == RT_OK; ++kb) {
        if ((status = r.fill_queue(kb + (p.fused() ? 0 : p.ahead) + 1))) break;   // fused: enqueue_fused(kb) waits for batch kb
        bool merged = true;
        if ((status = r.complete_batch(kb, merged))) break;
        // the threshold stop (error_frame_kernel set `stop` and `converged` after an earlier batch): the gates
        // skip every later batch, and nobody cancelled
        const bool conv = r.err_active && p.gated && ctl_load(sc->ctl, kCtlConverged) != 0;
        if (!merged && !sc->cancel.load() && !conv) {
            // a gate skipped a batch although nobody cancelled (rt_cancel sets `cancel` before the word the
            // kernels read): an item-count mismatch or a lost flag — an internal failure, not a cancel
            status = fail(RT_ERR_DEVICE, "batch %d was not committed (internal error)", kb);
            break;
        }
        const int be = sc->ckpt_done;
        if (merged && progress && be < p.s1 && progress((double)(be - p.s0) / (double)(p.s1 - p.s0), user)) {
            sc->cancel.store(1);
            ctl_cancel(sc->ctl, 1);
        }
        if (!merged || sc->cancel.load() || (conv && be < p.s1)) {
            if ((rc = r.stop_render(kb, conv, status))) return rc;
            break;
        }
    }
    if (status != RT_OK && status != RT_ERR_CANCELLED) {
        r.drain_after_error();
        return status;
    }
    return r.finish_render(status, stats, t_start);
}

}  // namespace

extern "C" {

int rt_render(rt_scene* sc, const rt_settings* s, const rt_output* out, rt_progress_fn progress, void* user,
              rt_stats* stats) {
    return render_impl(sc, s, out, progress, user, stats, nullptr, 0);
}

int rt_render_checkpoint(rt_scene* sc, double* sums, size_t count, int32_t* samples_done) {
    if (!sc || !samples_done) return fail(RT_ERR_INVALID, "NULL argument");
    if (sc->ckpt_pixels == 0) return fail(RT_ERR_INVALID, "no render to checkpoint");
    if (!sums && count == 0) {                     // samples_done only (the sums stay on the device)
        *samples_done = sc->ckpt_done;
        return RT_OK;
    }
    if (!sums) return fail(RT_ERR_INVALID, "NULL argument");
    if (count != 3 * sc->ckpt_pixels)
        return fail(RT_ERR_INVALID, "checkpoint holds %zu doubles, caller gave %zu", 3 * sc->ckpt_pixels, count);
    HIP_TRY(hipSetDevice(sc->home.device));
    HIP_TRY(hipMemcpyAsync(sums, sc->home.sum.p, count * sizeof(double), hipMemcpyDeviceToHost, sc->home.stream));
    HIP_TRY(hipStreamSynchronize(sc->home.stream));
    *samples_done = sc->ckpt_done;
    return RT_OK;
}

int rt_render_resume(rt_scene* sc, const rt_settings* s, const double* sums, int32_t samples_done,
                     const rt_output* out, rt_progress_fn progress, void* user, rt_stats* stats) {
    if (s && (samples_done < std::max(0, s->sample_begin) || samples_done > s->samples))
        return fail(RT_ERR_INVALID, "samples_done %d outside [sample_begin, samples]", samples_done);
    if (!sums) {                                   // from the scene's own checkpoint, still on its device
        int cw = 0, ch = 0;
        if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
        if (int rc = check_settings(s, &cw, &ch)) return rc;
        if (sc->ckpt_pixels == 0 || sc->ckpt_pixels != (size_t)cw * ch || samples_done != sc->ckpt_done)
            return fail(RT_ERR_INVALID, "no resident checkpoint of %d samples over %d x %d pixels (sums NULL)",
                        samples_done, cw, ch);
        if (!(sc->ckpt_key == ckpt_key(s, cw, ch)))
            return fail(RT_ERR_INVALID, "the resident checkpoint is of another frame, crop, sample_begin, precision, "
                        "seed, aa_mode or max_depth (sums NULL)");
        return render_impl(sc, s, out, progress, user, stats, nullptr, samples_done, true);
    }
    return render_impl(sc, s, out, progress, user, stats, sums, samples_done);
}

int rt_trace_device(rt_scene* sc, const rt_settings* s, double* d_sum, void* hip_stream, int sync, rt_stats* stats) {
    const double t_start = now_ms();
    if (!sc || !d_sum) return fail(RT_ERR_INVALID, "NULL argument");
    int cw, ch;
    int rc = check_settings(s, &cw, &ch);
    if (!rc) rc = check_accel(sc, s);
    if (rc) return rc;
    if (s->device_count > 1)
        return fail(RT_ERR_INVALID, "rt_trace_device traces on the scene's device (device_count %d): split the "
                    "samples over processes, or use rt_render", s->device_count);
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    // NULL is the default (null) stream, as for rt_finalize_device: the caller's zeroing of d_sum and
    // its reduce / epilogue on that stream are ordered with this trace (the scene's own non-blocking
    // stream would not be: a zeroing enqueued on the default stream could run after the trace's
    // reduce pass)
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(ds.total.ensure(kTotalSlots));
    ImageParams im = image_params(s, cw, ch);
    Counters c{d_sum, nullptr, nullptr, ds.total.p};
    if (s->max_depth > 0 && (rc = ensure_partials(sc, ds, cw, ch, im.s_end - im.s_begin, use_pool(s), c))) return rc;
    HIP_TRY(order_scratch(ds, st));
    HIP_TRY(hipMemsetAsync(ds.total.p, 0, kTotalSlots * sizeof(unsigned long long), st));
    HIP_TRY(hipEventRecord(ds.ev[0], st));
    HIP_TRY(trace(sc, ds, s, im, c, st));
    HIP_TRY(hipEventRecord(ds.ev[1], st));
    unsigned long long totals[kTotalSlots] = {};
    if (sync || stats) HIP_TRY(hipMemcpyAsync(totals, ds.total.p, sizeof totals, hipMemcpyDeviceToHost, st));
    HIP_TRY(release_scratch(ds, st));
    if (sync || stats) {
        HIP_TRY(hipStreamSynchronize(st));
        if (stats) return trace_stats(stats, sc, s, ds, totals, (size_t)cw * ch, im, t_start);
    }
    return RT_OK;
}

int rt_trace_device_bands(rt_scene* sc, const rt_settings* s, double* d_sum, void* hip_stream, int32_t bands,
                          rt_band_fn band_ready, void* user, rt_stats* stats) {
    const double t_start = now_ms();
    if (!sc || !d_sum) return fail(RT_ERR_INVALID, "NULL argument");
    int cw, ch;
    int rc = check_settings(s, &cw, &ch);
    if (!rc) rc = check_accel(sc, s);
    if (rc) return rc;
    if (s->device_count > 1) return fail(RT_ERR_INVALID, "rt_trace_device_bands traces on the scene's device");
    const int tile_rows = (ch + 7) / 8;
    const int nb = std::max(1, std::min({(int)bands, tile_rows, kMaxFused}));
    ImageParams im = image_params(s, cw, ch);
    auto deliver_all = [&](int from) -> int {   // bands [from, nb) at once (nothing left to overlap)
        for (int b = from; b < nb && band_ready; ++b) {
            im.bands = nb;
            const int r0 = band_row0(im, b) * 8, r1 = std::min(ch, band_row0(im, b + 1) * 8);
            if (band_ready(b, r0, r1 - r0, user)) return fail(RT_ERR_CANCELLED, "band_ready stopped at band %d", b);
        }
        return RT_OK;
    };
    // no pool (sample order) or nothing to trace: rt_trace_device, then every band
    if (!use_pool(s) || s->max_depth <= 0 || im.s_end <= im.s_begin) {
        if ((rc = rt_trace_device(sc, s, d_sum, hip_stream, 0, stats))) return rc;
        return deliver_all(0);
    }
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    hipStream_t st = (hipStream_t)hip_stream;
    const PoolPlan plan = pool_plan(cw, ch, im.s_end - im.s_begin, sc->tri_bvh, 0);
    HIP_TRY(ds.total.ensure(kTotalSlots));
    HIP_TRY(ds.fused_count.ensure((size_t)nb));
    HIP_TRY(ds.gate_skip.ensure(1));
    if (ds.part.n * sizeof(double) < plan.part_bytes) {     // every chunk's partials (even one chunk)
        HIP_TRY(scratch_idle(ds));
        HIP_TRY(ds.part.ensure(plan.part_bytes / sizeof(double)));
    }
    // the control words are reset from the host: the gates of the scratch's last user (the last bands of an
    // earlier call that returned without a host synchronization) must have read theirs first, or such a gate
    // finds its flag cleared, skips its band and leaves `stop` set for every band of this call
    HIP_TRY(scratch_idle(ds));
    HIP_TRY(order_scratch(ds, st));
    for (int b = 0; b < nb; ++b) ctl_store(sc->ctl, kCtlFlag + b, 0);
    ctl_store(sc->ctl, kCtlStop, 0);
    ctl_store(sc->ctl, kCtlFusedAborted, 0);
    // the trace runs on the scene's own trace stream, after the caller's work so far (d_sum's zeroing);
    // the band reduces run on the caller's stream as the bands complete, beside the trace
    hipStream_t ts = ds.tstream[0];
    HIP_TRY(hipMemsetAsync(ds.total.p, 0, kTotalSlots * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(ds.fused_count.p, 0, (size_t)nb * sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(ds.setup_ev, st));
    HIP_TRY(hipStreamWaitEvent(ts, ds.setup_ev, 0));
    Counters c{d_sum, nullptr, nullptr, ds.total.p};
    c.batch_count = ds.fused_count.p;
    c.batch_flag = sc->ctl_dev + kCtlFlag;
    const bool bvh = use_bvh(sc, s);
    PoolPlan used{};
    HIP_TRY(hipEventRecord(ds.ev[0], ts));
    HIP_TRY(with_view(ds, s->precision, [&](const auto& v) {
        return launch_trace_bands(v, im, c, bvh, nb, ds.part.p, ds.part.n * sizeof(double), &used, ts);
    }));
    HIP_TRY(hipEventRecord(ds.ev[1], ts));
    HIP_TRY(hipEventRecord(ds.fused_done, ts));
    im.bands = nb;
    im.band_chunks = used.chunks;
    im.pool_chunk = used.chunk;
    const int tiles_x = (cw + 7) / 8;
    int status = RT_OK;
    for (int b = 0; b < nb && status == RT_OK; ++b) {
        for (;;) {                                  // band b's items are all done
            if (ctl_load(sc->ctl, kCtlFlag + b)) break;
            const hipError_t q = hipEventQuery(ds.fused_done);
            if (q == hipSuccess) {
                if (!ctl_load(sc->ctl, kCtlFlag + b)) status = fail(RT_ERR_DEVICE, "band %d was not completed (internal error)", b);
                break;
            }
            if (q != hipErrorNotReady) {
                (void)hipGetLastError();
                status = fail(RT_ERR_DEVICE, "band %d: %s", b, hipGetErrorString(q));
                break;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        if (status != RT_OK) break;
        const ReduceGate gate = reduce_gate(sc, kCtlFusedAborted, 0, ds.gate_skip.p, b);   // the acquire end of the band's commit (item_done)
        const int r0 = band_row0(im, b), r1 = band_row0(im, b + 1);
        hipError_t e = launch_reduce_tiles(im, d_sum, ds.part.p, used.tiles, used.chunks, r0 * tiles_x,
                                           (r1 - r0) * tiles_x, st, &gate);
        if (e != hipSuccess) { status = fail(RT_ERR_DEVICE, "band reduce: %s", hipGetErrorString(e)); break; }
        if (band_ready && band_ready(b, r0 * 8, std::min(ch, r1 * 8) - r0 * 8, user))
            status = fail(RT_ERR_CANCELLED, "band_ready stopped at band %d", b);
    }
    // the caller's stream after the whole launch (work totals, and the scratch's next user)
    HIP_TRY(hipStreamWaitEvent(st, ds.fused_done, 0));
    unsigned long long totals[kTotalSlots] = {};
    if (stats) HIP_TRY(hipMemcpyAsync(totals, ds.total.p, sizeof totals, hipMemcpyDeviceToHost, st));
    HIP_TRY(release_scratch(ds, st));
    if (status != RT_OK) {
        const std::string err = g_error;
        (void)hipStreamSynchronize(st);
        g_error = err;
        return status;
    }
    if (stats) {
        HIP_TRY(hipStreamSynchronize(st));
        return trace_stats(stats, sc, s, ds, totals, (size_t)cw * ch, im, t_start);
    }
    return RT_OK;
}

int rt_scene_walk(rt_scene* sc, int32_t precision, int32_t accel) {
    if (!sc) return fail(RT_ERR_INVALID, "NULL argument");
    if (precision != RT_PREC_F64 && precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", precision);
    rt_settings s{};
    s.accel = accel;
    if (s.accel < RT_ACCEL_AUTO || s.accel > RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "accel %d", accel);
    const int rc = check_accel(sc, &s);
    if (rc) return rc;
    if (!use_bvh(sc, &s)) return 0;
    const bool grid = with_view(sc->home, precision, [](const auto& v) { return trace_walks_grid(v); });
    return grid ? 2 : 1;
}

int rt_closest_hits(rt_scene* sc, int32_t precision, int32_t accel, const double* rays, size_t n, double* t,
                    int32_t* kind, int32_t* index) {
    if (!sc || (n > 0 && !rays)) return fail(RT_ERR_INVALID, "NULL argument");
    if (precision != RT_PREC_F64 && precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", precision);
    rt_settings s{};
    s.accel = accel;
    if (s.accel < RT_ACCEL_AUTO || s.accel > RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "accel %d", accel);
    int rc = check_accel(sc, &s);
    if (rc) return rc;
    if (n == 0) return RT_OK;
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    DevBuf<double> d_rays, d_t;
    DevBuf<int> d_kind, d_idx;
    auto cleanup = [&] { d_rays.release(); d_t.release(); d_kind.release(); d_idx.release(); };
    hipError_t e = d_rays.ensure(6 * n);
    if (e == hipSuccess) e = d_t.ensure(n);
    if (e == hipSuccess) e = d_kind.ensure(n);
    if (e == hipSuccess) e = d_idx.ensure(n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays.p, rays, 6 * n * sizeof(double), hipMemcpyHostToDevice, ds.stream);
    const bool bvh = use_bvh(sc, &s);
    if (e == hipSuccess)
        e = with_view(ds, precision, [&](const auto& v) {
            return launch_closest_hits(v, bvh, d_rays.p, n, d_t.p, d_kind.p, d_idx.p, ds.stream);
        });
    if (e == hipSuccess && t) e = hipMemcpyAsync(t, d_t.p, n * sizeof(double), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && kind) e = hipMemcpyAsync(kind, d_kind.p, n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && index) e = hipMemcpyAsync(index, d_idx.p, n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    cleanup();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_closest_hits: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_hit_records(rt_scene* sc, int32_t precision, int32_t accel, const double* rays, size_t n, double* t, int32_t* kind,
                   int32_t* index, double* point, double* normal, uint8_t* front, int32_t* mat) {
    if (!sc || (n > 0 && !rays)) return fail(RT_ERR_INVALID, "NULL argument");
    if (precision != RT_PREC_F64 && precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", precision);
    rt_settings s{};
    s.accel = accel;
    if (s.accel < RT_ACCEL_AUTO || s.accel > RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "accel %d", accel);
    int rc = check_accel(sc, &s);
    if (rc) return rc;
    if (n == 0) return RT_OK;
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    DevBuf<double> d_rays, d_t, d_rec;
    DevBuf<int> d_kind, d_idx, d_mat;
    DevBuf<uint8_t> d_front;
    hipError_t e = d_rays.ensure(6 * n);
    if (e == hipSuccess) e = d_t.ensure(n);
    if (e == hipSuccess) e = d_rec.ensure(6 * n);
    if (e == hipSuccess) e = d_kind.ensure(n);
    if (e == hipSuccess) e = d_idx.ensure(n);
    if (e == hipSuccess) e = d_mat.ensure(n);
    if (e == hipSuccess) e = d_front.ensure(n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays.p, rays, 6 * n * sizeof(double), hipMemcpyHostToDevice, ds.stream);
    const bool bvh = use_bvh(sc, &s);
    if (e == hipSuccess)
        e = with_view(ds, precision, [&](const auto& v) {
            return launch_hit_records(v, bvh, d_rays.p, n, d_t.p, d_kind.p, d_idx.p, d_rec.p, d_front.p, d_mat.p, ds.stream);
        });
    // the device rows are point then normal; the host gets them as two n x 3 arrays
    std::vector<double> rec(point || normal ? 6 * n : 0);
    if (e == hipSuccess && t) e = hipMemcpyAsync(t, d_t.p, n * sizeof(double), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && kind) e = hipMemcpyAsync(kind, d_kind.p, n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && index) e = hipMemcpyAsync(index, d_idx.p, n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && mat) e = hipMemcpyAsync(mat, d_mat.p, n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && front) e = hipMemcpyAsync(front, d_front.p, n, hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && !rec.empty())
        e = hipMemcpyAsync(rec.data(), d_rec.p, 6 * n * sizeof(double), hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    d_rays.release(); d_t.release(); d_rec.release(); d_kind.release(); d_idx.release(); d_mat.release(); d_front.release();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_hit_records: %s", hipGetErrorString(e));
    for (size_t r = 0; r < n && !rec.empty(); ++r)
        for (int k = 0; k < 3; ++k) {
            if (point) point[3 * r + k] = rec[6 * r + k];
            if (normal) normal[3 * r + k] = rec[6 * r + 3 + k];
        }
    return RT_OK;
}

int rt_shade_segments(rt_scene* sc, int32_t precision, int32_t accel, int32_t variant, const double* rays,
                      const uint32_t* keys, int32_t depth, size_t n, double* out_f, int32_t* out_i) {
    if (!sc || (n > 0 && (!rays || !keys))) return fail(RT_ERR_INVALID, "NULL argument");
    if (precision != RT_PREC_F64 && precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", precision);
    if (variant < 0 || variant >= kShadeVariants) return fail(RT_ERR_INVALID, "variant %d", variant);
    rt_settings s{};
    s.accel = accel;
    if (s.accel < RT_ACCEL_AUTO || s.accel > RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "accel %d", accel);
    int rc = check_accel(sc, &s);
    if (rc) return rc;
    DeviceState& ds = sc->home;
    // what the variant's feature set compiled out (the lean kernels' conditions, kernel_select.h) must not be there
    const char* missing = with_view(ds, precision, [&](const auto& v) -> const char* {
        if (v.num_tex > 0) return "procedural textures";
        if (variant == 0) return nullptr;
        if (v.background != RT_BG_GRADIENT) return "a background other than the gradient";
        if (v.num_boxes > 0) return "boxes";
        if (variant == 2 && (v.num_planes > 0 || sc->desc.d.num_triangles > 0)) return "planes or triangles";
        return nullptr;
    });
    if (missing) return fail(RT_ERR_INVALID, "rt_shade_segments: the scene has %s, which variant %d leaves out", missing, variant);
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(ds.device));
    DevBuf<double> d_rays, d_f;
    DevBuf<uint32_t> d_keys;
    DevBuf<int> d_i;
    hipError_t e = d_rays.ensure(6 * n);
    if (e == hipSuccess) e = d_keys.ensure(2 * n);
    if (e == hipSuccess) e = d_f.ensure(12 * n);
    if (e == hipSuccess) e = d_i.ensure(4 * n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays.p, rays, 6 * n * sizeof(double), hipMemcpyHostToDevice, ds.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_keys.p, keys, 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice, ds.stream);
    const bool bvh = use_bvh(sc, &s);
    if (e == hipSuccess)
        e = with_view(ds, precision, [&](const auto& v) {
            return launch_shade_segments(v, bvh, variant, d_rays.p, d_keys.p, depth, n, d_f.p, d_i.p, ds.stream);
        });
    if (e == hipSuccess && out_f) e = hipMemcpyAsync(out_f, d_f.p, 12 * n * sizeof(double), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && out_i) e = hipMemcpyAsync(out_i, d_i.p, 4 * n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    d_rays.release(); d_keys.release(); d_f.release(); d_i.release();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_shade_segments: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_camera_rays(rt_scene* sc, const rt_settings* s, int32_t variant, const int32_t* pixels, size_t n, double* out,
                   uint32_t* draws) {
    if (!sc || (n > 0 && !pixels)) return fail(RT_ERR_INVALID, "NULL argument");
    int cw, ch;
    const int rc = check_settings(s, &cw, &ch);
    if (rc) return rc;
    if (variant < 0 || variant >= kCameraVariants) return fail(RT_ERR_INVALID, "variant %d", variant);
    if ((variant & 2) && (sc->desc.d.camera.type != RT_CAM_PERSPECTIVE || s->aa_mode != RT_AA_SUPERSAMPLING))
        return fail(RT_ERR_INVALID, "rt_camera_rays: variant %d is the lean kernels' (perspective camera, supersampling)", variant);
    for (size_t r = 0; r < n; ++r)
        if (pixels[3 * r] < 0 || pixels[3 * r] >= s->width || pixels[3 * r + 1] < 0 || pixels[3 * r + 1] >= s->height ||
            pixels[3 * r + 2] < 0)
            return fail(RT_ERR_INVALID, "pixels[%zu] = (%d, %d, %d) outside %dx%d", r, pixels[3 * r], pixels[3 * r + 1],
                        pixels[3 * r + 2], s->width, s->height);
    if (n == 0) return RT_OK;
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    const ImageParams im = image_params(s, cw, ch);
    DevBuf<int> d_pix;
    DevBuf<double> d_out;
    DevBuf<uint32_t> d_draws;
    hipError_t e = d_pix.ensure(3 * n);
    if (e == hipSuccess) e = d_out.ensure(6 * n);
    if (e == hipSuccess) e = d_draws.ensure(n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pix.p, pixels, 3 * n * sizeof(int), hipMemcpyHostToDevice, ds.stream);
    if (e == hipSuccess)
        e = with_view(ds, s->precision, [&](const auto& v) {
            return launch_camera_rays(v, im, variant, d_pix.p, n, d_out.p, d_draws.p, ds.stream);
        });
    if (e == hipSuccess && out) e = hipMemcpyAsync(out, d_out.p, 6 * n * sizeof(double), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && draws) e = hipMemcpyAsync(draws, d_draws.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    d_pix.release(); d_out.release(); d_draws.release();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_camera_rays: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_occluded(rt_scene* sc, int32_t precision, int32_t accel, const double* rays, const double* tmax, size_t n,
                uint8_t* out) {
    if (!sc || (n > 0 && (!rays || !tmax || !out))) return fail(RT_ERR_INVALID, "NULL argument");
    if (precision != RT_PREC_F64 && precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", precision);
    rt_settings s{};
    s.accel = accel;
    if (s.accel < RT_ACCEL_AUTO || s.accel > RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "accel %d", accel);
    int rc = check_accel(sc, &s);
    if (rc) return rc;
    if (n == 0) return RT_OK;
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    DevBuf<double> d_rays, d_tmax;
    DevBuf<uint8_t> d_out;
    hipError_t e = d_rays.ensure(6 * n);
    if (e == hipSuccess) e = d_tmax.ensure(n);
    if (e == hipSuccess) e = d_out.ensure(n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays.p, rays, 6 * n * sizeof(double), hipMemcpyHostToDevice, ds.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmax.p, tmax, n * sizeof(double), hipMemcpyHostToDevice, ds.stream);
    const bool bvh = use_bvh(sc, &s);
    if (e == hipSuccess)
        e = with_view(ds, precision, [&](const auto& v) {
            return launch_occluded(v, bvh, d_rays.p, d_tmax.p, n, d_out.p, ds.stream);
        });
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out.p, n, hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    d_rays.release(); d_tmax.release(); d_out.release();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_occluded: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_texture_values(rt_scene* sc, int32_t precision, int32_t texture, const double* points, size_t n, double* rgb) {
    if (!sc || (n > 0 && (!points || !rgb))) return fail(RT_ERR_INVALID, "NULL argument");
    if (precision != RT_PREC_F64 && precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", precision);
    if (texture < 0 || texture >= sc->desc.d.num_textures)
        return fail(RT_ERR_INVALID, "texture %d of %d", texture, sc->desc.d.num_textures);
    if (!scene_textured(sc->desc.d)) return fail(RT_ERR_INVALID, "no material of the scene uses a texture");
    if (n == 0) return RT_OK;
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    DevBuf<double> d_pts, d_rgb;
    hipError_t e = d_pts.ensure(3 * n);
    if (e == hipSuccess) e = d_rgb.ensure(3 * n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pts.p, points, 3 * n * sizeof(double), hipMemcpyHostToDevice, ds.stream);
    if (e == hipSuccess)
        e = with_view(ds, precision, [&](const auto& v) {
            return launch_texture_values(v, texture, d_pts.p, n, d_rgb.p, ds.stream);
        });
    if (e == hipSuccess) e = hipMemcpyAsync(rgb, d_rgb.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    d_pts.release();
    d_rgb.release();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_texture_values: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_finalize_device(rt_scene* sc, const rt_settings* s, const double* d_sum, double* d_mean, float* d_post,
                       uint8_t* d_rgba8, void* hip_stream) {
    if (!sc || !d_sum) return fail(RT_ERR_INVALID, "NULL argument");
    int cw, ch;
    int rc = check_settings(s, &cw, &ch);
    if (!rc) rc = check_guided(sc, s, cw, ch);
    if (!rc && sc->gvar_sigma > 0.0)
        rc = fail(RT_ERR_INVALID, "rt_finalize_device has no error estimate (rt_trace_device produces none): switch the "
                  "variance-guided form off");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(sc->home.device));
    HIP_TRY(epilogue(sc, s, cw, ch, d_sum, d_mean, d_post, d_rgba8, (hipStream_t)hip_stream, true));
    return RT_OK;
}

int rt_scene_set_guided(rt_scene* sc, const rt_guided_params* p) {
    // the parameters first: a bad set is RT_ERR_INVALID with or without a device (or a scene)
    if (p && (p->levels < 1 || p->levels > RT_GUIDED_MAX_LEVELS))
        return fail(RT_ERR_INVALID, "guided levels %d (1 .. %d)", p->levels, RT_GUIDED_MAX_LEVELS);
    if (p && !guided_params_ok(p))
        return fail(RT_ERR_INVALID, "guided sigmas (%g, %g, %g, %g): each must be > 0", p->sigma_color, p->sigma_albedo,
                    p->sigma_normal, p->sigma_depth);
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    sc->guided_on = p != nullptr;
    if (p) sc->guided = *p;
    return RT_OK;
}

int rt_scene_set_emitter_sampling(rt_scene* sc, int32_t on) {
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    const bool was = sc->emitter_sampling;
    const std::vector<int> kind0 = sc->hs.emit_kind, idx0 = sc->hs.emit_idx;
    std::string err;
    if (!build_emitters(sc->hs, sc->desc.d, on != 0, err)) {
        sc->emitter_sampling = false;
        if (!kind0.empty()) (void)rt_scene_set_emitter_sampling(sc, 0);     // off: the plain records again
        return fail(RT_ERR_INVALID, "%s", err.c_str());
    }
    sc->emitter_sampling = on != 0;
    if (was == sc->emitter_sampling && kind0 == sc->hs.emit_kind && idx0 == sc->hs.emit_idx) return RT_OK;
    if (kind0.empty() && sc->hs.emit_idx.empty()) return RT_OK;             // no emitter either way: nothing moves
    // the records of every device that holds the scene, with or without the emitter list (the arrays in place:
    // DevBuf::ensure keeps a buffer that is large enough); what the sums on the device were is no longer what a
    // render would add to
    std::vector<DeviceState*> all{&sc->home};
    for (DeviceState* r : sc->replicas)
        if (r) all.push_back(r);
    for (DeviceState* ds : all) {
        ds->sync_all();
        HIP_TRY(hipSetDevice(ds->device));
        int rc;
        if ((rc = build_device(ds->s64, sc->hs, sc->desc.d)) || (rc = build_device(ds->s32, sc->hs, sc->desc.d))) return rc;
    }
    sc->ckpt_pixels = 0;
    sc->ckpt_done = 0;
    return RT_OK;
}

int rt_scene_emitter_count(rt_scene* sc, int32_t* count) {
    if (!sc || !count) return fail(RT_ERR_INVALID, "NULL argument");
    *count = (int32_t)sc->hs.emit_idx.size();
    return RT_OK;
}

int rt_emitter_samples(rt_scene* sc, int32_t precision, int32_t accel, const double* points, const uint32_t* keys,
                       size_t n, int32_t* emitter, double* omega, double* p_l, double* t_e, uint8_t* visible) {
    if (!sc || (n > 0 && (!points || !keys))) return fail(RT_ERR_INVALID, "NULL argument");
    if (precision != RT_PREC_F64 && precision != RT_PREC_F32) return fail(RT_ERR_INVALID, "precision %d", precision);
    rt_settings s{};
    s.accel = accel;
    if (s.accel < RT_ACCEL_AUTO || s.accel > RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "accel %d", accel);
    if (sc->hs.emit_idx.empty()) return fail(RT_ERR_INVALID, "emitter sampling is off, or the scene lists no emitter");
    int rc = check_accel(sc, &s);
    if (rc) return rc;
    if (n == 0) return RT_OK;
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    DevBuf<double> d_pts, d_out;      // d_out: n x 5 doubles (omega, p_l, t_e)
    DevBuf<uint32_t> d_keys;
    DevBuf<int> d_ev;                 // n x 2 ints: emitter, visible
    hipError_t e = d_pts.ensure(6 * n);
    if (e == hipSuccess) e = d_keys.ensure(n);
    if (e == hipSuccess) e = d_out.ensure(5 * n);
    if (e == hipSuccess) e = d_ev.ensure(2 * n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pts.p, points, 6 * n * sizeof(double), hipMemcpyHostToDevice, ds.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_keys.p, keys, n * sizeof(uint32_t), hipMemcpyHostToDevice, ds.stream);
    const bool bvh = use_bvh(sc, &s);
    if (e == hipSuccess)
        e = with_view(ds, precision, [&](const auto& v) {
            return launch_emitter_samples(v, bvh, d_pts.p, d_keys.p, n, d_out.p, d_ev.p, ds.stream);
        });
    std::vector<double> out(5 * n);
    std::vector<int> ev(2 * n);
    if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_out.p, 5 * n * sizeof(double), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ev.data(), d_ev.p, 2 * n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    d_pts.release(); d_keys.release(); d_out.release(); d_ev.release();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_emitter_samples: %s", hipGetErrorString(e));
    for (size_t i = 0; i < n; ++i) {
        if (omega) for (int k = 0; k < 3; ++k) omega[3 * i + k] = out[5 * i + k];
        if (p_l) p_l[i] = out[5 * i + 3];
        if (t_e) t_e[i] = out[5 * i + 4];
        if (emitter) emitter[i] = ev[2 * i];
        if (visible) visible[i] = (uint8_t)ev[2 * i + 1];
    }
    return RT_OK;
}

int rt_aovs_device(rt_scene* sc, const rt_settings* s, float* d_guides, void* hip_stream) {
    if (!sc || !d_guides) return fail(RT_ERR_INVALID, "NULL argument");
    if (((uintptr_t)d_guides & 15) != 0) return fail(RT_ERR_INVALID, "d_guides is not 16-byte aligned");
    int cw, ch;
    int rc = check_settings(s, &cw, &ch);
    if (!rc) rc = check_accel(sc, s);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(sc->home.device));
    HIP_TRY(aovs_on(sc, s, cw, ch, d_guides, nullptr, nullptr, (hipStream_t)hip_stream));
    return RT_OK;
}

int rt_aovs(rt_scene* sc, const rt_settings* s, const rt_aov_output* out) {
    if (!sc || !out) return fail(RT_ERR_INVALID, "NULL argument");
    int cw, ch;
    int rc = check_settings(s, &cw, &ch);
    if (!rc) rc = check_accel(sc, s);
    if (rc) return rc;
    const size_t n = (size_t)cw * ch;
    DeviceState& ds = sc->home;
    HIP_TRY(hipSetDevice(ds.device));
    DevBuf<float> d_g;
    DevBuf<int> d_kind, d_idx;
    std::vector<float> g(8 * n);
    hipError_t e = d_g.ensure(8 * n);
    if (e == hipSuccess) e = d_kind.ensure(n);
    if (e == hipSuccess) e = d_idx.ensure(n);
    if (e == hipSuccess) e = aovs_on(sc, s, cw, ch, d_g.p, d_kind.p, d_idx.p, ds.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(g.data(), d_g.p, 8 * n * sizeof(float), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && out->kind) e = hipMemcpyAsync(out->kind, d_kind.p, n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    if (e == hipSuccess && out->index) e = hipMemcpyAsync(out->index, d_idx.p, n * sizeof(int), hipMemcpyDeviceToHost, ds.stream);
    const hipError_t es = hipStreamSynchronize(ds.stream);
    if (e == hipSuccess) e = es;
    d_g.release(); d_kind.release(); d_idx.release();
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_aovs: %s", hipGetErrorString(e));
    for (size_t q = 0; q < n; ++q) {                 // the guide records into the planar host arrays
        const float* r = &g[8 * q];
        if (out->albedo) { out->albedo[3 * q] = r[0]; out->albedo[3 * q + 1] = r[1]; out->albedo[3 * q + 2] = r[2]; }
        if (out->normal) { out->normal[3 * q] = r[3]; out->normal[3 * q + 1] = r[4]; out->normal[3 * q + 2] = r[5]; }
        if (out->depth) out->depth[q] = r[6];
    }
    return RT_OK;
}

int rt_guided_filter_device(rt_scene* sc, int32_t width, int32_t height, const rt_guided_params* p, const double* d_color,
                            const float* d_guides, double* d_out, void* hip_stream) {
    if (p && !guided_params_ok(p))
        return fail(RT_ERR_INVALID, "guided parameters: levels %d (1 .. %d), sigmas (%g, %g, %g, %g) each > 0", p->levels,
                    RT_GUIDED_MAX_LEVELS, p->sigma_color, p->sigma_albedo, p->sigma_normal, p->sigma_depth);
    if (!sc || !p || !d_color || !d_guides || !d_out) return fail(RT_ERR_INVALID, "NULL argument");
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "image %dx%d", width, height);
    if (((uintptr_t)d_guides & 15) != 0) return fail(RT_ERR_INVALID, "d_guides is not 16-byte aligned");
    if (d_out == d_color) return fail(RT_ERR_INVALID, "d_out must not be d_color (the filter never runs in place)");
    const hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(sc->home.device));
    if (p->levels > 1) HIP_TRY(guided_ensure(sc, sc->g_ping, 3 * (size_t)width * height));
    HIP_TRY(guided_scratch_begin(sc, st));
    HIP_TRY(guided_levels(width, height, *p, d_color, d_guides, d_out, sc->g_ping.p, st));
    HIP_TRY(guided_scratch_end(sc, st));
    return RT_OK;
}

int rt_scene_set_guided_variance(rt_scene* sc, double sigma_variance) {
    // the parameter first: a bad one is RT_ERR_INVALID with or without a device (or a scene)
    if (!(sigma_variance >= 0.0)) return fail(RT_ERR_INVALID, "sigma_variance %g: 0 (off) or > 0", sigma_variance);
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    sc->gvar_sigma = sigma_variance > 0.0 ? sigma_variance : 0.0;
    return RT_OK;
}

int rt_guided_filter_variance_device(rt_scene* sc, int32_t width, int32_t height, const rt_guided_params* p,
                                     double sigma_variance, const double* d_color, const double* d_var, const float* d_guides,
                                     double* d_out, double* d_var_out, void* hip_stream) {
    if (p && !guided_params_ok(p))
        return fail(RT_ERR_INVALID, "guided parameters: levels %d (1 .. %d), sigmas (%g, %g, %g, %g) each > 0", p->levels,
                    RT_GUIDED_MAX_LEVELS, p->sigma_color, p->sigma_albedo, p->sigma_normal, p->sigma_depth);
    if (!vguided_sigma_ok(sigma_variance)) return fail(RT_ERR_INVALID, "sigma_variance %g: must be > 0", sigma_variance);
    if (!sc || !p || !d_color || !d_var || !d_guides || !d_out) return fail(RT_ERR_INVALID, "NULL argument");
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "image %dx%d", width, height);
    if (((uintptr_t)d_guides & 15) != 0) return fail(RT_ERR_INVALID, "d_guides is not 16-byte aligned");
    const size_t n = (size_t)width * height;
    struct Span { uintptr_t a, b; };
    const auto span = [](const void* q, size_t bytes) { return Span{(uintptr_t)q, (uintptr_t)q + bytes}; };
    const auto overlap = [](Span x, Span y) { return x.a < y.b && y.a < x.b; };
    const Span ins[3] = {span(d_color, 24 * n), span(d_var, 24 * n), span(d_guides, 32 * n)};
    const Span so = span(d_out, 24 * n), sv = span(d_var_out, d_var_out ? 24 * n : 0);
    for (const Span& in : ins)
        if (overlap(so, in) || (d_var_out && overlap(sv, in)))
            return fail(RT_ERR_INVALID, "an output overlaps an input (the filter never runs in place)");
    if (d_var_out && overlap(so, sv)) return fail(RT_ERR_INVALID, "d_out and d_var_out overlap");
    const hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(sc->home.device));
    if (p->levels > 1) {
        HIP_TRY(guided_ensure(sc, sc->g_ping, 3 * n));
        HIP_TRY(guided_ensure(sc, sc->gv_ping, 3 * n));
        if (!d_var_out) HIP_TRY(guided_ensure(sc, sc->gv_aux, 3 * n));
    }
    HIP_TRY(guided_scratch_begin(sc, st));
    HIP_TRY(vguided_levels(width, height, *p, sigma_variance, d_color, d_var, d_guides, d_out,
                           d_var_out ? d_var_out : sc->gv_aux.p, sc->g_ping.p, sc->gv_ping.p, d_var_out != nullptr, st));
    HIP_TRY(guided_scratch_end(sc, st));
    return RT_OK;
}

int rt_guided_filtered_variance(rt_scene* sc, double* var) {
    if (!sc || !var) return fail(RT_ERR_INVALID, "NULL argument");
    if (sc->gv_pixels == 0 || !sc->gv_pong.p)
        return fail(RT_ERR_INVALID, "no filtered variance (no variance-guided epilogue has run on this scene)");
    HIP_TRY(hipSetDevice(sc->home.device));
    const hipStream_t st = sc->home.stream;
    HIP_TRY(guided_scratch_begin(sc, st));
    HIP_TRY(hipMemcpyAsync(var, sc->gv_pong.p, 3 * sc->gv_pixels * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(guided_scratch_end(sc, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_scene_set_error_estimate(rt_scene* sc, int32_t on) {
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    if ((on != 0) != sc->err_on) {                   // a switch either way leaves no estimate (and no threshold when off)
        sc->err_valid = false;
        sc->err_groups = sc->err_samples = 0;
        sc->err_stats = rt_error_stats{};
    }
    sc->err_on = on != 0;
    if (!sc->err_on) {
        sc->err_threshold = 0.0;
        sc->err_min_samples = 0;
    }
    return RT_OK;
}

int rt_scene_set_noise_threshold(rt_scene* sc, double threshold, int32_t min_samples) {
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    if (threshold != threshold) return fail(RT_ERR_INVALID, "noise threshold is NaN");
    if (threshold > 0.0 && !sc->err_on) return fail(RT_ERR_INVALID, "a noise threshold needs the error estimate on");
    sc->err_threshold = threshold > 0.0 ? threshold : 0.0;
    sc->err_min_samples = std::max(0, min_samples);
    return RT_OK;
}

int rt_error_stats_get(rt_scene* sc, rt_error_stats* stats) {
    if (!sc || !stats) return fail(RT_ERR_INVALID, "NULL argument");
    *stats = sc->err_stats;
    return RT_OK;
}

int rt_error_estimate_device(rt_scene* sc, double* d_var_mean, float* d_rel_error, void* hip_stream) {
    if (!sc) return fail(RT_ERR_INVALID, "scene is NULL");
    if (!sc->err_on || !sc->err_valid || sc->err_groups < 2 || sc->err_samples <= 0 || sc->ckpt_pixels == 0 ||
        !(sc->err_key == sc->ckpt_key))
        return fail(RT_ERR_INVALID, "no estimate (%d groups)", sc->err_valid ? sc->err_groups : 0);
    ImageParams im{};
    im.cw = sc->err_key.cw;
    im.ch = sc->err_key.ch;
    HIP_TRY(hipSetDevice(sc->home.device));
    HIP_TRY(launch_error_estimate(im, sc->home.sum.p, sc->err_q.p, sc->err_groups, sc->err_samples, d_var_mean, d_rel_error,
                                  nullptr, nullptr, (hipStream_t)hip_stream));
    return RT_OK;
}

int rt_error_estimate(rt_scene* sc, const rt_error_output* out) {
    if (!sc || !out) return fail(RT_ERR_INVALID, "NULL argument");
    const size_t n = sc->ckpt_pixels;
    HIP_TRY(hipSetDevice(sc->home.device));
    if (out->var_mean && n) HIP_TRY(sc->err_var.ensure(3 * n));
    if (out->rel_error && n) HIP_TRY(sc->err_rel.ensure(n));
    hipStream_t st = sc->home.stream;
    if (int rc = rt_error_estimate_device(sc, out->var_mean ? sc->err_var.p : nullptr, out->rel_error ? sc->err_rel.p : nullptr, st))
        return rc;
    if (out->var_mean) HIP_TRY(hipMemcpyAsync(out->var_mean, sc->err_var.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out->rel_error) HIP_TRY(hipMemcpyAsync(out->rel_error, sc->err_rel.p, n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

}  // extern "C"
