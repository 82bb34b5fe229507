/*
 * rt_hip.h — C ABI of the MI355X path-tracing backend (librt_hip.so).
 *
 * Drop-in boundary for the per-pixel path-tracing loop of Shinzef/BlenderRayTracer:
 *   RayTracer.prototype.render(onProgress)            js/ray-tracer.js:166-281
 *     -> rayColor(ray, depth)                          js/ray-tracer.js:102-123
 *     -> World.hit / background                        js/world.js:20-110
 *     -> Sphere/Plane/Box/Triangle/TriangleMesh.hit    js/geometry.js:15-262
 *     -> Lambertian/Metal/Dielectric/Emissive          js/materials.js:14-96
 *     -> Camera.getRay                                 js/camera.js:38-51
 *     -> toneMap / gammaCorrect epilogue               js/ray-tracer.js:151-165, post-processor.js:9-42
 * The host (JS GpuRayTracer over N-API, or Python over ctypes) packs the reference's duck-typed
 * World/Camera objects into the plain arrays below; everything under render() runs on the GPU.
 *
 * Conventions: plain C types, caller owns every host buffer, the library owns device buffers.
 * Every int-returning entry point returns 0 on success and a negative rt_status on failure;
 * rt_last_error() then holds a thread-local message.  No C++ exception crosses this ABI.
 * Randomness: the keyed counter RNG documented in DESIGN.md §RNG replaces Math.random().
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3      /* what rt_abi_version() returns: the generation of the calls and of every
                                 struct field up to it (a caller built against it keeps working).
                                 2: rt_settings.device_count / devices (multi-GPU sample split)
                                 3: rt_settings.sum_order, rt_output.preview_rgba8, rt_closest_hits */
/* Procedural textures are an append-only extension of generation 3, not a new generation: nothing a
 * generation-3 caller uses moved, and rt_scene_desc.abi_version stays RT_ABI_VERSION.  A caller that fills
 * the texture fields appended behind `perm` says so in rt_scene_desc.extensions (formerly padding) with
 * RT_DESC_TEXTURES; with any other value there the library reads nothing behind `perm`, so a binary built
 * against the shorter struct stays valid.  rt_texture_desc and rt_texture_values come with it. */
#define RT_DESC_TEXTURES 0x54455834   /* "TEX4" */
/* Scene lights (direct lighting) extend the descriptor once more, the same way: RT_DESC_LIGHTS in
 * rt_scene_desc.extensions says that the texture fields AND the light fields appended behind them are filled.
 * RT_DESC_TEXTURES keeps its meaning (nothing behind `texture_perms` is read); every other value still means
 * the struct ends at `perm`.  rt_light_desc and rt_occluded come with it.  A scene created with at least one
 * light renders with direct lighting; the hosts pass lights only when asked to. */
#define RT_DESC_LIGHTS 0x4C495434     /* "LIT4" */
#define RT_MAX_LIGHTS 32

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,     /* bad argument / descriptor */
    RT_ERR_DEVICE = -2,      /* HIP runtime error */
    RT_ERR_NOMEM = -3,
    RT_ERR_CANCELLED = -4,   /* rt_cancel() / progress() stopped the render before its last sample */
    RT_ERR_NO_DEVICE = -5    /* no HIP device visible: the backend never falls back to the CPU */
} rt_status;

/* World object kinds, in the reference's World.objects insertion order (js/world.js:20-33). */
typedef enum rt_object_type {
    RT_OBJ_SPHERE = 0,    /* geometry.js:15-45   g = {cx, cy, cz, radius}                     */
    RT_OBJ_PLANE = 1,     /* geometry.js:56-74   g = {px, py, pz, nx, ny, nz} (n normalized)  */
    RT_OBJ_BOX = 2,       /* geometry.js:85-132  g = {minx, miny, minz, maxx, maxy, maxz}     */
    RT_OBJ_TRIANGLE = 3,  /* geometry.js:148-188 one world object = triangles[first]          */
    RT_OBJ_MESH = 4       /* geometry.js:248-262 triangles[first .. first+count), last tie wins */
} rt_object_type;

typedef enum rt_material_type {
    RT_MAT_LAMBERTIAN = 0, /* materials.js:14-26 */
    RT_MAT_METAL = 1,      /* materials.js:29-42 */
    RT_MAT_DIELECTRIC = 2, /* materials.js:45-84 */
    RT_MAT_EMISSIVE = 3    /* materials.js:87-96 */
} rt_material_type;

/* Procedural textures of TexturedLambertian / TexturedMetal (materials.js:99-126, textures.js:24-81).
 * Every one depends on the hit point only (u, v are never set).  SolidColor and the base Texture are
 * not listed: the host lowers them to the plain material's albedo. */
typedef enum rt_texture_type {
    RT_TEX_CHECKER = 0,   /* textures.js:24-36 */
    RT_TEX_NOISE = 1,     /* textures.js:39-50 */
    RT_TEX_MARBLE = 2,    /* textures.js:53-65 */
    RT_TEX_WOOD = 3       /* textures.js:68-81 */
} rt_texture_type;

typedef enum rt_background_type {
    RT_BG_GRADIENT = 0,        /* World.skyGradient      world.js:35-40  */
    RT_BG_SOLID = 1,           /* World.solidBackground  world.js:42-44 (updateBackground form) */
    RT_BG_HDRI = 2,            /* World.hdriBackground   world.js:74-110 (updateBackground form) */
    RT_BG_PROCEDURAL_SKY = 3,  /* World.proceduralSky    world.js:46-72  */
    RT_BG_NAN = 4              /* JSON "solid"/"hdri": the loader binds a factory, radiance is NaN
                                  (scene-loader.js:41-45) */
} rt_background_type;

#define RT_MAX_DEVICES 8

typedef enum rt_camera_type { RT_CAM_PERSPECTIVE = 0, RT_CAM_ORTHOGRAPHIC = 1 } rt_camera_type;
/* getAntiAliasSample (ray-tracer.js:125-149): any string other than 'stochastic' and
 * 'supersampling' samples the pixel centre (RT_AA_CENTER) */
typedef enum rt_aa_mode { RT_AA_SUPERSAMPLING = 0, RT_AA_STOCHASTIC = 1, RT_AA_CENTER = 2 } rt_aa_mode;
typedef enum rt_tone_map { RT_TM_REINHARD = 0, RT_TM_ACES = 1, RT_TM_LINEAR = 2 } rt_tone_map;

/* Arithmetic of the path kernel.  F64 is the reference's own arithmetic (JS numbers are IEEE
 * binary64, no FMA contraction): ray paths agree with the reference decision for decision.
 * F32 is the fast mode; its per-channel RMS vs the reference is measured in tests. */
typedef enum rt_precision { RT_PREC_F64 = 0, RT_PREC_F32 = 1 } rt_precision;

/* World.hit evaluation.  BRUTE walks World.objects in order (world.js:24-30); BVH walks one bounding
 * volume hierarchy over the spheres and one over the triangles (built by rt_scene_create) with the
 * same tie-breaking, so both give bit-identical renders.  AUTO picks BVH for large scenes. */
typedef enum rt_accel { RT_ACCEL_AUTO = 0, RT_ACCEL_BRUTE = 1, RT_ACCEL_BVH = 2 } rt_accel;

/* Order in which a pixel's sample radiances are added into its binary64 sum (the reference adds them
 * in sample order, ray-tracer.js:202-208).  Every path decision, segment and draw count is the same in
 * both; only the rounding of the binary64 sums differs (~1e-16 relative).
 *   RT_SUM_POOL (default, fastest): the sample pool adds a tile's samples in the order its wave
 *     finishes them, then the chunk partials in chunk order.  Deterministic (the same render reproduces
 *     its bits), but an RGBA8 byte can differ from a sample-order sum by one at a floor(c*255) boundary.
 *   RT_SUM_SAMPLE_ORDER: one lane per pixel adds samples [sample_begin, sample_end) in sample order,
 *     exactly the reference's loop order (slower: DESIGN.md §4). */
typedef enum rt_sum_order { RT_SUM_POOL = 0, RT_SUM_SAMPLE_ORDER = 1 } rt_sum_order;

typedef struct rt_material_desc {
    int32_t type;          /* rt_material_type */
    int32_t _pad;
    double albedo[3];      /* Lambertian / Metal albedo */
    double roughness;      /* Metal: already Math.min(roughness, 1) (materials.js:33) */
    double ior;            /* Dielectric refractionIndex */
    double emission[3];    /* Emissive: color.mul(intensity) (materials.js:95), evaluated in double */
} rt_material_desc;        /* 72 bytes */

typedef struct rt_object_desc {
    int32_t type;          /* rt_object_type */
    int32_t material;      /* index into rt_scene_desc.materials */
    int32_t first;         /* TRIANGLE / MESH: first triangle */
    int32_t count;         /* TRIANGLE: 1; MESH: number of triangles (may be 0) */
    double g[6];           /* geometry, see rt_object_type */
} rt_object_desc;          /* 64 bytes */

typedef struct rt_texture_desc {
    int32_t type;          /* rt_texture_type */
    int32_t perm;          /* NOISE / MARBLE / WOOD: index of the texture's own PerlinNoise.p in
                              rt_scene_desc.texture_perms; CHECKER: -1 */
    double scale;          /* finite */
    double odd[3];         /* CHECKER: colour where the product of sines is < 0 */
    double even[3];        /* CHECKER: colour elsewhere (a NaN product included) */
} rt_texture_desc;         /* 64 bytes */

/* lights.js:17-48.  Point: attenuation 1 / (1 + 0.1 d + 0.01 d^2), hard shadows.  Directional: v is the
 * direction as the constructor normalized it (a zero vector stays zero: such a light never contributes). */
typedef enum rt_light_type { RT_LIGHT_POINT = 0, RT_LIGHT_DIRECTIONAL = 1 } rt_light_type;
typedef struct rt_light_desc {
    int32_t type;          /* rt_light_type */
    int32_t _pad;
    double v[3];           /* POINT: position; DIRECTIONAL: normalized direction */
    double color[3];
    double intensity;
} rt_light_desc;           /* 64 bytes */

typedef struct rt_camera_desc {  /* vectors exactly as js/camera.js:8-36 computes them */
    double origin[3];
    double lower_left[3];
    double horizontal[3];
    double vertical[3];
    double u[3], v[3], w[3];
    double lens_radius;
    int32_t type;          /* rt_camera_type ("orthographic" => normalized, focal length 1) */
    int32_t _pad;
} rt_camera_desc;

typedef struct rt_scene_desc {
    int32_t abi_version;                 /* RT_ABI_VERSION */
    int32_t num_objects;
    const rt_object_desc* objects;
    int32_t num_materials;
    int32_t num_triangles;
    const rt_material_desc* materials;
    const double* triangles;             /* 12 doubles each: v0, v1, v2, unit geometric normal
                                            normalize(cross(v1-v0, v2-v0)) (geometry.js:143-145) */
    rt_camera_desc camera;
    int32_t background;                  /* rt_background_type */
    int32_t extensions;                  /* RT_DESC_TEXTURES: the texture fields behind `perm` are filled;
                                            RT_DESC_LIGHTS: those and the light fields behind them; anything
                                            else (it was padding): nothing behind `perm` is read */
    double sky_intensity;                /* World.skyIntensity */
    double solid_color[3];               /* RT_BG_SOLID color (updateBackground uses 0.1,0.1,0.1) */
    int32_t perm[512];                   /* World.cloudNoise.p (noise.js:6-18) */
    /* extensions == RT_DESC_TEXTURES only (appended; every field above keeps its offset; not read
     * otherwise).  A textured material keeps its type
     * (RT_MAT_LAMBERTIAN / RT_MAT_METAL) and roughness; its attenuation is the texture's value at the hit
     * point instead of albedo. */
    int32_t num_textures;
    int32_t num_texture_perms;
    const rt_texture_desc* textures;     /* num_textures records */
    const int32_t* material_texture;     /* num_materials entries: texture index, -1 = untextured; may be
                                            NULL when num_textures == 0 */
    const int32_t* texture_perms;        /* num_texture_perms x 512: each noise-bearing texture's own
                                            PerlinNoise.p, entries in 0..255 */
    /* extensions == RT_DESC_LIGHTS only (appended behind the texture fields, which are then read too).  With
     * num_lights > 0 every Lambertian / textured Lambertian hit adds, per light in this order, its unoccluded
     * (attenuation * light colour) * cos; no random number is drawn and no path decision changes. */
    int32_t num_lights;                  /* 0 .. RT_MAX_LIGHTS */
    int32_t _pad2;
    const rt_light_desc* lights;         /* num_lights records, World.lights order */
} rt_scene_desc;

typedef struct rt_settings {
    int32_t width, height;     /* full image; pixel key p = (H-1-j)*W + i (ray-tracer.js:215) */
    int32_t samples;           /* sampleCount of ray-tracer.js:201, resolved by the host:
                                  1 for antiAliasing 'none', else this.samples */
    int32_t max_depth;         /* this.maxBounces */
    int32_t aa_mode;           /* rt_aa_mode */
    int32_t tone_map;          /* rt_tone_map */
    double exposure;
    double gamma;
    uint32_t seed;             /* keyed RNG seed */
    int32_t sample_begin;      /* render samples [sample_begin, sample_end) of every pixel   */
    int32_t sample_end;        /* <= 0 means sampleCount                                       */
    int32_t crop_x0, crop_y0;  /* output window (top-down rows), crop_w/h == 0 -> full image   */
    int32_t crop_w, crop_h;
    int32_t precision;         /* rt_precision */
    int32_t batch_samples;     /* samples per launch (progress/cancel granularity); 0 = all;
                                  -N = about N batches, each a multiple of the sample pool's chunk
                                  (the Node drop-in's default, -16)                               */
    int32_t denoise;           /* this.denoising: PostProcessor.denoise after gamma (ray-tracer.js:266-276);
                                  needs the full frame (crop_w/h = 0 or the whole image) */
    double denoise_weights[2]; /* Math.exp(-1/(2s*s)), Math.exp(-2/(2s*s)), s = denoiseStrength, evaluated by
                                  the host with its own exp (post-processor.js:55) */
    int32_t accel;             /* rt_accel: how World.hit is evaluated (results are identical) */
    int32_t device_count;      /* 0 or 1: the scene's own device.  N in 2..RT_MAX_DEVICES:
                                  with the sample pool (sum_order RT_SUM_POOL), WHOLE sample batches are
                                  dealt round-robin — batch k traced on devices[k % N] — and each batch's
                                  chunk partials are copied to the scene's device and added there in
                                  batch order, so the sums are bit-identical to the same batches on one
                                  device (checkpoint/resume unchanged).  The batch size is then
                                  min(batch_samples, ceil((samples - sample_begin) / N)) so that every
                                  device gets work; batch_samples = 0 gives N batches.  With
                                  RT_SUM_SAMPLE_ORDER (or when the partial slots do not fit) every batch is
                                  instead split into N contiguous sample ranges, range k on devices[k],
                                  their sums added on the scene's device in range order (equal to one
                                  device up to the order of those additions).  A device may be listed more
                                  than once (its batches run on separate streams).  The scene is uploaded
                                  to each listed device on first use and kept. */
    int32_t devices[8];        /* HIP ordinals of the devices (device_count of them).  Peer access to the
                                  scene's device is enabled where the topology has it; without it the
                                  copies are staged through host memory (reported once on stderr) */
    int32_t sum_order;         /* rt_sum_order */
} rt_settings;

/* Host outputs of rt_render, each optional (NULL = not wanted). n = crop_w*crop_h pixels,
 * top-down row-major like imageData. */
typedef struct rt_output {
    double* mean;          /* n*3: per-pixel linear mean, the toneMap() input (ray-tracer.js:208) */
    float* post;           /* n*4: post-gamma floats + alpha 1.0 (the floatData of ray-tracer.js:216-219);
                              with denoise: the denoised floats the RGBA8 bytes are made from */
    uint8_t* rgba8;        /* n*4: min(255,max(0,floor(c*255))), NaN -> 0, alpha 255 (ray-tracer.js:226-252) */
    uint32_t* segments;    /* n: world.hit calls per pixel (diagnostic; enables device counting) */
    uint32_t* draws;       /* n: RNG draws per pixel (diagnostic) */
    uint8_t* preview_rgba8;   /* n*4, progressive display (ray-tracer.js:224-241 putImageData per row): with
                                 more than one sample batch, before every progress() call this buffer holds
                                 the RGBA8 frame of the samples traced so far (mean over those samples, tone
                                 map, gamma; no denoise, like the reference's rows before its final pass;
                                 these running frames take the bytes from per-gamma thresholds computed with
                                 the binary64 pow of the exact epilogue, so they equal the rgba8 frame a
                                 render of exactly those samples gives, byte for byte).
                                 After a cancel the buffer holds the exact frame of the checkpointed samples.  A batch
                                 whose successor has already finished when the host gets to it is skipped
                                 (the buffer keeps the previous frame until the newer one is copied) */
    int32_t* preview_samples; /* optional out: the samples (from sample_begin) in preview_rgba8's frame,
                                 updated with it */
} rt_output;

typedef struct rt_stats {
    double kernel_ms;            /* device time of the path-tracing launches (HIP events on the device's
                                    accumulation stream, from the render's set-up to its last batch's
                                    merge; the maximum over devices).  With several batches and a
                                    progress callback this includes any time the GPU waited for the host */
    double finalize_ms;          /* device time of the epilogue */
    double wall_ms;              /* host wall time of the call */
    uint64_t samples;            /* pixels x samples traced */
    uint64_t segments;           /* world.hit calls (ray segments) */
    uint64_t prim_tests;         /* primitives tested: segments x primitives (brute force), counted (BVH) */
    double algorithmic_bytes;    /* SURVEY §8(d) record bytes the tests read + 12 B/pixel framebuffer:
                                    brute force: segments x sum of primitive record bytes;
                                    BVH: 64 B/node visited + 16 B/sphere + 36 B/triangle tested
                                    + segments x 24 B per plane and box */
    uint64_t node_visits;        /* BVH nodes visited (0 for brute force) */
    uint64_t sphere_tests;       /* BVH: sphere / triangle tests in visited leaves (0 for brute force) */
    uint64_t tri_tests;
    /* Direct lighting: shadow rays are not segments and draw nothing, so `segments` (and the per-pixel
     * segments / draws outputs) of a lit render equal the unlit render's, and prim_tests / algorithmic_bytes
     * of a brute-force render, which derive from segments, do not count shadow-ray work.  In BVH mode
     * node_visits, sphere_tests and tri_tests (hence prim_tests and algorithmic_bytes there) include the
     * shadow rays' walks. */
} rt_stats;

typedef struct rt_scene rt_scene;   /* opaque: scene resident in HBM of one device */

/* Library / device info. */
int rt_abi_version(void);
const char* rt_last_error(void);
int rt_device_count(int* count);

/* Scene lifetime: copies the descriptor into device memory of `device` (HIP ordinal). */
int rt_scene_create(const rt_scene_desc* desc, int device, rt_scene** out);
void rt_scene_destroy(rt_scene* scene);

/* Full render into host buffers: trace, finalize (tone map, gamma, RGBA8) and copy back.
 * Replaces RayTracer.render (ray-tracer.js:166-281) minus the DOM. Synchronous.
 * progress(fraction, user) is called between sample batches from the calling thread; a non-zero
 * return value cancels (like window.renderCancelled, ray-tracer.js:190,196), as does rt_cancel from any
 * thread.  Batches are pipelined: on one device (up to 64 batches whose partials fit RT_FUSED_MB) all
 * of them are traced by ONE launch and each batch is added as soon as its last item is done; otherwise
 * up to 3 per device are queued on the GPU beyond the one the host waits for.  With the sample pool and
 * several batches a cancel stops the batches at their next 8x8 tile x sample-chunk item: the persistent
 * (LDS) pool launches read no cancel word — rt_cancel moves each in-flight launch's work queue past its
 * last item from a high-priority stream, so every wave's next take ends its loop and only the items
 * already taken finish (about 7 ms to return on config 3) — and the one-wave pool kernel's workgroups
 * read the cancel word as they start.  The render returns once the GPU has drained; the checkpoint holds
 * the batches fully added before that.  Otherwise (sample order, one batch, partials that do not fit)
 * it is observed between batches and the queued ones complete.
 * RT_ERR_CANCELLED unless every sample was traced.
 * Threading: one call in flight per scene (rt_render, rt_render_resume, rt_trace_device,
 * rt_finalize_device, rt_render_checkpoint), as for the reference's render(); calls on different
 * scenes may run concurrently from different threads.  Asynchronous device calls on different streams
 * are ordered by the scene itself (its scratch buffers are event-guarded). */
typedef int (*rt_progress_fn)(double fraction, void* user);
int rt_render(rt_scene* scene, const rt_settings* settings, const rt_output* out,
              rt_progress_fn progress, void* user, rt_stats* stats);

/* Progressive rendering (the reference's row-by-row progress, ray-tracer.js:258-261,
 * at sample granularity).  After rt_render / rt_render_resume returns — finished or cancelled
 * (RT_ERR_CANCELLED; the checkpoint is always a whole number of batches) — the scene holds the per-pixel float64 radiance sums
 * of samples [sample_begin, samples_done).  rt_render_checkpoint copies them out (count must be
 * 3 x crop pixels) so a host can persist them; rt_render_resume traces samples
 * [samples_done, sample_end) on top of such sums and finishes like rt_render.  Every pixel still
 * adds its samples in order, so a resumed render is bit-identical to an uninterrupted one.
 * Resident checkpoints (no host copy of the sums): rt_render_checkpoint(scene, NULL, 0, &done)
 * returns only samples_done, and rt_render_resume(..., sums = NULL, samples_done, ...) continues from
 * the sums the scene still holds on its device — valid until the scene's next render (the call fails
 * with RT_ERR_INVALID unless samples_done, the frame size, the crop window, sample_begin, precision,
 * seed, aa_mode and max_depth are the checkpoint's; a render that fails before its sums are consistent
 * leaves no checkpoint). */
int rt_render_checkpoint(rt_scene* scene, double* sums, size_t count, int32_t* samples_done);
int rt_render_resume(rt_scene* scene, const rt_settings* settings, const double* sums, int32_t samples_done,
                     const rt_output* out, rt_progress_fn progress, void* user, rt_stats* stats);

/* Device-level building blocks for multi-GPU (one process per GPU): trace samples
 * [sample_begin, sample_end) and ADD per-pixel radiance sums into d_sum (device, n*3 doubles,
 * caller zeroes it); segment counting goes to stats.  Asynchronous on `hip_stream`
 * (a hipStream_t, NULL = default stream); stats are filled after the stream is synchronized
 * when `sync` is non-zero. */
int rt_trace_device(rt_scene* scene, const rt_settings* settings, double* d_sum, void* hip_stream,
                    int sync, rt_stats* stats);

/* rt_trace_device with the frame delivered band by band, so a multi-GPU caller can reduce the first
 * bands across GPUs while the later ones still trace.  The crop's 8-pixel tile rows are
 * split into `bands` horizontal bands (at most 64 and the tile rows); the trace runs on the scene's own
 * stream (after the caller's work on `hip_stream` so far) with its work items band-major, and as soon as
 * band b's items are done its sums are added into d_sum on `hip_stream` and band_ready(b, row0, rows,
 * user) is called from this thread: the caller may enqueue work on rows [row0, row0 + rows) of d_sum on
 * hip_stream (or a stream that waits for it), which runs beside the later bands' trace.  A non-zero return
 * stops the delivery (RT_ERR_CANCELLED; the trace itself completes).  Returns once every band was
 * delivered and hip_stream has been ordered after the whole trace.  d_sum ends up equal to
 * rt_trace_device's, bit for bit (same work items, same chunk partials, same order of additions). */
typedef int (*rt_band_fn)(int32_t band, int32_t row0, int32_t rows, void* user);
int rt_trace_device_bands(rt_scene* scene, const rt_settings* settings, double* d_sum, void* hip_stream, int32_t bands,
                          rt_band_fn band_ready, void* user, rt_stats* stats);

/* Epilogue on device: mean = sum / sampleCount, toneMap, gammaCorrect, optional denoise, RGBA8
 * (ray-tracer.js:208-276).  Any output pointer may be NULL.  All pointers are device pointers; the
 * scene provides the scratch buffer the denoise pass reads from. */
int rt_finalize_device(rt_scene* scene, const rt_settings* settings, const double* d_sum, double* d_mean,
                       float* d_post, uint8_t* d_rgba8, void* hip_stream);

/* Diagnostic (tests): World.hit for `n` rays on the scene's device — the device arithmetic of the
 * trace kernel's closest-hit stage (brute force in World.objects order, or the BVH walk), so the
 * BVH's bit-identity proof is checked on the instructions the GPU runs.  rays: host, n x 6 doubles
 * (origin xyz, direction xyz; rounded to binary32 first in RT_PREC_F32).  Outputs (host, n each, any may
 * be NULL): t (binary64 of the winning parameter, +inf when nothing is hit), kind (-1 none, 0 sphere,
 * 1 plane, 2 box, 3 triangle), index (primitive index within its kind, in World.objects order; mesh
 * triangles in mesh order). */
int rt_closest_hits(rt_scene* scene, int32_t precision, int32_t accel, const double* rays, size_t n,
                    double* t, int32_t* kind, int32_t* index);

/* Diagnostic (tests): the lit trace kernels' occlusion (any-hit) query, World.hit(ray, 0.001, tmax[i]) !== null,
 * for `n` rays on the scene's device, the diagnostic twin of rt_closest_hits (same rays layout, precision and
 * accel; any scene, lit or not).  out: host, n bytes, 1 = occluded.  A primitive at t == tmax does not occlude;
 * tmax may be +inf. */
int rt_occluded(rt_scene* scene, int32_t precision, int32_t accel, const double* rays, const double* tmax, size_t n,
                uint8_t* out);

/* Diagnostic (tests): Texture.value(u, v, p) of texture `texture` at `n` host points (n x 3 doubles; rounded
 * to binary32 first in RT_PREC_F32) evaluated on the scene's device by the function the trace kernels call;
 * rgb: host, n x 3 doubles.  RT_ERR_INVALID unless 0 <= texture < num_textures. */
int rt_texture_values(rt_scene* scene, int32_t precision, int32_t texture, const double* points, size_t n,
                      double* rgb);

/* Diagnostic: the walk a render with these precision / accel settings runs on this scene — 0 World.objects
 * order (brute force), 1 a BVH tree walk, 2 the uniform grid over the spheres (sphere-only scenes where
 * the host's sampled cost estimate prefers it, scene_pack.h choose_walk; never for a scene with textures,
 * lights or sampled emitters, whose kernels walk World order or the trees); < 0 an error status.  Every walk finds the same closest
 * hit; they differ in speed only. */
int rt_scene_walk(rt_scene* scene, int32_t precision, int32_t accel);

/* Feature buffers and the guided denoiser: an append-only extension of generation 3 (RT_ABI_VERSION and every
 * struct above stay as they are).
 *
 * Feature buffers (AOVs) of the primary hit: one ray per pixel through the pixel centre (the RT_AA_CENTER
 * formula) from a pinhole (lens offset zero), so no random number is drawn; the closest hit is the trace
 * kernels' own query (rt_closest_hits).  Per pixel: albedo (Lambertian / Metal: the albedo, a textured
 * material's texture value at the hit point — in RT_PREC_F32 with the textures' sines taken from the binary64
 * sine rounded to binary32, so the buffer is the same bits on every device and host, within an ulp or two of
 * the value the binary32 trace kernels use; Dielectric (1, 1, 1); Emissive min(emission, 1) per channel),
 * the hit record's normal (facing the ray) and depth = t |d|; a miss gives albedo and normal 0 and depth
 * +inf.  Computed in the settings' precision, stored as binary32.  Only width, height, the crop window,
 * precision and accel of the settings are read. */
#define RT_GUIDED_MAX_LEVELS 8
/* the hosts' defaults (chosen by the sweep of DESIGN.md §4 "Guided filter") */
#define RT_GUIDED_DEFAULT_LEVELS 5
#define RT_GUIDED_DEFAULT_SIGMA_COLOR 1.0
#define RT_GUIDED_DEFAULT_SIGMA_ALBEDO 0.1
#define RT_GUIDED_DEFAULT_SIGMA_NORMAL 0.35
#define RT_GUIDED_DEFAULT_SIGMA_DEPTH 0.05
typedef struct rt_guided_params {
    int32_t levels, _pad;      /* 1 .. RT_GUIDED_MAX_LEVELS à-trous levels (step 1, 2, 4, ...) */
    double sigma_color, sigma_albedo, sigma_normal, sigma_depth;   /* each > 0; +inf switches the term off */
} rt_guided_params;
/* Host outputs of rt_aovs, each optional (NULL = not wanted); n = crop pixels, top-down row-major. */
typedef struct rt_aov_output {
    float* albedo;             /* n*3 */
    float* normal;             /* n*3 */
    float* depth;              /* n */
    int32_t* kind;             /* n: as rt_closest_hits reports it (-1 none) */
    int32_t* index;            /* n: likewise */
} rt_aov_output;
int rt_aovs(rt_scene* scene, const rt_settings* settings, const rt_aov_output* out);
/* The same on device: d_guides (n x 8 floats, 16-byte aligned) = albedo[3], normal[3], depth, 0 per pixel, the
 * guide records rt_guided_filter_device reads.  Asynchronous on hip_stream. */
int rt_aovs_device(rt_scene* scene, const rt_settings* settings, float* d_guides, void* hip_stream);
/* The guided filter (edge-avoiding à-trous wavelet filter): d_color (width x height x 3 binary64,
 * the linear mean) filtered along d_guides into d_out, always in binary64; d_color is not written and d_out
 * must not overlap it.  The intermediate levels ping-pong between d_out and one scratch frame the scene owns.
 * Non-finite pixels pass through unchanged and are never averaged into others.  Asynchronous on hip_stream. */
int rt_guided_filter_device(rt_scene* scene, int32_t width, int32_t height, const rt_guided_params* params,
                            const double* d_color, const float* d_guides, double* d_out, void* hip_stream);
/* NULL = off (the default).  While set, the final epilogue of rt_render / rt_render_resume and
 * rt_finalize_device filter the mean (sum / samples) along the guides of the settings' frame before tone
 * mapping: rt_output.mean is the filtered mean and post / rgba8 are made from it (the Gaussian `denoise`, if
 * also on, runs after it).  Like `denoise` it needs the full frame (RT_ERR_INVALID for a crop).  Running
 * preview frames are not filtered, and the scene's sums are never overwritten: checkpoints and resumes are
 * unchanged.  The parameters are validated before any device is touched (RT_ERR_INVALID). */
int rt_scene_set_guided(rt_scene* scene, const rt_guided_params* params);

/* Emitter sampling (next-event estimation with multiple importance sampling): an append-only
 * extension of generation 3.  Off by default.  While on, every Lambertian / TexturedLambertian hit but the last
 * allowed bounce's samples one of the scene's listed emitters — every Emissive sphere (finite r2 > 0) and
 * triangle (standalone or of a mesh; finite normal and area > 0) whose emission is finite with a component
 * > 0, in World.objects order — and the emission a scattered ray meets is weighted by the balance heuristic,
 * so the render has the plain render's expectation with less variance.  Emissive boxes and planes are not
 * listed and keep weight 1.  A scene without listed emitters renders exactly what it rendered before.
 * Switching it changes what later renders compute: not to be called while a render of the scene is in flight,
 * and a checkpoint taken before does not resume after.  RT_ERR_INVALID: scene NULL, or more than
 * RT_MAX_EMITTERS listed (the setting is then left off). */
#define RT_MAX_EMITTERS 1048576
int rt_scene_set_emitter_sampling(rt_scene* scene, int32_t on);
/* The number of listed emitters (0 while emitter sampling is off). */
int rt_scene_emitter_count(rt_scene* scene, int32_t* count);
/* Diagnostic (tests): the emitter-sampling kernels' own sample for `n` queries on the scene's device, the twin of
 * rt_occluded.  points: host, n x 6 doubles (hit point x, facing normal n; rounded to binary32 first in
 * RT_PREC_F32); keys: n 32-bit keys of the emitter stream (the kernels derive theirs from the sample's key and
 * the bounce).  Outputs (host, n each, any may be NULL): emitter (index in the list), omega (n x 3, the unit
 * direction), p_l (its solid-angle density, the 1 / N of the emitter choice included), t_e (the sampled
 * primitive's own candidate t along omega), visible (1: nothing nearer than t_e).  Stages a query does not reach
 * leave zeros: no sample (inside the sphere, an edge-on triangle) omega = p_l = 0; n . omega <= 0 or no candidate
 * t_e = 0 and visible = 0.  RT_ERR_INVALID unless emitter sampling is on with at least one emitter. */
int rt_emitter_samples(rt_scene* scene, int32_t precision, int32_t accel, const double* points, const uint32_t* keys,
                       size_t n, int32_t* emitter, double* omega, double* p_l, double* t_e, uint8_t* visible);

/* Per-pixel error estimate and the noise-threshold stop (DESIGN.md §4 "Error estimate"): an
 * append-only extension of generation 3.  Off by default; while off, renders run exactly as before.
 *
 * The sample pool writes one partial sum per pixel and chunk of samples.  While the estimate is on, every batch's
 * reduce is followed by a pass that adds S_c^2 / n_c of every chunk to a per-pixel second moment q (binary64,
 * 3 per pixel, on the scene's device) under the batch's commit gate, so the moments cover exactly the samples
 * the sums hold.  With K chunks over N samples and S their sum, B = q - S^2 / N has expectation (K - 1) sigma^2
 * whatever the chunk sizes; var_mean = max(0, B) / ((K - 1) N) estimates the variance of the pixel's mean per
 * channel.  A pixel's relative error is e_p = sqrt(sum_ch var_mean) / (sum_ch mean + 0.03); the frame's error is
 * the mean of e_p over the pixels whose sums and moments are finite.  A pixel with a non-finite sum or moment
 * has NaN in every channel and is counted in nonfinite_pixels.
 *
 * rt_render zeroes the moments; rt_render_resume with sums NULL continues them; a resume from host sums leaves
 * no estimate.  rt_render / rt_render_resume return RT_ERR_INVALID while the estimate is on and the render has
 * no chunk partials: RT_SUM_SAMPLE_ORDER (or the pool switched off), max_depth <= 0, or several devices that
 * split every batch's samples (whole batches per device are supported).  rt_trace_device and
 * rt_trace_device_bands never produce an estimate.  Not to be switched while a render is in flight. */
int rt_scene_set_error_estimate(rt_scene* scene, int32_t on);
/* Stop a progressive render at the first batch after which frame_error <= threshold and the estimate covers at
 * least min_samples samples (counted from sample_begin).  threshold <= 0: off (the default).  A threshold > 0
 * needs the estimate on (RT_ERR_INVALID otherwise, here and in rt_render).  The decision is taken on the device
 * in stream order (it sets the word the later batches' commit gates read), so the batch a render stops at does
 * not depend on host timing.  The stopped render drains like a cancelled one, runs the normal epilogue over the
 * samples committed (mean = sum / samples done; guided filter, tone map and denoise as configured), reports
 * them in rt_stats.samples, leaves the checkpoint there (a resume may continue to the full count) and returns
 * RT_OK.  A render of one batch has nothing to stop; a threshold with several batches that do not overlap on
 * the device (RT_OVERLAP=0, or no memory for the partial slots) is RT_ERR_INVALID. */
int rt_scene_set_noise_threshold(rt_scene* scene, double threshold, int32_t min_samples);
typedef struct rt_error_stats {
    int32_t samples;            /* samples (from sample_begin) the estimate covers = the committed batches */
    int32_t groups;             /* K, chunk partials accumulated per pixel (< 2: no estimate, the figures are NaN) */
    int32_t chunk_samples;      /* the pool's chunk for this render */
    int32_t converged;          /* 1: the frame met the threshold (the render stopped there unless it was its last batch) */
    int64_t pixels, nonfinite_pixels;
    double frame_error, max_error;
} rt_error_stats;
/* The figures after the last committed batch the host has seen.  Host read only: may be called inside
 * progress() (the figures of the batch just reported).  groups = 0 when there is no estimate at all. */
int rt_error_stats_get(rt_scene* scene, rt_error_stats* stats);
typedef struct rt_error_output {
    double* var_mean;           /* n*3, may be NULL */
    float* rel_error;           /* n, may be NULL */
} rt_error_output;
/* The per-pixel estimate of the last render, between renders.  RT_ERR_INVALID ("no estimate") when groups < 2,
 * when there has been no render since the estimate was switched on, or after a resume from host sums. */
int rt_error_estimate(rt_scene* scene, const rt_error_output* out);
/* The same into device buffers (either may be NULL), asynchronous on hip_stream: it reads the scene's sums and
 * moments, so the caller orders it before the scene's next render. */
int rt_error_estimate_device(rt_scene* scene, double* d_var_mean, float* d_rel_error, void* hip_stream);

/* The variance-guided form of the guided filter (DESIGN.md §4 "Variance-guided filter"): an
 * append-only extension of generation 3.  Off by default; while off, every render runs exactly as before.
 *
 * The colour term of a tap is |c_p - c_q|^2 / (sigma_variance^2 (vb_p + 2^-40)) on the raw linear colour, vb_p
 * being the 3 x 3 binomial mean of the channels' summed variance around p; rt_guided_params.sigma_color is not
 * read, and no sigma is scaled per level.  Every level also propagates the variance, v' = sum w^2 v / (sum w)^2, so
 * the stop tightens as the levels smooth.  Always binary64.  A pixel whose colour or variance has a non-finite
 * channel passes through in both outputs and is never averaged into others; a negative variance reads as 0. */
#define RT_GUIDED_DEFAULT_SIGMA_VARIANCE 4.0   /* the hosts' default (the sweep of DESIGN.md §4) */
/* sigma_variance: 0 = off (the default); > 0 (+inf allowed) = on; negative or NaN: RT_ERR_INVALID, validated before
 * any device is touched.  While on, the guided epilogue of rt_render / rt_render_resume filters the mean with the
 * variance form, var_mean being the error estimate's of the committed samples and groups; the sums and moments
 * are only read, so checkpoints and resumes are unchanged.  It needs the guided filter set (and so the full
 * frame) and the error estimate on, and a render that commits at least 2 groups (rt_error_stats.groups):
 * rt_render / rt_render_resume return RT_ERR_INVALID before anything is traced otherwise — also for a resume from
 * host sums, which leaves no estimate.  rt_finalize_device returns RT_ERR_INVALID while it is on
 * (rt_trace_device never produces an estimate).  Running previews and cancelled renders stay unfiltered. */
int rt_scene_set_guided_variance(rt_scene* scene, double sigma_variance);
/* The building block on caller buffers: d_color and d_var (width x height x 3 binary64: the linear mean and the
 * variance of the mean per channel) filtered along d_guides (16-byte aligned) into d_out and d_var_out (the
 * propagated variance; may be NULL).  The inputs are not written; an output that overlaps an input or the other
 * output is RT_ERR_INVALID.  params->sigma_color is not read (it must still be > 0).  The intermediate levels use
 * scratch frames the scene owns.  Asynchronous on hip_stream. */
int rt_guided_filter_variance_device(rt_scene* scene, int32_t width, int32_t height, const rt_guided_params* params,
                                     double sigma_variance, const double* d_color, const double* d_var,
                                     const float* d_guides, double* d_out, double* d_var_out, void* hip_stream);
/* The propagated variance v' of the scene's last variance-guided epilogue: n x 3 doubles on the host, n the
 * pixels of that render.  RT_ERR_INVALID when there is none. */
int rt_guided_filtered_variance(rt_scene* scene, double* var);

/* Request cancellation of an in-flight rt_render on `scene` (the pool kernels read it between items;
 * see rt_render). */
int rt_cancel(rt_scene* scene);

/* Diagnostic (tests): the hit record the trace kernels rebuild at World.hit's winner, for `n` rays on the scene's
 * device: rt_closest_hits' query (same rays layout, precision rounding and accel) followed by the function the
 * shading stage calls on its result.  Outputs (host, any may be NULL): t, kind and index as rt_closest_hits
 * reports them; point and normal (n x 3 doubles each: origin + direction * t and the normal turned against the
 * ray), front (n bytes, 1: the ray met the outward side) and mat (n: the material's index in the scene).  A row
 * without a hit gets NaN in point and normal, front 0 and mat -1. */
int rt_hit_records(rt_scene* scene, int32_t precision, int32_t accel, const double* rays, size_t n, double* t,
                   int32_t* kind, int32_t* index, double* point, double* normal, uint8_t* front, int32_t* mat);

/* Diagnostic (tests): one path segment of the trace kernels for `n` rays on the scene's device.  Ray r starts with
 * the random stream {key = keys[2 r], draws so far = keys[2 r + 1]}, throughput (1, 1, 1) and `depth` bounces left;
 * its closest hit is found as the trace kernels find it (rays, precision and accel as rt_closest_hits; RT_ACCEL_BVH
 * is the general tree walk) and handed to the kernels' own shading function: emission, scatter or background.
 * out_f (host, n x 12 doubles, may be NULL): the next ray's origin and direction, the throughput T and the radiance
 * L the segment ends the path with; out_i (host, n x 4, may be NULL): done (1: the path ended; origin, direction and
 * T are then whatever the function left), the hit's kind and index as rt_closest_hits reports them, and the stream's
 * draw count afterwards.  Any scene without procedural textures, an empty one included (every ray then gets the
 * background); scene lights and emitter sampling are not evaluated.  variant: 0 the general feature set; 1 the lean
 * triangle-tree kernel's (spheres, planes, triangles; the sky gradient) with its out-of-line exact Schlick path;
 * 2 the lean grid kernel's (spheres alone; the sky gradient).  RT_ERR_INVALID when the scene has what the variant
 * leaves out. */
int rt_shade_segments(rt_scene* scene, int32_t precision, int32_t accel, int32_t variant, const double* rays,
                      const uint32_t* keys, int32_t depth, size_t n, double* out_f, int32_t* out_i);

/* Diagnostic (tests): the camera ray the trace kernels start sample s of pixel (i, j) with (j counted from the
 * bottom row, as getRay's t), for `n` triples pixels[3 r ..] = (i, j, s) on the scene's device.  Of the settings
 * width, height, aa_mode, seed and precision are read (the pixel's key is the render's).  out (host, n x 6 doubles,
 * may be NULL): origin and direction; draws (host, n, may be NULL): random numbers the sample start consumed.
 * variant bit 0: the camera is read from the kernel-argument segment at every sample start, as the binary32 and the
 * lean grid kernels read it; bit 1: the lean kernels' form without orthographic cameras and without the stochastic
 * and centre AA modes (RT_ERR_INVALID for a scene or settings that need them).  All four give the same bits. */
int rt_camera_rays(rt_scene* scene, const rt_settings* settings, int32_t variant, const int32_t* pixels, size_t n,
                   double* out, uint32_t* draws);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
