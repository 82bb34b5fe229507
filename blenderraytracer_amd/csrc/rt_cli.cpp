// rt_cli.cpp — Node-free command line front end of librt_hip.so (SURVEY §8b "a C++ bench CLI").
//
//   rt_render_cli scene.json [--width W] [--height H] [--spp S] [--depth D] [--seed N]
//                 [--aa supersampling|stochastic|none] [--tone reinhard|aces|linear]
//                 [--exposure E] [--gamma G] [--denoise STRENGTH] [--precision f64|f32]
//                 [--accel auto|bvh|brute] [--frames K] [--warmup W] [--batch B] [--device N]
//                 [--out image.ppm|image.pam] [--lights] [--nee]
//                 [--guided] [--guided-levels N] [--guided-sigma C,A,N,Z] [--aovs PREFIX]
//                 [--guided-variance [S]] [--noise T] [--min-spp N]
//
// --noise T: stop at the first progress batch after which the frame's estimated error (rt_error_stats.frame_error)
// is at or under T; --min-spp N: not before N samples.  Either implies the error estimate
// (rt_scene_set_error_estimate) and at least 16 progress batches (--batch B is kept when it gives that many);
// the JSON line then carries samples_done, frame_error and converged
// --guided: the edge-aware guided filter over the linear mean (rt_scene_set_guided; --guided-levels and
// --guided-sigma colour,albedo,normal,depth override the defaults and imply it)
// --guided-variance [S]: the filter's variance-guided form (rt_scene_set_guided_variance) with sigma_variance S
// (default RT_GUIDED_DEFAULT_SIGMA_VARIANCE); implies --guided and the error estimate, and without --batch about 4
// progress batches (the form needs at least 2 chunk partials per pixel)
// --aovs PREFIX: the feature buffers of the primary hit (rt_aovs) as PREFIX.albedo.pfm, PREFIX.normal.pfm (colour
// PFM) and PREFIX.depth.pfm (greyscale PFM), little-endian binary32, rows bottom-up as PFM has them
// --nee: sample the scene's emissive spheres and triangles with MIS (rt_scene_set_emitter_sampling; off by default)
// --lights: direct lighting from the scene's "lights" (rt_json_scene_desc_lit; off by default)
//
// Does what a reference user does in the browser: RayTracer(width, height) -> loadFromJSON(scene)
// (rt_json_scene_load: scene-loader.js semantics incl. a camera "resolution" resize) ->
// updateRenderSettings({...}) (ray-tracer.js:554-566, `||` defaults) -> render() (rt_render).
// Prints one JSON line with the timing of the timed frames; writes the RGBA8 image of the last
// frame as binary PPM (RGB) or PAM (RGBA).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_hip.h"
#include "../../include/rt_scene_json.h"
#include "js_math.h"

namespace {

[[noreturn]] void die(const char* what, const char* detail = "") {
    fprintf(stderr, "rt_render_cli: %s%s\n", what, detail);
    exit(2);
}

void check(int status, const char* what) {
    if (status != RT_OK) die(what, (std::string(": ") + rt_last_error()).c_str());
}

std::string read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) die("cannot open ", path);
    std::string s;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// `value || dflt` for a numeric setting (updateRenderSettings, ray-tracer.js:556-565)
double js_or(double v, double dflt) { return (v == 0 || v != v) ? dflt : v; }

// a Portable Float Map: "PF" (3 channels) or "Pf" (1), a negative scale = little-endian, rows bottom to top
void write_pfm(const std::string& path, const float* data, int width, int height, int channels) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) die("cannot write ", path.c_str());
    fprintf(f, "%s\n%d %d\n-1.0\n", channels == 3 ? "PF" : "Pf", width, height);
    for (int row = height - 1; row >= 0; --row) fwrite(data + (size_t)row * width * channels, sizeof(float), (size_t)width * channels, f);
    fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !strcmp(argv[1], "--help")) {
        fprintf(stderr, "usage: rt_render_cli scene.json [--width W --height H --spp S --depth D --seed N --aa MODE "
                        "--tone MAP --exposure E --gamma G --denoise STRENGTH --precision f64|f32 --accel auto|bvh|brute "
                        "--frames K --warmup W --batch B --device N --out FILE --lights --nee --guided --guided-levels N "
                        "--guided-sigma C,A,N,Z --guided-variance [S] --aovs PREFIX --noise T --min-spp N]\n");
        return argc < 2 ? 2 : 0;
    }
    const char* scene_path = argv[1];
    int width = 800, height = 600, frames = 1, warmup = 0, batch = 0, device = 0;
    double spp = 4, depth = 5, exposure = 1.0, gamma = 2.2, denoise = 0, noise = 0;
    int min_spp = 0;
    bool estimate = false;
    uint32_t seed = 1;
    std::string aa = "supersampling", tone = "reinhard", precision = "f64", accel = "auto", out, aovs;
    bool lights = false, guided = false, nee = false, gvar = false;
    double gvar_sigma = RT_GUIDED_DEFAULT_SIGMA_VARIANCE;
    rt_guided_params gp{RT_GUIDED_DEFAULT_LEVELS, 0, RT_GUIDED_DEFAULT_SIGMA_COLOR, RT_GUIDED_DEFAULT_SIGMA_ALBEDO,
                        RT_GUIDED_DEFAULT_SIGMA_NORMAL, RT_GUIDED_DEFAULT_SIGMA_DEPTH};
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--lights") { lights = true; continue; }
        if (a == "--nee") { nee = true; continue; }
        if (a == "--guided") { guided = true; continue; }
        if (a == "--guided-variance") {                     // the value is optional
            gvar = guided = true;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) {
                gvar_sigma = atof(argv[++i]);
                if (!(gvar_sigma > 0.0)) die("--guided-variance takes a sigma > 0: ", argv[i]);
            }
            continue;
        }
        if (i + 1 >= argc) die("missing value for ", a.c_str());
        const char* v = argv[++i];
        if (a == "--width") width = atoi(v);
        else if (a == "--height") height = atoi(v);
        else if (a == "--spp") spp = atof(v);
        else if (a == "--depth") depth = atof(v);
        else if (a == "--seed") seed = (uint32_t)strtoul(v, nullptr, 0);
        else if (a == "--aa") aa = v;
        else if (a == "--tone") tone = v;
        else if (a == "--exposure") exposure = atof(v);
        else if (a == "--gamma") gamma = atof(v);
        else if (a == "--denoise") denoise = atof(v);
        else if (a == "--precision") precision = v;
        else if (a == "--accel") accel = v;
        else if (a == "--frames") frames = atoi(v);
        else if (a == "--warmup") warmup = atoi(v);
        else if (a == "--batch") batch = atoi(v);
        else if (a == "--device") device = atoi(v);
        else if (a == "--out") out = v;
        else if (a == "--aovs") aovs = v;
        else if (a == "--noise") { noise = atof(v); estimate = true; }
        else if (a == "--min-spp") { min_spp = atoi(v); estimate = true; }
        else if (a == "--guided-levels") { gp.levels = atoi(v); guided = true; }
        else if (a == "--guided-sigma") {
            if (sscanf(v, "%lf,%lf,%lf,%lf", &gp.sigma_color, &gp.sigma_albedo, &gp.sigma_normal, &gp.sigma_depth) != 4)
                die("--guided-sigma takes colour,albedo,normal,depth: ", v);
            guided = true;
        }
        else die("unknown option ", a.c_str());
    }
    if (frames < 1 || warmup < 0) die("--frames must be >= 1 and --warmup >= 0");

    const std::string text = read_file(scene_path);
    rt_json_scene* js = nullptr;
    check(rt_json_scene_load(text.data(), text.size(), width, height, seed, &js), "loading the scene");
    rt_json_scene_size(js, &width, &height);                 // a camera "resolution" resizes
    rt_scene* scene = nullptr;
    const double t_up = now_ms();
    const rt_scene_desc* desc = lights ? rt_json_scene_desc_lit(js) : rt_json_scene_desc(js);
    if (!desc) die("--lights: ", rt_last_error());
    check(rt_scene_create(desc, device, &scene), "uploading the scene");
    const double upload_ms = now_ms() - t_up;
    if (nee) check(rt_scene_set_emitter_sampling(scene, 1), "--nee");
    if (guided) check(rt_scene_set_guided(scene, &gp), "--guided");

    rt_settings s{};
    s.width = width;
    s.height = height;
    s.samples = aa == "none" ? 1 : (int)js_or(spp, 4);     // sampleCount (ray-tracer.js:201)
    s.max_depth = (int)js_or(depth, 5);
    s.aa_mode = aa == "supersampling" ? RT_AA_SUPERSAMPLING : (aa == "stochastic" ? RT_AA_STOCHASTIC : RT_AA_CENTER);
    s.tone_map = tone == "aces" ? RT_TM_ACES : (tone == "linear" ? RT_TM_LINEAR : RT_TM_REINHARD);
    s.exposure = js_or(exposure, 1.0);
    s.gamma = js_or(gamma, 2.2);
    s.seed = seed;
    s.precision = precision == "f32" ? RT_PREC_F32 : RT_PREC_F64;
    s.accel = accel == "bvh" ? RT_ACCEL_BVH : (accel == "brute" ? RT_ACCEL_BRUTE : RT_ACCEL_AUTO);
    s.batch_samples = batch;
    if (estimate) {
        // at least 16 progress batches for the threshold to act on (-16: about 16, sized to the pool's chunks)
        if (batch <= 0 || (s.samples + batch - 1) / batch < 16) s.batch_samples = -16;
        check(rt_scene_set_error_estimate(scene, 1), "--noise");
        check(rt_scene_set_noise_threshold(scene, noise, min_spp), "--noise");
    }
    if (gvar) {
        if (!estimate) {
            if (batch <= 0) s.batch_samples = -4;
            check(rt_scene_set_error_estimate(scene, 1), "--guided-variance");
        }
        check(rt_scene_set_guided_variance(scene, gvar_sigma), "--guided-variance");
    }
    if (denoise > 0) {                                       // post-processor.js:55 weights, host exp
        s.denoise = 1;
        s.denoise_weights[0] = jsm::exp(-1.0 / (2 * denoise * denoise));   // V8's Math.exp (post-processor.js:60)
        s.denoise_weights[1] = jsm::exp(-2.0 / (2 * denoise * denoise));
    }
    const size_t n = (size_t)width * height;
    std::vector<uint8_t> rgba(4 * n);
    rt_output o{};
    o.rgba8 = rgba.data();
    rt_stats st{};
    for (int k = 0; k < warmup; ++k) check(rt_render(scene, &s, &o, nullptr, nullptr, &st), "rendering");
    double wall = 0, kernel = 0;
    uint64_t segments = 0, nodes = 0, traced = 0;
    for (int k = 0; k < frames; ++k) {
        const double t0 = now_ms();
        check(rt_render(scene, &s, &o, nullptr, nullptr, &st), "rendering");
        wall += now_ms() - t0;
        kernel += st.kernel_ms;
        segments += st.segments;
        traced += st.samples;                                // (fewer than n * spp when --noise stopped the frame)
        nodes += st.node_visits;
    }
    const double samples = (double)traced;
    rt_error_stats es{};
    if (estimate) check(rt_error_stats_get(scene, &es), "--noise");
    printf("{\"scene\": \"%s\", \"width\": %d, \"height\": %d, \"spp\": %d, \"max_depth\": %d, \"precision\": \"%s\", "
           "\"accel\": \"%s\", \"frames\": %d, \"msamples_per_s\": %.3f, \"kernel_msamples_per_s\": %.3f, "
           "\"ms_per_frame\": %.3f, \"kernel_ms_per_frame\": %.3f, \"upload_ms\": %.3f, \"segments_per_sample\": %.4f, "
           "\"bvh_nodes_per_segment\": %.3f",
           scene_path, width, height, s.samples, s.max_depth, precision.c_str(), accel.c_str(), frames,
           samples / (wall * 1e-3) / 1e6, samples / (kernel * 1e-3) / 1e6, wall / frames, kernel / frames, upload_ms,
           segments / samples, segments ? (double)nodes / segments : 0.0);
    if (estimate) {                                         // the last frame's: samples done and the frame's error
        printf(", \"samples_done\": %d, \"converged\": %d, \"error_groups\": %d, \"frame_error\": ", es.samples, es.converged,
               es.groups);
        if (es.frame_error == es.frame_error) printf("%.17g", es.frame_error);
        else printf("null");
    }
    printf("}\n");
    if (!out.empty()) {
        FILE* f = fopen(out.c_str(), "wb");
        if (!f) die("cannot write ", out.c_str());
        const bool pam = out.size() > 4 && out.compare(out.size() - 4, 4, ".pam") == 0;
        if (pam) {
            fprintf(f, "P7\nWIDTH %d\nHEIGHT %d\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n", width, height);
            fwrite(rgba.data(), 1, rgba.size(), f);
        } else {
            fprintf(f, "P6\n%d %d\n255\n", width, height);
            std::vector<uint8_t> rgb(3 * n);
            for (size_t q = 0; q < n; ++q) memcpy(&rgb[3 * q], &rgba[4 * q], 3);
            fwrite(rgb.data(), 1, rgb.size(), f);
        }
        fclose(f);
    }
    if (!aovs.empty()) {
        std::vector<float> albedo(3 * n), normal(3 * n), zdepth(n);
        rt_aov_output ao{albedo.data(), normal.data(), zdepth.data(), nullptr, nullptr};
        check(rt_aovs(scene, &s, &ao), "--aovs");
        write_pfm(aovs + ".albedo.pfm", albedo.data(), width, height, 3);
        write_pfm(aovs + ".normal.pfm", normal.data(), width, height, 3);
        write_pfm(aovs + ".depth.pfm", zdepth.data(), width, height, 1);
    }
    rt_scene_destroy(scene);
    rt_json_scene_destroy(js);
    return 0;
}
