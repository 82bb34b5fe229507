// pt_guided.hip — the feature buffers (aov_kernel), the guided filter (guided_level_kernel) and its
// variance-guided form (vguided_level_kernel) for gfx950.
//
// A translation unit of its own, built with the common flags only: the trace kernels' units do not see it,
// so their code generation stays what it was.  The per-pixel bodies are aov_pixel (pt_path.h) and
// guided_pixel (pt_guided.h) and vguided_pixel (pt_vguided.h), which tests/hostcheck compiles for the CPU.
#include <algorithm>

#include "pt_guided.h"
#include "pt_vguided.h"
#include "kernel_select.h"

namespace rt {

// ---- feature buffers of the primary hit -------------------------------------------------------------
// One-wave workgroups with the traversal stack in LDS, as closest_hits_kernel (pt_trace.hip) has it, and the
// same walk: an LDS mode reads the copy one wave stages here — the grid's [records][cell offsets], or the
// WideLds block of the sphere tree (or of the triangle tree's top levels) with the wave's stacks.
namespace {

// two-child nodes [0, n) into LDS: child boxes at box[3k .. 3k+2], references at kid[k]
__device__ __forceinline__ void stage_wide_nodes(const Bvh2Node* src, int n, rt_u4* box, rt_u2* kid, int t) {
    for (int k = t; k < n; k += 64) {
        const rt_u4* g = reinterpret_cast<const rt_u4*>(src + k);
        const rt_u4 q3 = g[3];
        box[3 * k] = g[0];
        box[3 * k + 1] = g[1];
        box[3 * k + 2] = g[2];
        kid[k] = rt_u2{q3.x, q3.y};
    }
}

template <class R, int ACC>
__device__ __forceinline__ BvhStack stage_walk_lds(const SceneView<R>& sc, unsigned char* lds_dyn) {
    BvhStack stk{nullptr, 0};
    if constexpr (ACC == ACC_GRID_LDS || ACC == ACC_GRID_LDS_LEAN) {
        rt_u4* grec = reinterpret_cast<rt_u4*>(lds_dyn);
        int* gcell = reinterpret_cast<int*>(lds_dyn + grid_lds_rec_bytes(sc));
        copy_grid_lds<R, grid_filter_x<R, ACC>()>(sc, grec, gcell, threadIdx.x, 64);
        stk.gcell = gcell;
        stk.grec = grec;
    } else {
        constexpr bool TOP = ACC == ACC_BVH_TRI_LDS;
        const WideLds l{TOP ? sc.tri_lds_nodes : sc.num_sphere_wide, min(sc.stack_entries, RT_BVH_STACK)};
        rt_u4* box = reinterpret_cast<rt_u4*>(lds_dyn + l.boxes());
        rt_u2* kid = reinterpret_cast<rt_u2*>(lds_dyn + l.kids());
        stage_wide_nodes(TOP ? sc.tri_wide : sc.sphere_wide, l.n, box, kid, threadIdx.x);
        stk = BvhStack{reinterpret_cast<int*>(lds_dyn + l.stacks()) + threadIdx.x, 64, box, kid};
        if constexpr (TOP) stk.ntop = l.n;
    }
    return stk;
}

}  // namespace

template <class R, int ACC>
__global__ __launch_bounds__(64) void aov_kernel(const SceneView<R> sc, const AovFrame f, float* __restrict__ guides,
                                                 int* __restrict__ kind_out, int* __restrict__ idx_out) {
    BvhStack stk{nullptr, 0};
    if constexpr (lds_form(ACC)) {
        extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
        stk = stage_walk_lds<R, ACC>(sc, lds_dyn);
        __syncthreads();
    } else {
        __shared__ int stack[RT_BVH_STACK * 64];
        stk = BvhStack{stack + threadIdx.x, 64};
    }
    const size_t r = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= (size_t)f.cw * (size_t)f.ch) return;
    const int cx = (int)(r % (size_t)f.cw), cy = (int)(r / (size_t)f.cw);
    float g[8];
    const AovHit h = aov_pixel<R, ACC>(sc, f.width, f.height, f.x0 + cx, f.height - 1 - (f.y0 + cy), stk, g);
    float4* out = reinterpret_cast<float4*>(guides + 8 * r);
    out[0] = make_float4(g[0], g[1], g[2], g[3]);
    out[1] = make_float4(g[4], g[5], g[6], g[7]);
    if (kind_out) kind_out[r] = h.kind;
    if (idx_out) idx_out[r] = h.idx;
}

template <class R>
hipError_t launch_aovs(const SceneView<R>& sc, bool bvh, const AovFrame& f, float* guides, int* kind, int* idx,
                       hipStream_t stream) {
    const size_t n = (size_t)f.cw * (size_t)f.ch;
    if (f.cw <= 0 || f.ch <= 0) return hipSuccess;
    // launch_closest_hits' selection: the walk of the kernel a pool launch of this scene runs, with the
    // process's knobs (the environment, read once)
    static const SelectKnobs knobs = knobs_from_env();
    const KernelChoice k = select_kernel<R>(scene_facts(sc), 0, bvh, true, knobs);
    SceneView<R> v = sc;
    if (k.acc == ACC_BVH_TRI_LDS) v.tri_lds_nodes = k.tri_lds_nodes;
    with_acc(k.acc, [&](auto tag) {
        constexpr int ACC = walk_of<plain_of(decltype(tag)::value)>();
        // one wave's share of the trace launch's dynamic LDS: the grid's copy, or the nodes and one stack
        const size_t lb = !lds_form(ACC) ? 0 : ACC == ACC_GRID_LDS ? k.lds_bytes
                        : WideLds{ACC == ACC_BVH_TRI_LDS ? v.tri_lds_nodes : v.num_sphere_wide,
                                  std::min(v.stack_entries, RT_BVH_STACK)}.bytes(1);
        hipLaunchKernelGGL((aov_kernel<R, ACC>), dim3((unsigned)((n + 63) / 64)), dim3(64), lb, stream, v, f, guides,
                           kind, idx);
    });
    return hipGetLastError();
}
template hipError_t launch_aovs<double>(const SceneView<double>&, bool, const AovFrame&, float*, int*, int*, hipStream_t);
template hipError_t launch_aovs<float>(const SceneView<float>&, bool, const AovFrame&, float*, int*, int*, hipStream_t);

// ---- the guided filter: one kernel per level, one thread per pixel ------------------------------------
// 32 x 8 pixel workgroups (four waves, each a 32 x 2 strip): a level's 25 taps per pixel are 32-byte guide
// records (two 16-byte loads) and 24-byte colours, reused across neighbouring threads through the caches.
__global__ __launch_bounds__(256) void guided_level_kernel(const GuidedLevel L, const double* __restrict__ in,
                                                           const float* __restrict__ guides, double* __restrict__ out) {
    const int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if (x >= L.w || y >= L.h) return;
    double o[3];
    guided_pixel(L, in, guides, x, y, o);
    double* dst = out + 3 * ((size_t)y * L.w + x);
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

hipError_t launch_guided_level(const GuidedLevel& L, const double* in, const float* guides, double* out, hipStream_t stream) {
    if (L.w <= 0 || L.h <= 0) return hipSuccess;
    hipLaunchKernelGGL(guided_level_kernel, dim3((unsigned)((L.w + 31) / 32), (unsigned)((L.h + 7) / 8)), dim3(32, 8), 0,
                       stream, L, in, guides, out);
    return hipGetLastError();
}

// ---- the variance-guided form: the same launch shape, colour and variance frames side by side ---------
// A level reads 48 bytes per tap (colour and variance) beside the 32-byte guide record, and the 3 x 3 variance
// prefilter is part of the level's kernel: its nine taps are the level-0 taps' cache lines.  Like
// guided_level_kernel it is bound by the binary64 exponentials, not by the loads, so there is no LDS tile.
__global__ __launch_bounds__(256) void vguided_level_kernel(const VGuidedLevel L, const double* __restrict__ cin,
                                                            const double* __restrict__ vin,
                                                            const float* __restrict__ guides, double* __restrict__ cout,
                                                            double* __restrict__ vout) {
    const int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if (x >= L.w || y >= L.h) return;
    double oc[3], ov[3];
    vguided_pixel(L, cin, vin, guides, x, y, oc, ov);
    const size_t p = 3 * ((size_t)y * L.w + x);
    cout[p] = oc[0]; cout[p + 1] = oc[1]; cout[p + 2] = oc[2];
    if (vout) {
        vout[p] = ov[0]; vout[p + 1] = ov[1]; vout[p + 2] = ov[2];
    }
}

hipError_t launch_vguided_level(const VGuidedLevel& L, const double* cin, const double* vin, const float* guides,
                                double* cout, double* vout, hipStream_t stream) {
    if (L.w <= 0 || L.h <= 0) return hipSuccess;
    hipLaunchKernelGGL(vguided_level_kernel, dim3((unsigned)((L.w + 31) / 32), (unsigned)((L.h + 7) / 8)), dim3(32, 8), 0,
                       stream, L, cin, vin, guides, cout, vout);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void mean_kernel(const double* __restrict__ sum, const int samples,
                                                   double* __restrict__ mean, const size_t n) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) mean[k] = sum[k] / (double)samples;
}

hipError_t launch_mean(const double* sum, int samples, double* mean, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sum, samples, mean, n);
    return hipGetLastError();
}

}  // namespace rt
