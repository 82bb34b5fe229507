// kernel_select.h — which trace kernel a launch runs: the one selection behind launch_trace, _partials,
// _batches and _bands, rt_closest_hits and rt_scene_walk (pt_trace.hip), with the occupancy constants and
// the LDS layout its budget arithmetic needs.  select_kernel is a pure function of what the scene has, the
// launch and the knobs: no HIP call, no environment read, so tests/hostcheck pins it on the CPU
// (tests/test_walk_select.py).  A new kernel family is one enumerator (pt_core.h Accel) and one line here.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "pt_core.h"

namespace rt {

// ---- occupancy: waves per SIMD of each kernel (its __launch_bounds__), waves per LDS workgroup ----
// One wave (an 8x8 pixel tile) per workgroup: one-wave workgroups measured fastest (RTOW f64 4350 vs
// 4190 Msamples/s for 16x16 tiles, mesh50k 3342 vs 3094): finer work items shorten the frame's tail.
#ifndef RT_MIN_WAVES_PER_SIMD
#define RT_MIN_WAVES_PER_SIMD 6   // brute force: 80 VGPRs.  At 8 waves (64 VGPRs) the binary64 pool kernel
#endif                            // spills 300 B/lane: Cornell f64 5175 (8) / 6730 (4) / 6830 (6) Msamples/s,
                                  // f32 9274 (8) / 9680 (4) / 9978 (6)
#ifndef RT_BVH_WAVES_PER_SIMD
#define RT_BVH_WAVES_PER_SIMD 4   // binary64 BVH walk: 128 VGPRs (measured 3/4/5 waves: 5405/5462/5092)
#endif
#ifndef RT_BVH_WAVES_F32
#define RT_BVH_WAVES_F32 5        // binary32 BVH walk: 96 VGPRs (measured 4/5/6 waves: 6070/6628/6542)
#endif

#ifndef RT_SPHERES_WAVES_PER_SIMD
#define RT_SPHERES_WAVES_PER_SIMD 5   // binary64 sphere-only walk (ACC_BVH_SPHERES): 96 VGPRs, 13 spilled to
#endif                                // scratch in cold paths; RTOW 128 spp 4 / 5 waves: 7119 / 7335 Msamples/s
#ifndef RT_SPHERES_WAVES_F32
#define RT_SPHERES_WAVES_F32 6       // binary32 sphere-only walk: 80 VGPRs (5 / 6 waves: 8536 / 8800 RTOW f32)
#endif

#ifndef RT_LDS_OCC_F64
#define RT_LDS_OCC_F64 4          // waves/SIMD of the LDS-node kernel (trace_pool_lds_kernel)
#endif
#ifndef RT_LDS_OCC_F32
#define RT_LDS_OCC_F32 6
#endif

#ifndef RT_GRID_WAVES_PER_SIMD
#define RT_GRID_WAVES_PER_SIMD 5
#endif
#ifndef RT_GRID_WAVES_F32
#define RT_GRID_WAVES_F32 6
#endif

template <class R, int ACC>
constexpr int waves_per_simd() {
    if constexpr (ACC == ACC_GRID || ACC == ACC_GRID_LDS || ACC == ACC_GRID_LDS_LEAN)
        return sizeof(R) == 8 ? RT_GRID_WAVES_PER_SIMD : RT_GRID_WAVES_F32;
    if constexpr (ACC == ACC_BVH_SPHERES) return sizeof(R) == 8 ? RT_SPHERES_WAVES_PER_SIMD : RT_SPHERES_WAVES_F32;
    if constexpr (ACC == ACC_BVH_SPHERES_LDS) return sizeof(R) == 8 ? RT_LDS_OCC_F64 : RT_LDS_OCC_F32;
    if constexpr (ACC == ACC_BVH_TRI_LDS) return sizeof(R) == 8 ? RT_BVH_WAVES_PER_SIMD : RT_BVH_WAVES_F32;
    // (the textured kernels take their walks' occupancy: texture_value is out of line)
    return walk_of<ACC>() >= ACC_BVH ? (sizeof(R) == 8 ? RT_BVH_WAVES_PER_SIMD : RT_BVH_WAVES_F32) : RT_MIN_WAVES_PER_SIMD;
}

// Waves per workgroup of the LDS pool kernels: a multiple of 4, so that every workgroup puts the same
// number of waves on each SIMD (10-wave workgroups at 5 waves/SIMD left one SIMD a wave short of the
// second workgroup: one workgroup per CU, RTOW -28 %)
#ifndef RT_LDS_WAVES_F64
#define RT_LDS_WAVES_F64 8        // 2 workgroups per CU at 4 waves/SIMD
#endif
#ifndef RT_LDS_WAVES_F32
#define RT_LDS_WAVES_F32 12       // 2 workgroups per CU at 6 waves/SIMD
#endif
// the grid's LDS kernel (ACC_GRID_LDS) holds no stacks: smaller workgroups, each with its own copy
#ifndef RT_GRID_LDS_WAVES_F64
#define RT_GRID_LDS_WAVES_F64 4   // 5 workgroups per CU at 5 waves/SIMD
#endif
#ifndef RT_GRID_LDS_WAVES_F32
#define RT_GRID_LDS_WAVES_F32 12  // 2 workgroups per CU at 6 waves/SIMD (8: 3 per CU, -0.7 %)
#endif
// the triangle tree's LDS kernel (ACC_BVH_TRI_LDS): one workgroup per CU at 4 waves/SIMD, so that the
// CU's one copy of the top levels is as large as its LDS allows beside the 16 waves' stacks and partials
// (binary32, 5 waves/SIMD: 4-wave workgroups, five copies per CU)
#ifndef RT_TRI_LDS_WAVES_F64
#define RT_TRI_LDS_WAVES_F64 16
#endif
#ifndef RT_TRI_LDS_WAVES_F32
#define RT_TRI_LDS_WAVES_F32 4
#endif
template <class R, int ACC = ACC_BVH_SPHERES_LDS>
constexpr int lds_waves() {
    if constexpr (ACC == ACC_GRID_LDS || ACC == ACC_GRID_LDS_LEAN) return sizeof(R) == 8 ? RT_GRID_LDS_WAVES_F64 : RT_GRID_LDS_WAVES_F32;
    if constexpr (ACC == ACC_BVH_TRI_LDS) return sizeof(R) == 8 ? RT_TRI_LDS_WAVES_F64 : RT_TRI_LDS_WAVES_F32;
    return sizeof(R) == 8 ? RT_LDS_WAVES_F64 : RT_LDS_WAVES_F32;
}

// ---- the wide-node LDS block of the LDS kernels: [child boxes 48 B x n][child references 8 B x n]
// [per wave: a stack of `entries` x 64 ints]; byte offsets into the workgroup's dynamic LDS ----
struct WideLds {
    int n, entries;                // two-child nodes staged; stack entries per lane (the deepest leaf, <= RT_BVH_STACK)
    RT_HD int boxes() const { return 0; }
    RT_HD int kids() const { return 48 * n; }
    RT_HD int stacks() const { return 56 * n; }
    RT_HD size_t bytes(int waves) const { return (size_t)56 * n + (size_t)waves * entries * 64 * 4; }
};
// what a CU's 160 KiB of LDS leave each workgroup of kernel ACC, and what every LDS workgroup holds beside
// its dynamic part: the waves' 3 x 64 binary64 partials and 256 B of slack
template <class R, int ACC>
constexpr long long lds_budget(int fewer_workgroups = 0) {
    return 160 * 1024 / (4 * waves_per_simd<R, ACC>() / lds_waves<R, ACC>() - fewer_workgroups);
}
// RT_COOP_SPHERE: the binary64 lean grid kernel's waves also hold unit_sphere_point's hand-off slots (pt_path.h:
// 64 slots of 16 B per wave)
template <class R, int ACC>
constexpr long long coop_lds_bytes() {
    return RT_COOP_SPHERE && sizeof(R) == 8 && ACC == ACC_GRID_LDS_LEAN ? (long long)lds_waves<R, ACC>() * 64 * 16 : 0;
}
template <class R, int ACC>
constexpr long long lds_fixed_bytes() { return (long long)lds_waves<R, ACC>() * 3 * 64 * 8 + 256 + coop_lds_bytes<R, ACC>(); }

// ---- the knobs (A/B runs): compile-time defaults, overridden from the environment once per process ----
// Which sphere-only launches read the nodes from LDS: binary32 (RTOW 256 spp, 6 waves/SIMD: 9752 vs
// 9504 Msamples/s); binary64 only when asked (RT_LDS_NODES=2): RTOW's 481 nodes (27 KB) + 5 workgroups'
// stacks and partials exceed 160 KiB at 5 waves/SIMD, and at 4 the LDS kernel (7497) is slower than the
// one-wave kernel at 5 (7744; at 4: 7291).  RT_LDS_NODES=0: never (A/B).
#ifndef RT_LDS_NODES
#define RT_LDS_NODES 1
#endif
// Which grid launches read the grid from LDS (trace_pool_lds_kernel<.., ACC_GRID_LDS>): RT_LDS_GRID=0
// never (A/B), 1 (default) whenever the copy fits
#ifndef RT_LDS_GRID
#define RT_LDS_GRID 1
#endif
// RT_MAT_LDS (A/B): the grid LDS kernel also stages the material records in LDS (the budget check then
// counts them: fewer workgroups per CU when they do not fit beside the grid)
#ifndef RT_MAT_LDS
#define RT_MAT_LDS 0
#endif
// Which launches of scenes with a triangle tree run trace_pool_lds_kernel<.., ACC_BVH_TRI_LDS> (the top
// levels of the triangle tree in LDS): RT_LDS_TRI = 0 (default) never, 1 binary64, 2 both precisions.
// Measured (round 6, mesh50k 1080p x 128 spp f64, interleaved x2, identical images): the one-wave kernel
// 6915 / 6845 Msamples/s; the persistent kernel with 1019 / 255 / 64 top nodes in LDS 6360-6369 /
// 6319-6323 / 6238-6272, in 8-wave workgroups (507 nodes, two copies per CU) 6283-6336: the LDS nodes buy
// +1.8 % over the same kernel without them, the persistent form loses 9 % against hardware-dispatched
// one-wave workgroups (round 5's persistent one-wave kernel with per-XCD queues: -10 %) — DESIGN.md §4
#ifndef RT_LDS_TRI
#define RT_LDS_TRI 0
#endif
// The lean kernels (feat_of, pt_core.h) serve launches whose scene has the sky gradient, the perspective
// camera and supersampling AA, and the lean kernel's primitives: the grid's (ACC_GRID_LDS_LEAN) spheres
// alone, the triangle BVH walk's (ACC_BVH_STACK_LEAN) and World order's (ACC_BRUTE_LEAN) no boxes (World
// order: no triangles either).  RT_LEAN=0: never (A/B); 1 (default): all three; 2: the grid's only.
#ifndef RT_LEAN
#define RT_LEAN 1
#endif
// RT_BVH_WALK (A/B): skip = the stackless preorder walk, two = the general ordered walk, tree = the sphere
// tree even where the grid was chosen, grid = the grid wherever one was built; default: the ordered
// two-child walk, in its sphere-only form (or the grid, choose_walk) for scenes without triangles
constexpr int kWalkTree = -2;
inline int parse_bvh_walk(const char* e) {
    return e && !strncmp(e, "skip", 4) ? ACC_BVH : e && !strncmp(e, "two", 3) ? ACC_BVH_STACK
         : e && !strncmp(e, "grid", 4) ? ACC_GRID : e && !strncmp(e, "tree", 4) ? kWalkTree : ACC_BVH_SPHERES;
}
struct SelectKnobs {
    int bvh_walk = ACC_BVH_SPHERES;        // RT_BVH_WALK (parse_bvh_walk)
    int lean = RT_LEAN;
    int lds_grid = RT_LDS_GRID;
    int lds_nodes = RT_LDS_NODES;
    int lds_tri = RT_LDS_TRI;
    int tri_lds_nodes = RT_TRI_TOP_NODES;  // RT_TRI_LDS_NODES: at most this many triangle-tree nodes staged
};
// an integer knob of the environment (unset: def)
inline int env_int(const char* name, int def) {
    const char* e = getenv(name);
    return e ? atoi(e) : def;
}
inline SelectKnobs knobs_from_env() {
    SelectKnobs k;
    k.bvh_walk = parse_bvh_walk(getenv("RT_BVH_WALK"));
    k.lean = env_int("RT_LEAN", RT_LEAN);
    k.lds_grid = env_int("RT_LDS_GRID", RT_LDS_GRID);
    k.lds_nodes = env_int("RT_LDS_NODES", RT_LDS_NODES);
    k.lds_tri = env_int("RT_LDS_TRI", RT_LDS_TRI);
    k.tri_lds_nodes = std::max(0, std::min(env_int("RT_TRI_LDS_NODES", RT_TRI_TOP_NODES), RT_TRI_TOP_NODES));
    return k;
}

// ---- the selection ----
// what the decision reads of a SceneView
struct SceneFacts {
    int num_lights, num_tex, num_tri_nodes, num_tri_wide, num_sphere_wide, num_grid_cells, use_grid, num_planes,
        num_boxes, background, cam_ortho, stack_entries, num_mats;
    size_t grid_lds_bytes;         // the grid's LDS copy in this precision (pt_core.h grid_lds_bytes)
    int num_emitters;              // listed emitters of a render with emitter sampling
};
template <class R>
SceneFacts scene_facts(const SceneView<R>& sc) {
    return SceneFacts{sc.num_lights, sc.num_tex, sc.num_tri_nodes, sc.num_tri_wide, sc.num_sphere_wide, sc.num_grid_cells,
                      sc.use_grid, sc.num_planes, sc.num_boxes, sc.background, sc.cam_ortho, sc.stack_entries,
                      sc.num_mats, grid_lds_bytes(sc), sc.num_emitters};
}

constexpr int kAccelCount = ACC_BVH_STACK_NEE + 1;
// the kernels of trace_pool_lds_kernel (persistent multi-wave workgroups taking items from a queue, their
// walk's data staged in LDS); every other mode is a one-wave kernel
constexpr bool lds_form(int acc) {
    return acc == ACC_BVH_SPHERES_LDS || acc == ACC_GRID_LDS || acc == ACC_GRID_LDS_LEAN || acc == ACC_BVH_TRI_LDS;
}
// a lean mode's general twin: the same walk with nothing left out
constexpr int plain_of(int acc) {
    return acc == ACC_GRID_LDS_LEAN ? ACC_GRID_LDS : acc == ACC_BVH_STACK_LEAN ? ACC_BVH_STACK
         : acc == ACC_BRUTE_LEAN ? ACC_BRUTE : acc;
}
// rt_scene_walk's answer: 0 World order, 1 a tree, 2 the uniform grid
constexpr int walk_report(int acc) {
    return acc == ACC_BRUTE || acc == ACC_BRUTE_LEAN || acc == ACC_BRUTE_TEX || acc == ACC_BRUTE_LIT || acc == ACC_BRUTE_NEE ? 0
         : acc == ACC_GRID || acc == ACC_GRID_LDS || acc == ACC_GRID_LDS_LEAN ? 2 : 1;
}

struct KernelChoice {
    Accel acc;                     // the kernel's mode, LDS and lean forms included
    bool lds;                      // an LDS pool launch (lds_form(acc)), else a one-wave kernel
    size_t lds_bytes;              // lds: the launch's dynamic LDS (the one-wave kernels size their own stacks)
    int tri_lds_nodes;             // ACC_BVH_TRI_LDS: the launch's SceneView::tri_lds_nodes, else 0
};

// runtime mode -> compile-time tag: f(std::integral_constant<int, ACC>) of the mode `acc`
template <int A = 0, class F>
auto with_acc(int acc, F&& f) -> decltype(f(std::integral_constant<int, 0>{})) {
    if constexpr (A + 1 == kAccelCount) return f(std::integral_constant<int, A>{});
    else return acc == A ? f(std::integral_constant<int, A>{}) : with_acc<A + 1>(acc, f);
}

// bvh: walk the acceleration structures, else World order.  pool: a sample-pool launch, else the
// lane-per-pixel kernel, which has no lean or LDS form.
template <class R>
KernelChoice select_kernel(const SceneFacts& s, int aa_mode, bool bvh, bool pool, const SelectKnobs& k) {
    const auto one_wave = [](Accel acc) { return KernelChoice{acc, false, 0, 0}; };
    // emitter sampling, direct lighting, then procedural textures: the F_NEE / F_LIGHT / F_TEX kernels (World
    // order and the general ordered walk, one-wave forms only), whatever the walk choice and the knobs
    if (s.num_emitters > 0) return one_wave(bvh ? ACC_BVH_STACK_NEE : ACC_BRUTE_NEE);
    if (s.num_lights > 0) return one_wave(bvh ? ACC_BVH_STACK_LIT : ACC_BRUTE_LIT);
    if (s.num_tex > 0) return one_wave(bvh ? ACC_BVH_STACK_TEX : ACC_BRUTE_TEX);
    // the lean form of a kernel compiled for the primitives `feat`
    const auto lean = [&](int feat) {
        if (k.lean == 0 || (k.lean == 2 && feat != 0)) return false;
        return (s.num_planes == 0 || (feat & F_PLANES)) && (s.num_boxes == 0 || (feat & F_BOXES)) &&
               (s.num_tri_nodes == 0 || (feat & F_TRIS)) && s.background == 0 && !s.cam_ortho && aa_mode == 0;
    };
    // the walk: World order, or by the scene's primitives and RT_BVH_WALK — with triangles the general
    // ordered walk (skip: the stackless one); without, the grid where one was built and chosen
    // (choose_walk; grid: wherever built; tree: never), else the sphere-only ordered walk (skip / two: those)
    Accel walk = ACC_BRUTE;
    if (bvh && s.num_tri_nodes > 0) walk = k.bvh_walk == ACC_BVH ? ACC_BVH : ACC_BVH_STACK;
    else if (bvh && s.num_grid_cells > 0 && (k.bvh_walk == ACC_GRID || (k.bvh_walk == ACC_BVH_SPHERES && s.use_grid)))
        walk = ACC_GRID;
    else if (bvh) walk = k.bvh_walk == ACC_BVH || k.bvh_walk == ACC_BVH_STACK ? (Accel)k.bvh_walk : ACC_BVH_SPHERES;
    if (!pool) return one_wave(walk);
    // the walk's form in a pool launch
    const int entries = std::min(s.stack_entries, RT_BVH_STACK);
    if (walk == ACC_BRUTE && lean(feat_of<ACC_BRUTE_LEAN>())) return one_wave(ACC_BRUTE_LEAN);
    if (walk == ACC_GRID && k.lds_grid >= 1) {
        // the grid's cell offsets and records in LDS whenever the copy fits (RT_MAT_LDS: with the material
        // records, one workgroup per CU fewer)
        const size_t b = ((s.grid_lds_bytes + 15) & ~(size_t)15) + (RT_MAT_LDS ? sizeof(MatRec<R>) * (size_t)s.num_mats : 0);
        // (the lean form's fixed part is the larger in binary64, coop_lds_bytes: a copy that fits only without it
        // takes the general form)
        const long long budget = lds_budget<R, ACC_GRID_LDS>(RT_MAT_LDS ? 1 : 0);
        if (lean(feat_of<ACC_GRID_LDS_LEAN>()) && (long long)b + lds_fixed_bytes<R, ACC_GRID_LDS_LEAN>() <= budget)
            return KernelChoice{ACC_GRID_LDS_LEAN, true, b, 0};
        if ((long long)b + lds_fixed_bytes<R, ACC_GRID_LDS>() <= budget) return KernelChoice{ACC_GRID_LDS, true, b, 0};
    }
    // the sphere tree's nodes in LDS: binary32, binary64 only with RT_LDS_NODES=2, when the tree fits
    if (walk == ACC_BVH_SPHERES && k.lds_nodes >= (sizeof(R) == 8 ? 2 : 1) && s.num_sphere_wide > 0) {
        constexpr int W = lds_waves<R, ACC_BVH_SPHERES_LDS>();
        const size_t b = WideLds{s.num_sphere_wide, entries}.bytes(W);
        if ((long long)b + lds_fixed_bytes<R, ACC_BVH_SPHERES_LDS>() <= lds_budget<R, ACC_BVH_SPHERES_LDS>())
            return KernelChoice{ACC_BVH_SPHERES_LDS, true, b, 0};
    }
    if (walk == ACC_BVH_STACK) {
        // the triangle tree's top levels in LDS (RT_LDS_TRI = 1 binary64, 2 both): as many nodes of the
        // breadth-first prefix as fit the CU's LDS beside the workgroups' stacks and partials, at least 64
        if (k.lds_tri >= (sizeof(R) == 8 ? 1 : 2) && s.num_tri_wide > 0) {
            constexpr int W = lds_waves<R, ACC_BVH_TRI_LDS>();
            const long long fixed = (long long)W * entries * 64 * 4 + lds_fixed_bytes<R, ACC_BVH_TRI_LDS>();
            const long long n = std::min<long long>({(long long)s.num_tri_wide, (long long)k.tri_lds_nodes,
                                                     (lds_budget<R, ACC_BVH_TRI_LDS>() - fixed) / 56});
            if (n >= 64) return KernelChoice{ACC_BVH_TRI_LDS, true, WideLds{(int)n, entries}.bytes(W), (int)n};
        }
        if (lean(feat_of<ACC_BVH_STACK_LEAN>())) return one_wave(ACC_BVH_STACK_LEAN);
    }
    return one_wave(walk);
}

}  // namespace rt
