// wave_census.cpp — DEV TOOL (scripts/wave_census.py; tests/test_wave_census.py checks its structure).  Replays the
// schedule of pt_trace.hip's pool_item on the CPU for given 8x8 tiles — 64 lanes, items dealt in sample-major order,
// RT_DEFER_REGEN's deferred regeneration — over the kernel's own per-lane code (closest_hit_acc<double, ACC_GRID>,
// shade_segment<double, 0>, start_sample; built with -DRT_HOST_COUNTERS), and charges every phase of a loop trip to the
// wave twice: as SIMT runs it (the maximum over the lanes: a phase costs the wave what its slowest lane needs) and as
// the ideal (the sum over the lanes / 64).  ideal / SIMT is the lane efficiency the phase can reach at most; over all
// phases it models the kernel's measured lane utilization.  Nothing on the GPU reads this.
//
// Two views of the grid walk: by events (the iteration's maximum of each event count, as the shading phases) and
// stepped (the walk's loops as the device runs them: the dominant spheres, then cell by cell a filter loop over the
// cell's records and a loop over the filter's survivors, each trip charged while any lane is in it).  The stepped
// walk restates closest_hit_grid's traversal over the product's own filter and candidate functions; every closest hit
// it finds is compared with closest_hit_acc's (`mismatches`, which must stay 0).
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../blenderraytracer_amd/csrc/pt_path.h"
#include "../../blenderraytracer_amd/csrc/scene_pack.h"

using namespace rt;
namespace rt { unsigned long long rt_host_count[16]; }

namespace {

template <class R>
struct HostView {                  // the scene staged as rt_scene_create stages it (pt_hostcheck.cpp's)
    HostScene hs;
    HostRecords<R> rec;
    SceneView<R> v{};
    bool init(const rt_scene_desc* d) {
        std::string err;
        if (!pack_host(*d, hs, err)) return false;
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
        return true;
    }
};

// ---- the stepped walk's log of one lane's query ----
struct Survivor { bool disc, root2; };                        // a binary64 test: its discriminant passed, it took the second root
struct CellStep { int records; std::vector<Survivor> survivors; };
struct WalkLog {
    Survivor big[4];
    bool big_pass[4];
    std::vector<CellStep> steps;
    bool entered;
};

bool candidate_logged(const SphereRec<double>& s, V3<double> o, V3<double> d, double a, double tmin, double& t, bool away,
                      double ya, Survivor& sv) {
    auto& hc = rt::rt_host_count;
    const unsigned long long d0 = hc[HC_DISC_OK], r0 = hc[HC_SECOND_ROOT];
    const bool ok = sphere_candidate(s, o, d, a, tmin, t, away, ya);
    sv.disc = hc[HC_DISC_OK] != d0;
    sv.root2 = hc[HC_SECOND_ROOT] != r0;
    return ok;
}

// closest_hit_grid's traversal (pt_core.h), logging what each of its loops does for this lane
Closest<double> grid_logged(const SceneView<double>& sc, V3<double> o, V3<double> d, int origin, WalkLog& lg) {
    typedef double R;
    lg.steps.clear();
    lg.entered = false;
    const R tmin = 0.001;
    Closest<R> b{(R)INFINITY, HIT_NONE, 0, 0, -1};
    float tl = bvh_tlimit(b.t);
    const R a = dot(d, d), ya = root_rcp(a);
    const FilterRay fr = make_filter_ray(o, d);
    for (int k = 0; k < 4; ++k) { lg.big_pass[k] = false; lg.big[k] = Survivor{false, false}; }
    for (int k = 0; k < sc.num_big_spheres && k < 4; ++k) {
        const SphereLeaf<R> L = sc.big_spheres[k];
        if (!sphere_filter_pass(L.f, fr)) continue;
        lg.big_pass[k] = true;
        R t;
        if (!candidate_logged(L.s, o, d, a, tmin, t, true, ya, lg.big[k])) continue;
        if (better(t, L.obj, L.id, b)) { b = Closest<R>{t, HIT_SPHERE, L.id, L.mat, L.obj}; tl = bvh_tlimit(b.t); }
    }
    const GridRefs gp{sc.grid_n, sc.grid_lo, sc.grid_hi, sc.grid_cs, sc.grid_ics, sc.grid_far};
    const float of[3] = {(float)o.x, (float)o.y, (float)o.z}, df[3] = {(float)d.x, (float)d.y, (float)d.z};
    float inv[3], t0 = 0.0f, t1 = tl;
    for (int k = 0; k < 3; ++k) {
        float v = rt_rcp_approx(df[k]);
        if (!(fabsf(v) <= 0x1p126f)) v = copysignf(0x1p126f, df[k]);
        inv[k] = v;
        const float ta = (gp.lo[k] - of[k]) * v, tb = (gp.hi[k] - of[k]) * v;
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
    }
    if (!(t0 <= t1)) return b;
    lg.entered = true;
    int cell[3], step[3];
    float tmax[3];
    for (int k = 0; k < 3; ++k) {
        const float p = of[k] + t0 * df[k];
        int c = (int)floorf((p - gp.lo[k]) / gp.cs[k]);
        c = c < 0 ? 0 : (c >= gp.n[k] ? gp.n[k] - 1 : c);
        cell[k] = c;
        step[k] = df[k] > 0.0f ? 1 : (df[k] < 0.0f ? -1 : 0);
        tmax[k] = step[k] == 0 ? INFINITY : (gp.lo[k] + (float)(c + (step[k] > 0)) * gp.cs[k] - of[k]) * inv[k];
    }
    for (;;) {
        const int ci = cell[0] + gp.n[0] * (cell[1] + gp.n[1] * cell[2]);
        CellStep st;
        st.records = sc.grid_cell[ci + 1] - sc.grid_cell[ci];
        for (int k = sc.grid_cell[ci]; k < sc.grid_cell[ci + 1]; ++k) {
            const SphereLeaf<R> L = sc.grid_leaf[k];
            if (!sphere_filter_pass(L.f, fr)) continue;
            Survivor sv{false, false};
            R t;
            const bool ok = candidate_logged(L.s, o, d, a, tmin, t, L.id == origin, ya, sv);
            st.survivors.push_back(sv);
            if (ok && better(t, L.obj, L.id, b)) { b = Closest<R>{t, HIT_SPHERE, L.id, L.mat, L.obj}; tl = bvh_tlimit(b.t); }
        }
        lg.steps.push_back(st);
        const int ax = tmax[0] <= tmax[1] ? (tmax[0] <= tmax[2] ? 0 : 2) : (tmax[1] <= tmax[2] ? 1 : 2);
        const float tx = tmax[ax];
        if (b.t < (R)tx || !(tx < INFINITY)) break;
        const int nc = cell[ax] + step[ax];
        if (nc < 0 || nc >= gp.n[ax]) break;
        cell[ax] = nc;
        tmax[ax] = (gp.lo[ax] + (float)(nc + (step[ax] > 0)) * gp.cs[ax] - of[ax]) * inv[ax];
    }
    return b;
}

// The trips a wave needs for its requesters' remaining rejection rounds `rem` when H lanes share them (a requester of
// rank r among S gets H div S + (r < H mod S) rounds per trip: RT_COOP_SPHERE's assignment); `shared`: the trips in
// which some lane evaluated another lane's round
void shared_trips(std::vector<int> rem, int H, double& trips, double& shared) {
    while (!rem.empty()) {
        const int S = (int)rem.size();
        if (H < S) H = S;
        trips += 1;
        if (H > S) shared += 1;
        std::vector<int> next;
        for (int r = 0; r < S; ++r) {
            const int c = H / S + (r < H % S);
            if (rem[r] > c) next.push_back(rem[r] - c);
        }
        rem.swap(next);
    }
}

}  // namespace

// the phases: by events (walk: cells .. root2; shading: hit .. miss; regeneration: regen, dround), then the stepped walk
enum Phase { P_CELLS, P_FILT, P_F64, P_DISC, P_ROOT2, P_HIT, P_SROUND, P_NORM, P_LAMB, P_METAL, P_DIEL, P_SCHLICK, P_MISS,
             P_REGEN, P_DROUND,
             W_SETUP, W_BIG_FILT, W_BIG_F64, W_BIG_DISC, W_BIG_ROOT2, W_ENTRY, W_STEP, W_FILT, W_SURV_F64, W_SURV_DISC,
             W_SURV_ROOT2, NP };
enum Extra { X_ITERS, X_ACTIVE, X_WAITING, X_REGENS, X_REGEN_LANES, X_SEGMENTS, X_REQUESTERS, X_ROUNDS, X_TRIPS_NOW,
             X_TRIPS_ALL_SHARED, X_SHARED_ALL_SHARED, X_TRIPS_FIRST_PLAIN, X_SHARED_FIRST_PLAIN,
             X_DISK_TRIPS_NOW, X_MAX_STEPS, X_LANE_STEPS, X_ENTERED, X_MISMATCHES, NX };

// cost[NP]: the slots of one event of each phase.  tiles_xy: the tiles' top-left pixels (full tiles of the frame of
// `s`); chunk samples per item; K = RT_DEFER_REGEN.  out[NP] SIMT slots, out[NP + ..] ideal slots, extra[NX].
extern "C" int wcs_census(const rt_scene_desc* d, const rt_settings* s, int ntiles, const int* tiles_xy, int chunk, int K,
                          const double* cost, double* out, double* extra) {
    HostView<double> hv;
    if (!hv.init(d)) return -1;
    const SceneView<double>& sc = hv.v;
    if (sc.num_grid_cells <= 0 || sc.num_tri_nodes != 0 || sc.num_big_spheres > 4) return -2;
    ImageParams im{};
    im.width = s->width; im.height = s->height; im.cw = s->width; im.ch = s->height;
    im.samples = s->samples; im.s_begin = 0; im.s_end = s->samples; im.max_depth = s->max_depth;
    im.aa_mode = s->aa_mode; im.seedm = host_seed_mix(s->seed);
    double simt[NP] = {0}, ideal[NP] = {0}, x[NX] = {0};
    auto& hc = rt::rt_host_count;
    auto charge = [&](int p, double worst, double total) { simt[p] += worst * cost[p]; ideal[p] += total / 64 * cost[p]; };
    for (int t = 0; t < ntiles; ++t) {
        const int x0 = tiles_xy[2 * t], y0 = tiles_xy[2 * t + 1];
        if (x0 < 0 || y0 < 0 || x0 + 8 > im.width || y0 + 8 > im.height) return -3;
        const uint32_t total = 64u * (uint32_t)chunk;
        int li[64], lj[64], depth[64], origin[64];
        uint32_t pk[64];
        Rng<double> g[64];
        V3<double> o[64], dd[64], T[64];
        bool live[64], waiting[64];
        std::vector<WalkLog> logs(64);
        Work w{};
        int stack[64];
        const BvhStack stk{stack, 1};
        auto begin_item = [&](int l, uint32_t k) {           // pool_item's begin_item; returns the lens disk's rounds
            const uint32_t m = k & 63, sr = k >> 6;
            const int px = x0 + (int)(m & 7), py = y0 + (int)(m >> 3);
            li[l] = px; lj[l] = im.height - 1 - py;
            pk[l] = pixel_key(im.seedm, (uint32_t)py * (uint32_t)im.width + (uint32_t)px);
            T[l] = mk<double>(1, 1, 1);
            depth[l] = im.max_depth;
            origin[l] = -1;
            const unsigned long long d0 = hc[HC_DISK_DRAW_ROUNDS];
            start_sample<double, false, 0>(sc, im, li[l], lj[l], pk[l], (int)sr, g[l], o[l], dd[l]);
            return (double)(hc[HC_DISK_DRAW_ROUNDS] - d0);
        };
        uint32_t next = 64;
        {
            double worst = 0, sum = 0;
            for (int l = 0; l < 64; ++l) {
                live[l] = true; waiting[l] = false;
                const double dr = begin_item(l, (uint32_t)l);
                worst = std::max(worst, dr); sum += dr;
            }
            charge(P_REGEN, 1, 64);
            charge(P_DROUND, worst, sum);
        }
        for (;;) {
            int nlive = 0;
            for (int l = 0; l < 64; ++l) nlive += live[l];
            if (!nlive) break;
            double mx[P_REGEN] = {0}, sm[P_REGEN] = {0};
            std::vector<int> A, rounds;
            int nwait = 0;
            for (int l = 0; l < 64; ++l) {
                if (!live[l]) continue;
                if (waiting[l]) { ++nwait; continue; }
                A.push_back(l);
                // the stepped walk's log first, its event counts taken back: the events are the product walk's
                unsigned long long c0[16];
                for (int k = 0; k < 16; ++k) c0[k] = hc[k];
                const Closest<double> cl = grid_logged(sc, o[l], dd[l], origin[l], logs[l]);
                for (int k = 0; k < 16; ++k) hc[k] = c0[k];
                double ev[P_REGEN] = {0};
                const unsigned n0 = w.nodes;
                const Closest<double> c = closest_hit_acc<double, ACC_GRID>(sc, o[l], dd[l], w, stk, false, origin[l]);
                if (c.kind != cl.kind || (c.kind != HIT_NONE && (c.idx != cl.idx || c.t != cl.t))) x[X_MISMATCHES] += 1;
                ev[P_CELLS] = w.nodes - n0;
                V3<double> L;
                const bool done = shade_segment<double, 0>(sc, c, o[l], dd[l], T[l], depth[l], g[l], L);
                origin[l] = !done && c.kind == HIT_SPHERE ? c.idx : -1;
                auto dl = [&](int k) { return (double)(hc[k] - c0[k]); };
                ev[P_FILT] = dl(HC_FILTER_TESTS); ev[P_F64] = dl(HC_F64_TESTS); ev[P_DISC] = dl(HC_DISC_OK);
                ev[P_ROOT2] = dl(HC_SECOND_ROOT); ev[P_HIT] = c.kind != HIT_NONE; ev[P_SROUND] = dl(HC_SPHERE_DRAW_ROUNDS);
                ev[P_NORM] = 1; ev[P_LAMB] = dl(HC_LAMBERT); ev[P_METAL] = dl(HC_METAL); ev[P_DIEL] = dl(HC_DIELECTRIC);
                ev[P_SCHLICK] = dl(HC_DIELECTRIC_SCHLICK); ev[P_MISS] = dl(HC_MISS);
                if (ev[P_SROUND] > 0) rounds.push_back((int)ev[P_SROUND]);
                x[X_SEGMENTS] += 1;
                for (int k = 0; k < P_REGEN; ++k) { mx[k] = std::max(mx[k], ev[k]); sm[k] += ev[k]; }
                waiting[l] = done;
            }
            if (!A.empty()) {
                const double na = (double)A.size();
                x[X_ITERS] += 1; x[X_ACTIVE] += na; x[X_WAITING] += nwait;
                for (int k = 0; k < P_REGEN; ++k) charge(k, mx[k], sm[k]);
                // the rejection loop: today's trips (the slowest lane's rounds) and the shared schemes'
                x[X_REQUESTERS] += (double)rounds.size();
                for (int r : rounds) x[X_ROUNDS] += r;
                x[X_TRIPS_NOW] += mx[P_SROUND];
                {
                    double tr = 0, sh = 0;
                    shared_trips(rounds, (int)A.size(), tr, sh);
                    x[X_TRIPS_ALL_SHARED] += tr;
                    x[X_SHARED_ALL_SHARED] += sh;
                    std::vector<int> rest;
                    for (int r : rounds) if (r > 1) rest.push_back(r - 1);
                    tr = rounds.empty() ? 0 : 1; sh = 0;
                    shared_trips(rest, (int)A.size(), tr, sh);
                    x[X_TRIPS_FIRST_PLAIN] += tr;
                    x[X_SHARED_FIRST_PLAIN] += sh;
                }
                // the stepped walk
                charge(W_SETUP, 1, na);
                for (int k = 0; k < 4; ++k) {
                    int np = 0, nd = 0, nr = 0;
                    for (int l : A) { np += logs[l].big_pass[k]; nd += logs[l].big[k].disc; nr += logs[l].big[k].root2; }
                    if (k < sc.num_big_spheres) charge(W_BIG_FILT, 1, na);
                    charge(W_BIG_F64, np > 0, np); charge(W_BIG_DISC, nd > 0, nd); charge(W_BIG_ROOT2, nr > 0, nr);
                }
                size_t most = 0;
                for (int l : A) {
                    x[X_ENTERED] += logs[l].entered;
                    most = std::max(most, logs[l].steps.size());
                    x[X_LANE_STEPS] += (double)logs[l].steps.size();
                }
                charge(W_ENTRY, 1, na);
                x[X_MAX_STEPS] += (double)most;
                for (size_t j = 0; j < most; ++j) {
                    int in_step = 0, worst_records = 0, records = 0;
                    size_t worst_surv = 0;
                    for (int l : A)
                        if (logs[l].steps.size() > j) {
                            ++in_step;
                            worst_records = std::max(worst_records, logs[l].steps[j].records);
                            records += logs[l].steps[j].records;
                            worst_surv = std::max(worst_surv, logs[l].steps[j].survivors.size());
                        }
                    charge(W_STEP, 1, in_step);
                    charge(W_FILT, worst_records, records);
                    for (size_t r = 0; r < worst_surv; ++r) {
                        int nf = 0, nd = 0, nr = 0;
                        for (int l : A)
                            if (logs[l].steps.size() > j && logs[l].steps[j].survivors.size() > r) {
                                ++nf; nd += logs[l].steps[j].survivors[r].disc; nr += logs[l].steps[j].survivors[r].root2;
                            }
                        charge(W_SURV_F64, 1, nf); charge(W_SURV_DISC, nd > 0, nd); charge(W_SURV_ROOT2, nr > 0, nr);
                    }
                }
            }
            int need = 0, tracing = 0;
            for (int l = 0; l < 64; ++l) if (live[l]) { need += waiting[l]; tracing += !waiting[l]; }
            if (need && (need >= K || tracing == 0)) {       // pool_item's deferred regeneration
                int rank = 0, started = 0;
                double worst = 0, sum = 0;
                for (int l = 0; l < 64; ++l)
                    if (live[l] && waiting[l]) {
                        const uint32_t k = next + (uint32_t)rank++;
                        live[l] = k < total;
                        if (live[l]) {
                            const double dr = begin_item(l, k);
                            worst = std::max(worst, dr); sum += dr; ++started;
                        }
                        waiting[l] = false;
                    }
                next += (uint32_t)need;
                if (started) {
                    x[X_REGENS] += 1; x[X_REGEN_LANES] += started; x[X_DISK_TRIPS_NOW] += worst;
                    charge(P_REGEN, 1, started);
                    charge(P_DROUND, worst, sum);
                }
            }
        }
    }
    for (int k = 0; k < NP; ++k) { out[k] = simt[k]; out[NP + k] = ideal[k]; }
    for (int k = 0; k < NX; ++k) extra[k] = x[k];
    return 0;
}
