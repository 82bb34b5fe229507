// coop_check.cpp — TEST INFRASTRUCTURE ONLY.  The wave-cooperative unit-sphere draw (RT_COOP_SPHERE: pt_core.h
// sphere_round, coop_rcp, coop_assign, coop_rounds, coop_pack, coop_take — the functions pt_path.h
// unit_sphere_point calls on the device) with a 64-lane wave emulated by plain loops in that function's order, against
// random_in_unit_sphere per lane.  The LDS slots are arrays; the ranks mbcnt gives are counted bits.
#include <cstdint>
#include <cstring>

#include "../../blenderraytracer_amd/csrc/pt_core.h"

using namespace rt;
#ifdef RT_HOST_COUNTERS
namespace rt { unsigned long long rt_host_count[16]; }
#endif

namespace {

inline uint32_t rank_below(uint64_t mask, int lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1)); }

struct WaveOut {
    uint32_t ux[64], uy[64], uz[64], k[64];
    uint32_t flags[64];      // 1: the point was a trip's last candidate of this lane (offset c - 1); 2: the first candidate
                             // (offset 0) of a trip after the lane's first; 4: the lane's own first round
    int trips, shared_rounds;
};

// mutation (what the tests must catch): 1 a helper evaluates the round one past its offset; 2 a requester that took
// nothing forgets k += 3 c; 3 the take rule accepts offset c too
void wave(uint64_t need_mask, uint64_t E, const uint32_t* key, const uint32_t* k0, int mutation, WaveOut& o) {
    bool need[64];
    int lane_trips[64] = {0};
    o.trips = 0;
    o.shared_rounds = 0;
    for (int l = 0; l < 64; ++l) {
        need[l] = (need_mask >> l & 1) != 0;
        o.ux[l] = o.uy[l] = o.uz[l] = 1u << 23;
        o.k[l] = k0[l];
        o.flags[l] = 0;
    }
    for (int l = 0; l < 64; ++l)
        if (need[l]) {
            need[l] = !sphere_round(key[l], o.k[l], o.ux[l], o.uy[l], o.uz[l]);
            o.k[l] += 3;
            if (!need[l]) o.flags[l] |= 4;
        }
    auto ballot = [&] { uint64_t m = 0; for (int l = 0; l < 64; ++l) if (need[l]) m |= 1ull << l; return m; };
    uint64_t N = ballot();
    while (N) {
        ++o.trips;
        const uint32_t n = (uint32_t)__builtin_popcountll(N), H = (uint32_t)__builtin_popcountll(E);
        const float rn = coop_rcp(n);
        unsigned long long stream[64], word[64];
        for (int l = 0; l < 64; ++l)
            if (need[l]) {
                const uint32_t rho = rank_below(N, l);
                stream[rho] = ((unsigned long long)o.k[l] << 32) | key[l];
                word[rho] = kCoopNone;
            }
        for (int l = 0; l < 64; ++l) {
            if (!(E >> l & 1)) continue;
            const CoopShare a = coop_assign(rank_below(E, l), n, rn);
            uint32_t hx, hy, hz;
            ++o.shared_rounds;
            if (sphere_round((uint32_t)stream[a.q], (uint32_t)(stream[a.q] >> 32) + 3 * (a.j + (mutation == 1 ? 1 : 0)), hx, hy, hz)) {
                const unsigned long long w = coop_pack(a.j, hx, hy);
                if (w < word[a.q]) word[a.q] = w;
            }
        }
        for (int l = 0; l < 64; ++l) {
            if (!need[l]) continue;
            const uint32_t rho = rank_below(N, l);
            const uint32_t c = coop_rounds(rho, H, n, rn) + (mutation == 3 ? 1 : 0);
            const uint32_t before = o.k[l];
            ++lane_trips[l];
            if (coop_take(word[rho], c, o.k[l], o.ux[l], o.uy[l])) {
                Rng<double> gz{key[l], o.k[l] - 1};
                o.uz[l] = gz.next_u24();
                need[l] = false;
                const uint32_t best = (o.k[l] - before) / 3 - 1;
                if (best == c - 1) o.flags[l] |= 1;
                if (best == 0 && lane_trips[l] > 1) o.flags[l] |= 2;
            } else if (mutation == 2) {
                o.k[l] = before;
                if (o.trips > 4096) return;       // (the mutant never ends where a lane's share holds no accepted round)
            }
        }
        N = ballot();
    }
}

inline double coord(uint32_t u) { return (double)((int)u - (1 << 23)) * 0x1p-23; }

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

// One wave: lanes of need_mask (a subset of exec_mask) draw a point.  out_p[64][3] the points (0 where none was
// asked), out_k[64] the draw counts afterwards, out_flags[64] (WaveOut), out_stats = {trips, shared rounds}
extern "C" int coc_wave(uint64_t need_mask, uint64_t exec_mask, const uint32_t* key, const uint32_t* k0, int mutation, double* out_p,
                        uint32_t* out_k, uint32_t* out_flags, int* out_stats) {
    if (need_mask & ~exec_mask) return -1;
    WaveOut o;
    wave(need_mask, exec_mask, key, k0, mutation, o);
    for (int l = 0; l < 64; ++l) {
        out_p[3 * l] = coord(o.ux[l]); out_p[3 * l + 1] = coord(o.uy[l]); out_p[3 * l + 2] = coord(o.uz[l]);
        out_k[l] = o.k[l];
        out_flags[l] = o.flags[l];
    }
    out_stats[0] = o.trips;
    out_stats[1] = o.shared_rounds;
    return 0;
}

// random_in_unit_sphere<double> for n streams: the points, the draw counts afterwards
extern "C" void coc_sequential(const uint32_t* key, const uint32_t* k0, long long n, double* out_p, uint32_t* out_k) {
    for (long long q = 0; q < n; ++q) {
        Rng<double> g{key[q], k0[q]};
        const V3<double> p = random_in_unit_sphere(g);
        out_p[3 * q] = p.x; out_p[3 * q + 1] = p.y; out_p[3 * q + 2] = p.z;
        out_k[q] = g.k;
    }
}

// `cases` random waves from `seed`: exec masks of every density (full, sparse, single lanes), need masks of every
// density within them, random keys and draw counts (near 2^32 too: k wraps as ++k does).  out = {lanes compared, lanes
// whose (x, y, z, k) differ from random_in_unit_sphere's bits or that changed without need, trips, waves whose trips
// (with the own first round) exceed the longest sequential loop, lanes taken at offset c - 1, lanes taken at a later trip's offset 0}
extern "C" void coc_random(long long cases, uint64_t seed, int mutation, long long* out) {
    uint64_t s = seed;
    long long lanes = 0, bad = 0, trips = 0, slow = 0, last = 0, first = 0;
    for (long long c = 0; c < cases; ++c) {
        auto mask = [&](uint64_t within) {
            const int mode = (int)(splitmix(s) % 6);
            uint64_t m = splitmix(s);
            if (mode == 0) m = ~0ull;
            else if (mode == 1) m &= splitmix(s);
            else if (mode == 2) m &= splitmix(s) & splitmix(s) & splitmix(s);
            else if (mode == 3) m = 1ull << (splitmix(s) & 63);
            else if (mode == 4) m |= splitmix(s) | splitmix(s);
            return m & within;
        };
        uint64_t E = mask(~0ull);
        if (!E) E = 1;
        const uint64_t need = mask(E);
        uint32_t key[64], k0[64];
        for (int l = 0; l < 64; ++l) {
            key[l] = (uint32_t)splitmix(s);
            const uint64_t r = splitmix(s);
            k0[l] = r % 8 == 0 ? 0xFFFFFFFFu - (uint32_t)(r >> 8) % 40 : (uint32_t)(r >> 8) % 200;
        }
        WaveOut o;
        wave(need, E, key, k0, mutation, o);
        int longest = 0;
        for (int l = 0; l < 64; ++l) {
            ++lanes;
            if (need >> l & 1) {
                Rng<double> g{key[l], k0[l]};
                const V3<double> p = random_in_unit_sphere(g);
                const double q[3] = {coord(o.ux[l]), coord(o.uy[l]), coord(o.uz[l])}, e[3] = {p.x, p.y, p.z};
                if (std::memcmp(q, e, sizeof(q)) != 0 || o.k[l] != g.k) ++bad;
                longest = longest > (int)((g.k - k0[l]) / 3) ? longest : (int)((g.k - k0[l]) / 3);
            } else if (o.k[l] != k0[l] || o.ux[l] != 1u << 23 || o.uy[l] != 1u << 23 || o.uz[l] != 1u << 23) {
                ++bad;
            }
            last += (o.flags[l] & 1) != 0;
            first += (o.flags[l] & 2) != 0;
        }
        trips += o.trips;
        slow += o.trips + 1 > longest && longest > 0;
    }
    out[0] = lanes; out[1] = bad; out[2] = trips; out[3] = slow; out[4] = last; out[5] = first;
}

// the number of rounds random_in_unit_sphere takes on each of n streams
extern "C" void coc_rounds(const uint32_t* key, const uint32_t* k0, long long n, int* out) {
    for (long long q = 0; q < n; ++q) {
        Rng<double> g{key[q], k0[q]};
        random_in_unit_sphere(g);
        out[q] = (int)((g.k - k0[q]) / 3);
    }
}

// coop_assign and coop_rounds against integer division for every h, H <= 64 and n in [1, 64], with the reciprocal the
// host computes and with it moved by up to two ulps either way (the device's v_rcp_f32 is within one): violations
extern "C" int coc_assign_check() {
    int bad = 0;
    for (uint32_t n = 1; n <= 64; ++n)
        for (int ulps = -2; ulps <= 2; ++ulps) {
            float rn = coop_rcp(n);
            uint32_t bits;
            std::memcpy(&bits, &rn, 4);
            bits += (uint32_t)ulps;
            std::memcpy(&rn, &bits, 4);
            for (uint32_t h = 0; h <= 64; ++h) {
                const CoopShare a = coop_assign(h, n, rn);
                bad += a.j != h / n || a.q != h % n;
                for (uint32_t rho = 0; rho < n; ++rho) bad += coop_rounds(rho, h, n, rn) != h / n + (rho < h % n ? 1u : 0u);
            }
        }
    return bad;
}
