// pool_plan.h — the sample pool's split of a launch's samples into (8x8 tile, chunk) items and the bytes of
// their chunk partials.  Pure functions of the crop, the sample count and the scene's kind: no HIP call, so
// tests/hostcheck enumerates them on the CPU (tests/test_render_plan.py).  pt_trace.hip launches by them,
// render_plan.h plans a render's batches by them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace rt {

// chunk partial sums of one 8x8 tile: 3 channels x 64 pixels, binary64
constexpr size_t kPartialBytesPerTile = 3 * 64 * sizeof(double);

inline int crop_tiles(int cw, int ch) { return ((cw + 7) / 8) * ((ch + 7) / 8); }

// Samples per pool wave: ~2 sqrt(ns) (0.75 sqrt(ns) when the scene has a triangle BVH: its walks
// vary more in length, so shorter waves pay), for spheres doubled (up to ~4 sqrt(ns), <= 128) while
// the launch would have > 400k waves, halved (>= 4) until it has >= 64k waves (4x the chip's 16k wave slots).  Short waves shorten
// the frame's drain tail; long ones shorten each wave's own tail (its last items finish at different
// times) and write fewer chunk partials (each chunk is 24 B per pixel written and read back once).
// Measured (RTOW f64 Msamples/s): 1080p x 512 spp c45 / c90 7477 / 7436; x 256 c32 / c45 /
// c64 7363 / 7386 / 7295; x 128 c24 / c32 / c45 7330 / 7219 / 7156; x 64 c8 / c16 / c32 6720 / 7015 /
// 6947; 4K x 128 c23 / c45 7331 / 7393; mesh50k 256 spp c12 / c16 / c24 / c32 6786 / 6673 / 6687 /
// 6391; Cornell 512^2 x 64 spp (4096 tiles) 4.  RT_POOL_CHUNK overrides (A/B runs).
inline int pool_chunk(int ns, int tiles, bool tri_bvh) {
    static const int v = getenv("RT_POOL_CHUNK") ? std::max(1, atoi(getenv("RT_POOL_CHUNK"))) : 0;   // thread-safe initialization
    if (v) return v;
    int c = std::min(128, std::max(4, (int)((tri_bvh ? 0.75 : 2.0) * std::sqrt((double)ns) + 0.5)));
    const int cmax = tri_bvh ? c : std::min(128, std::max(4, (int)(4.0 * std::sqrt((double)ns) + 0.5)));
    while (c < cmax && (long long)tiles * ((ns + c - 1) / c) > 400000) c = std::min(cmax, c * 2);
    while (c > 4 && (long long)tiles * ((ns + c - 1) / c) < 65536) c = std::max(4, c / 2);
    return c;
}

// the sample pool's split of `ns` samples of a cw x ch crop: 8x8 tiles, samples per chunk, chunks and the
// bytes of all chunk partials of one launch (chunk > 0: that chunk instead of pool_chunk's)
struct PoolPlan { int tiles, chunk, chunks; size_t part_bytes; };
inline PoolPlan pool_plan(int cw, int ch, int ns, bool tri_bvh, int chunk = 0) {
    PoolPlan p{0, 0, 0, 0};
    if (cw <= 0 || ch <= 0 || ns <= 0) return p;
    p.tiles = crop_tiles(cw, ch);
    p.chunk = chunk > 0 ? chunk : pool_chunk(ns, p.tiles, tri_bvh);
    p.chunks = (ns + p.chunk - 1) / p.chunk;
    p.part_bytes = (size_t)p.chunks * p.tiles * kPartialBytesPerTile;
    return p;
}

// doubles of one batch's partials in a fused launch, and the items that complete it
inline size_t fused_batch_doubles(int cw, int ch, int batch, bool tri_bvh, int chunk) {
    return pool_plan(cw, ch, batch, tri_bvh, chunk).part_bytes / sizeof(double);
}
inline uint32_t fused_batch_items(int cw, int ch, int batch, bool tri_bvh, int chunk) {
    const PoolPlan p = pool_plan(cw, ch, batch, tri_bvh, chunk);
    return (uint32_t)((size_t)p.tiles * p.chunks);
}

}  // namespace rt
