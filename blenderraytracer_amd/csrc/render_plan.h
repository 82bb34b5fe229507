// render_plan.h — what a render (rt_render, rt_render_resume: rt_capi.cpp render_impl) will do, decided
// before anything is enqueued: its batches, which device traces which, how they are queued, the pool
// chunk of every launch and the error estimate's group counts.  plan_render is a pure function of its
// input and of the answers of `fit` (does this buffer fit this device?): no HIP call and no scene, so
// tests/hostcheck enumerates it on the CPU (tests/test_render_plan.py).  A new mode is a field here.
//
// rt_render and rt_render_resume: trace samples [first, sample_end) on top of `sums_in` (NULL: zeros;
// `resident`: the sums the scene's home device already holds, its checkpoint).
//
// Batches (rt_settings.batch_samples) are pipelined: batch k+1 is enqueued before the host waits for
// batch k, so the GPU never idles on the host's progress call.  With the sample pool and more than one
// batch, consecutive batches also trace on two streams into their own chunk partials (trace_overlapped):
// the next batch's waves fill the CUs while the previous one drains, and the reduces add the partials in
// batch order, so the sums are bit-identical to running the batches one after the other (and to a
// checkpoint + resume at any batch boundary).  A cancel (progress() returning non-zero, rt_cancel) stops
// the overlapped batches at their next (tile, chunk) item — a wave's item, about a millisecond — and
// the checkpoint is the batches fully reduced by then (`gated`); without overlapped batches it is
// observed after a batch, and the batches already queued complete.  Several devices: whole batches
// round-robin (trace_replica), or every batch split over the devices (merge_shards).
// rt_settings.batch_samples = -N: about N progress batches whose size is a multiple of the sample pool's
// chunk for the render (its rule for the whole sample range [sample_begin, samples), as for one device), so
// that every batch's items are the one-batch render's items.  Batches of ceil(S / N) samples otherwise cut
// the chunks: mesh50k (chunk 12) in 16 batches of 16 spp takes one 16-sample chunk per batch, +4 % against
// one batch.  The resolution depends only on the settings and the scene, so a resume sees
// the same batches.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "pool_plan.h"

namespace rt {

// Batches in flight per render: kSlots partial slots / trace streams per device; the host queues up to
// kSlots batches per device beyond the one it waits for (lookahead()), each with its own preview staging
// and completion event (lookahead() + kSlots of them, so a queued batch never writes a frame the host has
// not read yet).
constexpr int kSlots = 3;
inline int lookahead(int devices) { return kSlots * std::max(1, devices); }
constexpr int kMaxFused = 64;      // batches of one fused launch (one flag word each)

// Shard k of the sample range [b, e) over n shards (contiguous, sizes differ by at most one).
inline void shard_range(int b, int e, int k, int n, int& sb, int& se) {
    const long long len = e - b;
    sb = b + (int)(len * k / n);
    se = b + (int)(len * (k + 1) / n);
}

// the A/B switches of the environment, read once per process
struct RenderKnobs {
    bool overlap = true;          // RT_OVERLAP=0: batches one after the other
    bool item_cancel = true;      // RT_ITEM_CANCEL=0: no cancel word for the kernels
    bool fused_batches = true;    // RT_FUSED_BATCHES=0: one launch per batch
    bool fused_preview = false;   // RT_FUSED_PREVIEW=1: a fused batch's reduce and running frame in one kernel
};
inline const RenderKnobs& render_knobs() {
    static const RenderKnobs k = [] {   // thread-safe initialization
        const auto is = [](const char* name, char c) { return getenv(name) && getenv(name)[0] == c; };
        return RenderKnobs{!is("RT_OVERLAP", '0'), !is("RT_ITEM_CANCEL", '0'), !is("RT_FUSED_BATCHES", '0'),
                           is("RT_FUSED_PREVIEW", '1')};
    }();
    return k;
}

struct RenderPlanIn {
    int cw, ch;
    int sample_begin, sample_end, samples, batch_samples, max_depth;   // rt_settings (checked)
    bool pool;                    // the sample pool traces (rt_settings.sum_order, RT_SAMPLE_POOL)
    int first;                    // the first sample to trace (a resume: the samples the sums hold)
    bool tri_bvh;
    int shards;                   // device states of the render
    bool home_first;              // shard 0 is the scene's home state
    bool want_segs, want_draws, want_preview;   // outputs asked for
    bool err_active;              // this render starts or continues an error estimate, from err_groups
    int err_groups;               // chunk partials per pixel
    RenderKnobs knobs;
};

// a question to `fit`: kSlots partial slots of `bytes` each, or the fused buffers of `batches` batches of
// `doubles` doubles, on shard `shard`'s device
struct FitAsk {
    enum Kind { Slots, Fused } kind;
    int shard;
    size_t bytes, doubles;
    int batches;
};

enum class DeviceMode { One, Whole, Split };          // one device; whole batches round-robin; every batch split
enum class QueueMode { Serial, Overlapped, Fused };   // batch after batch; on kSlots streams; in one launch

struct RenderPlan {
    int base = 0;                 // the sums hold samples [base, done) of every pixel
    int s0 = 0, s1 = 0;           // this render traces [s0, s1)
    int batch = 1, nb = 0;        // in nb batches of `batch` samples (the last may be short)
    DeviceMode devices = DeviceMode::One;
    QueueMode queue = QueueMode::Serial;
    bool gated = false;           // every batch's reduce behind a ReduceGate: a cancel stops at an item
    bool preview = false;         // running frames
    int ahead = kSlots;           // batches queued beyond the one the host waits for
    int ring = 2 * kSlots;        // completion events / preview frames
    int shards = 1;
    std::vector<int> chunk_hint;  // per shard: the pool chunk of its launches (0: the pool's own rule)
    std::vector<size_t> slot_bytes;   // per shard: bytes of each overlap slot asked for (0: none)
    int fchunk = 0;               // fused: every batch's chunk, and the doubles of one batch's partials
    size_t fdoubles = 0;
    std::vector<int> groups_after;    // the estimate: chunk partials per pixel once batch kb is in
    int err_chunk = 0;
    int final_groups = 0;         // ... once the render has finished (0 without an estimate)

    bool whole() const { return devices == DeviceMode::Whole; }
    bool overlap() const { return queue != QueueMode::Serial; }
    bool fused() const { return queue == QueueMode::Fused; }
    // the pool chunk of a launch of ns samples on shard k
    int batch_chunk(int k, int ns) const { return chunk_hint[k] > 0 ? std::max(1, std::min(chunk_hint[k], ns)) : 0; }
    int batch_begin(int kb) const { return s0 + kb * batch; }
    int batch_end(int kb) const { return std::min(s1, s0 + (kb + 1) * batch); }
    // The launches of batch kb: one (on shard kb % shards), or with every batch split one per shard
    struct Piece { int begin, end, shard, chunk; };
    int pieces() const { return devices == DeviceMode::Split ? shards : 1; }
    Piece piece(int kb, int k) const {
        Piece q{batch_begin(kb), batch_end(kb), kb % shards, 0};
        if (devices == DeviceMode::Split) {
            q.shard = k;
            shard_range(batch_begin(kb), batch_end(kb), k, shards, q.begin, q.end);
        }
        q.chunk = fused() ? fchunk : batch_chunk(q.shard, q.end - q.begin);
        return q;
    }
    // shard k's part of the first batch (its scratch is sized by it), at least one sample
    int first_share(int k) const {
        int b0, b1;
        shard_range(s0, s0 + std::min(batch, s1 - s0), k, shards, b0, b1);
        return std::max(1, b1 - b0);
    }
};

inline void sample_range(int sample_begin, int sample_end, int samples, int& base, int& end) {
    base = std::max(0, sample_begin);
    end = sample_end > 0 ? std::min(sample_end, samples) : samples;
}

// rt_settings.batch_samples = -steps resolved (see above)
inline int progress_batch(const RenderPlanIn& in, int steps) {
    int base, end;
    sample_range(in.sample_begin, in.sample_end, in.samples, base, end);
    const int total = std::max(1, end - base);
    const int target = std::max(1, (total + steps - 1) / steps);
    if (!in.pool) return target;
    const int h = pool_plan(in.cw, in.ch, total, in.tri_bvh).chunk;
    if (h <= 0 || h >= target) return target;
    return h * std::max(1, (int)std::lround((double)target / (double)h));
}

// A batch of B samples is split into round(B / h) equal chunks (at least one), h being the pool's
// rule for the render's whole share: min(h, B)-sample chunks left a short remainder chunk in every
// batch (mesh50k in 16 batches of 16 spp: chunks of 12 + 4, 77.2 ms vs 75.0 ms as one 16-sample
// chunk).  B is the batch setting, not the samples left, so a resume sees the same chunks.
inline int balanced_chunk(int h, int b) {
    if (h <= 0 || b <= 0) return h;
    const int n = std::max(1, (int)std::lround((double)b / (double)h));
    return (b + n - 1) / n;
}

// fit(const FitAsk&) -> bool: whether the buffers fit the shard's device (rt_capi.cpp: it allocates them).
// A "no" downgrades the plan (whole -> split, overlapped -> serial, fused -> a launch per batch); the
// devices are asked in shard order, and a "no" ends the asking of that kind.
template <class Fit>
RenderPlan plan_render(const RenderPlanIn& in, Fit&& fit) {
    RenderPlan p;
    const int cw = in.cw, ch = in.ch, nsh = in.shards;
    const int setting = in.batch_samples < 0 ? progress_batch(in, -in.batch_samples) : in.batch_samples;
    int end;
    sample_range(in.sample_begin, in.sample_end, in.samples, p.base, end);
    const int base = p.base, s0 = p.s0 = std::max(base, in.first), s1 = p.s1 = std::max(end, s0);
    p.shards = nsh;
    p.slot_bytes.assign(nsh, 0);
    // Several devices with the sample pool: whole batches round-robin (batch k on states[k % nsh],
    // trace_replica), at least one batch per device — the batch size counts from sample_begin, so a
    // resume at a batch boundary sees the same batches.  Every batch's pool waves take min(batch, chunk)
    // samples, chunk being the pool's rule for the whole render (as one device's batches do), so the
    // sums are bit-identical to the same batches on one device.
    bool whole = nsh > 1 && in.pool && in.max_depth > 0 && in.knobs.overlap && s1 > s0;
    int whole_batch = 0, whole_chunk = 0;
    if (whole) {
        const int full = setting > 0 ? setting : std::max(1, s1 - base);
        whole_batch = std::max(1, std::min(full, (s1 - base + nsh - 1) / nsh));
        whole_chunk = balanced_chunk(pool_plan(cw, ch, std::max(1, s1 - base), in.tri_bvh).chunk, whole_batch);
        const int ns = std::min(whole_batch, s1 - s0);
        const size_t bytes = pool_plan(cw, ch, ns, in.tri_bvh, std::min(whole_chunk, ns)).part_bytes;
        for (int k = 0; k < nsh && whole; ++k) {    // every device's partial slots must fit, else split batches
            whole = fit(FitAsk{FitAsk::Slots, k, bytes, 0, 0});
            p.slot_bytes[k] = bytes;
        }
        if (!whole) p.slot_bytes.assign(nsh, 0);
    }
    p.devices = nsh == 1 ? DeviceMode::One : whole ? DeviceMode::Whole : DeviceMode::Split;
    const int batch = p.batch = whole ? whole_batch : setting > 0 ? setting : std::max(1, s1 - s0);
    const int nb = p.nb = s1 > s0 ? (s1 - s0 + batch - 1) / batch : 0;
    p.preview = in.want_preview && nb > 1;
    // Several batches (split mode): every batch's pool waves take min(batch, chunk) samples, chunk being
    // the pool's rule for the shard's whole share of the render (not for one batch: short chunks lengthen
    // each wave's drain relative to its work), balanced over the shard's part of a full batch.  The same
    // batches give the same chunks on a resume (the share is counted from sample_begin), so a resumed
    // render stays bit-identical — also when the resume has a single batch left (the render as a whole,
    // from sample_begin, has several: before round 5 that batch took the pool's rule for its own
    // samples, 1-ulp differences in the resumed sums).
    p.chunk_hint.assign(nsh, whole ? whole_chunk : 0);
    if (in.pool && !whole && (nb > 1 || (setting > 0 && setting < s1 - base)))
        for (int k = 0; k < nsh; ++k) {
            int a, b, fa, fb;
            shard_range(base, s1, k, nsh, a, b);
            shard_range(0, batch, k, nsh, fa, fb);
            p.chunk_hint[k] = balanced_chunk(pool_plan(cw, ch, std::max(1, b - a), in.tri_bvh).chunk, fb - fa);
        }
    // overlapped batches: the pool with several batches (always in whole-batch mode).  Not with per-pixel
    // counters over a split of every batch: the trace kernels add those directly, and a replica's merge
    // zeroes them between batches
    bool overlap = whole || (in.knobs.overlap && in.pool && nb > 1 && in.max_depth > 0 &&
                             !(nsh > 1 && (in.want_segs || in.want_draws)));
    for (int k = 0; k < nsh && !whole && overlap; ++k) {
        const int ns = p.first_share(k);
        p.slot_bytes[k] = pool_plan(cw, ch, ns, in.tri_bvh, p.batch_chunk(k, ns)).part_bytes;
        overlap = fit(FitAsk{FitAsk::Slots, k, p.slot_bytes[k], 0, 0});
    }
    if (!overlap) p.slot_bytes.assign(nsh, 0);
    p.ahead = whole ? lookahead(nsh) : kSlots;
    p.ring = p.ahead + kSlots;
    // A cancel inside a batch: the pool kernels read the cancel word before every item, and a batch with
    // untraced items is never reduced (ReduceGate), nor is any batch after it, so the sums always hold
    // the batches [0, k) for some k.  For batches reduced on one stream in batch order: one device, or
    // the whole-batch split.  The split of every batch over devices observes a cancel between batches.
    // (RT_ITEM_CANCEL=0 with fused batches: the gates run, the kernels poll no cancel word — A/B only)
    p.gated = (in.knobs.item_cancel || (in.knobs.fused_batches && nsh == 1)) && overlap && (nsh == 1 || whole);
    // Fused batches (one device, overlapped gated batches): every batch in ONE pool launch, its items
    // batch-major in the pool's queue (launch_trace_batches: the same items, chunks and partials as one
    // launch per batch), and each batch's reduce enqueued by the host once the batch's last item has
    // raised its flag — the persistent workgroups never drain between batches (16 batches of config 3
    // drained for 3.5 % of the trace time).  The reduces (16 VGPRs) and the preview frames (gamma
    // thresholds, 29 VGPRs) run beside the trace waves, which leave 32 of a SIMD's 512 VGPRs free.
    // Several devices (the whole-batch split): device d traces its batches k = d, d + N, ... in one launch
    // (ImageParams::batch_ways), raising batch k's flag; the host then copies that batch's partials to
    // the home device and reduces them there in batch order — the copies and reduces of trace_replica,
    // from one launch per device instead of one per batch.
    bool fused = in.knobs.fused_batches && p.gated && nb > 1 && nb <= kMaxFused && (whole || (nsh == 1 && in.home_first));
    if (fused) {
        p.fchunk = p.batch_chunk(0, batch);
        p.fdoubles = fused_batch_doubles(cw, ch, batch, in.tri_bvh, p.fchunk);
        for (int d = 0; d < nsh && fused; ++d) fused = fit(FitAsk{FitAsk::Fused, d, 0, p.fdoubles, (nb - d + nsh - 1) / nsh});
    }
    p.queue = fused ? QueueMode::Fused : overlap ? QueueMode::Overlapped : QueueMode::Serial;
    p.groups_after.assign(nb, 0);
    if (in.err_active) {
        int g = in.err_groups;
        for (int kb = 0; kb < nb; ++kb) {
            const int ns = p.batch_end(kb) - p.batch_begin(kb);
            const PoolPlan pp = pool_plan(cw, ch, ns, in.tri_bvh, fused ? p.fchunk : p.batch_chunk(whole ? kb % nsh : 0, ns));
            if (kb == 0) p.err_chunk = pp.chunk;
            p.groups_after[kb] = g += pp.chunks;
        }
        p.final_groups = g;
    }
    return p;
}

}  // namespace rt
