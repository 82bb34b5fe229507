// pt_error.hip — the error estimate's kernels (pt_error.h): the chunk moments after every batch's reduce, the
// per-pixel estimate with its per-tile partial sums, and the frame's figures.  One-wave workgroups like
// reduce_kernel (pt_trace.hip): they run beside the trace waves, which leave 32 VGPRs per SIMD lane free.
#include "pt_error.h"

#include "pool_order.h"
#include "pt_launch.h"

namespace rt {

// q[3 pix + ch] += S_c² / n_c in chunk order; one thread per pixel, one one-wave workgroup per tile, the
// indexing of reduce_kernel (its `skip` word and tile0 too)
__global__ __launch_bounds__(64) void error_moments_kernel(const ImageParams im, double* __restrict__ q,
                                                           const double* __restrict__ part, const int tiles,
                                                           const int chunks, const int chunk, const int ns,
                                                           const uint32_t* __restrict__ skip, const int tile0) {
    const int tile = tile0 + (int)blockIdx.x, m = threadIdx.x;
    if (tile >= tiles || (skip && *skip)) return;
    const Tile t = tile_of(im, tile);
    if (m >= t.nv) return;
    const size_t px = (size_t)(t.y0 + m / t.vw) * im.cw + (t.x0 + m % t.vw);
    const size_t stride = (size_t)tiles * 3 * 64;
    // a channel at a time (not unrolled): one binary64 division in flight, 32 VGPRs
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        const double* p = part + (size_t)tile * 3 * 64 + 64 * k + m;
        double a = q[3 * px + k];
#pragma unroll 1
        for (int c = 0; c < chunks; ++c, p += stride) a = error_moment_add(a, *p, error_group_samples(chunk, ns, c));
        q[3 * px + k] = a;
    }
}

// The estimate of every pixel of a tile and the tile's partial sums.  Lanes beyond the tile's pixels take part
// in the tree with zeros.
__global__ __launch_bounds__(64) void error_tile_kernel(const ImageParams im, const double* __restrict__ sum,
                                                        const double* __restrict__ q, const int groups, const int samples,
                                                        double* __restrict__ var_mean, float* __restrict__ rel_error,
                                                        double* __restrict__ tile_part, const uint32_t* __restrict__ skip) {
    __shared__ double se[64], sm[64], sb[64];
    const int tile = blockIdx.x, m = threadIdx.x;
    if (skip && *skip) return;                    // wave-uniform
    const Tile t = tile_of(im, tile);
    double e = 0.0, bad = 0.0;
    if (m < t.nv) {
        const size_t px = (size_t)(t.y0 + m / t.vw) * im.cw + (t.x0 + m % t.vw);
        const double r = error_pixel(sum + 3 * px, q + 3 * px, groups, samples, var_mean ? var_mean + 3 * px : nullptr);
        if (rel_error) rel_error[px] = (float)r;
        if (error_finite(r)) e = r;
        else bad = 1.0;
    }
    if (!tile_part) return;                       // wave-uniform
    se[m] = e; sm[m] = e; sb[m] = bad;
    __syncthreads();
    for (int off = 32; off >= 1; off >>= 1) {
        if (m < off) {
            error_tree_sum_level(se, m, off);
            error_tree_max_level(sm, m, off);
            error_tree_sum_level(sb, m, off);
        }
        __syncthreads();
    }
    if (m == 0) {
        tile_part[3 * (size_t)tile] = se[0];
        tile_part[3 * (size_t)tile + 1] = sm[0];
        tile_part[3 * (size_t)tile + 2] = sb[0];
    }
}

__global__ __launch_bounds__(64) void error_frame_kernel(const ErrorFrame f) {
    __shared__ double se[64], sm[64], sb[64];
    const int m = threadIdx.x;
    if (f.skip && *f.skip) return;                // wave-uniform
    double e = 0.0, mx = 0.0, bad = 0.0;
    if (f.groups >= 2)
        for (int t = m; t < f.tiles; t += 64) {
            e += f.tile_part[3 * (size_t)t];
            const double x = f.tile_part[3 * (size_t)t + 1];
            mx = x > mx ? x : mx;
            bad += f.tile_part[3 * (size_t)t + 2];
        }
    se[m] = e; sm[m] = mx; sb[m] = bad;
    __syncthreads();
    for (int off = 32; off >= 1; off >>= 1) {
        if (m < off) {
            error_tree_sum_level(se, m, off);
            error_tree_max_level(sm, m, off);
            error_tree_sum_level(sb, m, off);
        }
        __syncthreads();
    }
    if (m != 0) return;
    ErrorWords w;
    if (f.groups >= 2) error_frame_result(se[0], sm[0], (long long)sb[0], f.pixels, &w);
    else error_frame_result(0.0, 0.0, f.pixels, f.pixels, &w);      // no estimate yet: NaN figures
    if (f.groups < 2) w.nonfinite = 0;
    f.out->frame_error = w.frame_error;
    f.out->max_error = w.max_error;
    f.out->nonfinite = w.nonfinite;
    f.out->pixels = w.pixels;
    f.out->samples = f.samples;
    f.out->groups = f.groups;
    if (f.groups >= 2 && error_converged(w.frame_error, f.threshold, f.samples, f.min_samples)) {
        __hip_atomic_store(f.stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(f.converged, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_error_moments_chunks(const ImageParams& im, double* q, const double* part, int tiles, int chunks,
                                       int chunk, int ns, const uint32_t* skip, hipStream_t stream) {
    if (tiles <= 0 || chunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(error_moments_kernel, dim3((unsigned)tiles), dim3(64), 0, stream, im, q, part, tiles, chunks, chunk,
                       ns, skip, 0);
    return hipGetLastError();
}

hipError_t launch_error_moments(const ImageParams& im, double* q, const double* part, bool tri_bvh, const uint32_t* skip,
                                hipStream_t stream) {
    if (im.cw <= 0 || im.ch <= 0 || im.s_end <= im.s_begin) return hipSuccess;
    const int ns = im.s_end - im.s_begin;
    const PoolPlan p = pool_plan(im.cw, im.ch, ns, tri_bvh, im.pool_chunk);
    return launch_error_moments_chunks(im, q, part, p.tiles, p.chunks, p.chunk, ns, skip, stream);
}

hipError_t launch_error_estimate(const ImageParams& im, const double* sum, const double* q, int groups, int samples,
                                 double* var_mean, float* rel_error, double* tile_part, const uint32_t* skip,
                                 hipStream_t stream) {
    if (im.cw <= 0 || im.ch <= 0) return hipSuccess;
    if (groups < 2 || samples <= 0) return hipErrorInvalidValue;
    const int tiles = ((im.cw + 7) / 8) * ((im.ch + 7) / 8);
    hipLaunchKernelGGL(error_tile_kernel, dim3((unsigned)tiles), dim3(64), 0, stream, im, sum, q, groups, samples, var_mean,
                       rel_error, tile_part, skip);
    return hipGetLastError();
}

hipError_t launch_error_frame(const ErrorFrame& f, hipStream_t stream) {
    hipLaunchKernelGGL(error_frame_kernel, dim3(1), dim3(64), 0, stream, f);
    return hipGetLastError();
}

}  // namespace rt
