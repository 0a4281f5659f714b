// accum.hip -- the kernels of restir_accum_* (accum.h has the arithmetic, DESIGN.md §6 "Accumulating frames" the
// semantics).  Compiled with -ffp-contract=off like every other kernel: each step of the fold is the host's single
// float32 operation.
//
// k_accum_add is a pure stream over the image's floats: a lane folds four consecutive floats -- one 16-byte load of the
// image, one 16-byte load and store per state plane (36 B per pixel without the variance, 60 B with) -- and the
// count % 4 floats after the last whole group go to as many lanes one float each.  Nothing is shared between lanes: no
// LDS, no barrier; the grid is sized to the data and every index is 64-bit and below `count` by the tests below.
// k_accum_resolve writes the (optionally tone-mapped) mean back as the context's last image through tone_map_rgb, the
// final kernels' own function.  k_accum_stats is the first stage of a deterministic reduction: a block owns a fixed
// range, every lane sums its entries in index order in double, the block adds its lanes in a fixed tree; the host adds
// the blocks' partials in index order.  No float atomics anywhere.
#include "kernels_common.h"

#include "accum.h"

namespace romis {
namespace {

constexpr uint32_t kAccumBlock = 256;

template <bool kVar>
__global__ __launch_bounds__(kAccumBlock) void k_accum_add(const float* __restrict__ x, float* __restrict__ mean,
                                                           float* __restrict__ m2, uint64_t count, float inv_n) {
    const uint64_t i = (uint64_t)blockIdx.x * kAccumBlock + threadIdx.x;
    const uint64_t groups = count / 4u;
    if (i < groups) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        float4 m = reinterpret_cast<const float4*>(mean)[i];
        if (kVar) {
            float4 q = reinterpret_cast<const float4*>(m2)[i];
            accum_fold_var(v.x, inv_n, m.x, q.x);
            accum_fold_var(v.y, inv_n, m.y, q.y);
            accum_fold_var(v.z, inv_n, m.z, q.z);
            accum_fold_var(v.w, inv_n, m.w, q.w);
            reinterpret_cast<float4*>(m2)[i] = q;
        } else {
            accum_fold_mean(v.x, inv_n, m.x);
            accum_fold_mean(v.y, inv_n, m.y);
            accum_fold_mean(v.z, inv_n, m.z);
            accum_fold_mean(v.w, inv_n, m.w);
        }
        reinterpret_cast<float4*>(mean)[i] = m;
        return;
    }
    const uint64_t e = groups * 4u + (i - groups);   // the scalar tail: at most three lanes
    if (e >= count) return;
    float m = mean[e];
    if (kVar) {
        float q = m2[e];
        accum_fold_var(x[e], inv_n, m, q);
        m2[e] = q;
    } else {
        accum_fold_mean(x[e], inv_n, m);
    }
    mean[e] = m;
}

__global__ __launch_bounds__(kAccumBlock) void k_accum_resolve(const float* __restrict__ mean, float* __restrict__ rgb,
                                                               uint64_t pixels, FeaturesDev f) {
    const uint64_t p = (uint64_t)blockIdx.x * kAccumBlock + threadIdx.x;
    if (p >= pixels) return;
    const float* s = mean + p * 3u;
    const v3 color = tone_map_rgb(f, mk(s[0], s[1], s[2]), gl_global_tabs());
    float* o = rgb + p * 3u;
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
}

__global__ __launch_bounds__(kAccumStatsBlock) void k_accum_stats(const float* __restrict__ mean, const float* __restrict__ m2,
                                                                  uint64_t count, double nn1, AccumPartial* __restrict__ partials) {
    __shared__ double s_term[kAccumStatsBlock];
    __shared__ double s_value[kAccumStatsBlock];
    __shared__ uint32_t s_bad[kAccumStatsBlock];
    const uint64_t base = (uint64_t)blockIdx.x * kAccumStatsChunk;
    double term = 0.0, value = 0.0;
    uint32_t bad = 0;
    for (uint32_t k = 0; k < kAccumStatsPerLane; k++) {
        const uint64_t e = base + (uint64_t)k * kAccumStatsBlock + threadIdx.x;
        if (e >= count) break;
        double t, v;
        if (accum_stats_term(mean[e], m2[e], nn1, t, v)) {
            term += t;
            value += v;
        } else {
            bad++;
        }
    }
    s_term[threadIdx.x] = term;
    s_value[threadIdx.x] = value;
    s_bad[threadIdx.x] = bad;
    for (uint32_t w = kAccumStatsBlock / 2u; w > 0u; w >>= 1) {
        __syncthreads();
        if (threadIdx.x < w) {
            s_term[threadIdx.x] += s_term[threadIdx.x + w];
            s_value[threadIdx.x] += s_value[threadIdx.x + w];
            s_bad[threadIdx.x] += s_bad[threadIdx.x + w];
        }
    }
    if (threadIdx.x == 0) {
        AccumPartial out;
        out.term = s_term[0];
        out.value = s_value[0];
        out.nonfinite = s_bad[0];
        out.pad = 0;
        partials[blockIdx.x] = out;
    }
}

// blocks of `block` lanes over `items`; false when they do not fit a grid
bool grid_for(uint64_t items, uint32_t block, uint32_t& out) {
    const uint64_t b = (items + block - 1u) / block;
    if (b > 0x7FFFFFFFull) return false;
    out = (uint32_t)b;
    return true;
}

}  // namespace

hipError_t launch_accum_add(const float* x, float* mean, float* m2, uint64_t count, float inv_n, hipStream_t stream) {
    if (!count) return hipSuccess;
    uint32_t grid;
    if (!grid_for(count / 4u + count % 4u, kAccumBlock, grid)) return hipErrorInvalidValue;
    if (m2)
        hipLaunchKernelGGL(k_accum_add<true>, dim3(grid), dim3(kAccumBlock), 0, stream, x, mean, m2, count, inv_n);
    else
        hipLaunchKernelGGL(k_accum_add<false>, dim3(grid), dim3(kAccumBlock), 0, stream, x, mean, m2, count, inv_n);
    return hipGetLastError();
}

hipError_t launch_accum_resolve(const float* mean, float* rgb, uint64_t pixels, const FeaturesDev& f, hipStream_t stream) {
    if (!pixels) return hipSuccess;
    uint32_t grid;
    if (!grid_for(pixels, kAccumBlock, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_accum_resolve, dim3(grid), dim3(kAccumBlock), 0, stream, mean, rgb, pixels, f);
    return hipGetLastError();
}

hipError_t launch_accum_stats(const float* mean, const float* m2, uint64_t count, double nn1, AccumPartial* partials,
                              hipStream_t stream) {
    if (!count) return hipSuccess;
    uint32_t grid;
    if (!grid_for(accum_stats_blocks(count), 1u, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_accum_stats, dim3(grid), dim3(kAccumStatsBlock), 0, stream, mean, m2, count, nn1, partials);
    return hipGetLastError();
}

}  // namespace romis
