// accum.h -- frames accumulated on the device (restir_accum_*): a running mean, and optionally the sum of squared
// deviations m2, per float of the context's last image.  The operation is elementwise over the image's 3 W H floats.
// Folding the n-th value x (n = 1, 2, ...) is Welford's recurrence with the reciprocal inv_n = 1.0f / (float)n computed
// once on the host: every step below is a single float32 operation, compiled without contraction on both sides, so the
// kernel (accum.hip k_accum_add) and the host's restir_accum_fold agree bit for bit.  IEEE special values propagate as
// the operations give them; a NaN's payload and sign are not part of the contract (DESIGN.md §6 "Accumulating frames").
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROMIS_ACCUM_HD __host__ __device__ __forceinline__
#else
#define ROMIS_ACCUM_HD inline
#endif

namespace romis {

// the frame counts whose (float)n is exact: one more add is RESTIR_ERR_STATE
constexpr uint32_t kAccumMaxFrames = (1u << 24) - 1u;

// mean' = mean + (x - mean) * inv_n
ROMIS_ACCUM_HD void accum_fold_mean(float x, float inv_n, float& mean) {
    const float d = x - mean;
    mean = mean + d * inv_n;
}

// ... and m2' = m2 + (x - mean) * (x - mean')
ROMIS_ACCUM_HD void accum_fold_var(float x, float inv_n, float& mean, float& m2) {
    const float d = x - mean;
    const float m = mean + d * inv_n;
    m2 = m2 + d * (x - m);
    mean = m;
}

// One float's share of restir_accum_stats: after n >= 2 frames m2 / (n (n - 1)) estimates the variance of the mean.
// nn1 = (double)n * (double)(n - 1).  false: the entry is not finite and is left out of both sums.
ROMIS_ACCUM_HD bool accum_stats_term(float mean, float m2, double nn1, double& term, double& value) {
    const float big = 3.402823466e+38f;   // FLT_MAX: |v| <= big <=> v is finite (a NaN fails the comparison)
    const float am = mean < 0.0f ? -mean : mean, a2 = m2 < 0.0f ? -m2 : m2;
    if (!(am <= big) || !(a2 <= big)) return false;
    term = (double)m2 / nn1;
    value = (double)mean;
    return true;
}

// a block of k_accum_stats owns this many consecutive floats and writes one partial
constexpr uint32_t kAccumStatsBlock = 256;
constexpr uint32_t kAccumStatsPerLane = 16;
constexpr uint32_t kAccumStatsChunk = kAccumStatsBlock * kAccumStatsPerLane;

struct AccumPartial {
    double term;          // sum of accum_stats_term's terms over the block's range
    double value;         // ... of its means
    uint64_t nonfinite;   // entries left out
    uint64_t pad;
};

#if defined(__HIPCC__)
struct FeaturesDev;

// All three enqueue on `stream` and never synchronise.  Every buffer is 16-byte aligned (hipMalloc) and holds `count`
// floats (3 per pixel).
// state <- fold of image x as the n-th (inv_n = 1.0f / (float)n); m2 == nullptr: the mean alone
hipError_t launch_accum_add(const float* x, float* mean, float* m2, uint64_t count, float inv_n, hipStream_t stream);
// rgb <- tone_map_rgb(f, mean) per pixel (f.tone_map == 0: the mean's bits)
hipError_t launch_accum_resolve(const float* mean, float* rgb, uint64_t pixels, const FeaturesDev& f, hipStream_t stream);
// partials[b] for b < accum_stats_blocks(count): block b reduces floats [b * kAccumStatsChunk, ...) in double
inline uint64_t accum_stats_blocks(uint64_t count) { return (count + kAccumStatsChunk - 1u) / kAccumStatsChunk; }
hipError_t launch_accum_stats(const float* mean, const float* m2, uint64_t count, double nn1, AccumPartial* partials,
                              hipStream_t stream);
#endif

}  // namespace romis
