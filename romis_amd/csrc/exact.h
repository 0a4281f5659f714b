// exact.h -- the exact direct-lighting image of a point-light scene (restir_render_exact, k_exact in exact.hip) and the
// error figures of an image against a kept reference (restir_error_get / restir_error_measure).  The per-float terms of
// the figures live here once: k_error_stats and the host's error_measure_host compile the same text, both without
// contraction, and walk the same partition -- block b owns floats [kErrorChunk b, kErrorChunk (b + 1)), lane t of it the
// entries t, t + 256, ... in index order, the block adds its lanes in a fixed tree, the host adds the blocks' partials in
// index order -- so the two agree bit for bit (DESIGN.md §6 "Exact image and error figures").
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROMIS_ERROR_HD __host__ __device__ __forceinline__
#else
#define ROMIS_ERROR_HD inline
#endif

namespace romis {

constexpr double kErrorRelEps = 1e-2;   // RESTIR_ERROR_REL_EPS

// the sums of one lane, one block or the whole image
struct ErrorSums {
    double se, ae, rel, d, max_abs, ref;   // sums of d*d, |d|, d*d / (r*r + eps), d;  max |d|;  sum of r
    uint64_t counted, nonfinite;
};

ROMIS_ERROR_HD void error_zero(ErrorSums& s) {
    s.se = 0.0; s.ae = 0.0; s.rel = 0.0; s.d = 0.0; s.max_abs = 0.0; s.ref = 0.0;
    s.counted = 0; s.nonfinite = 0;
}

ROMIS_ERROR_HD void error_copy(ErrorSums& to, const ErrorSums& from) {
    to.se = from.se; to.ae = from.ae; to.rel = from.rel; to.d = from.d; to.max_abs = from.max_abs; to.ref = from.ref;
    to.counted = from.counted; to.nonfinite = from.nonfinite;
}

// One float's share: a against the reference's r, in double.  An entry whose a or r is not finite is left out of every
// sum and counted in `nonfinite`.
ROMIS_ERROR_HD void error_term(float a, float r, ErrorSums& s) {
    const float big = 3.402823466e+38f;   // FLT_MAX: |v| <= big <=> v is finite (a NaN fails the comparison)
    const float aa = a < 0.0f ? -a : a, ar = r < 0.0f ? -r : r;
    const bool finite = aa <= big && ar <= big;
    // (both counts by selects: one increment behind a branch became an indexed store through scratch memory)
    s.counted += finite ? 1u : 0u;
    s.nonfinite += finite ? 0u : 1u;
    if (!finite) return;
    const double rd = (double)r;
    const double d = (double)a - rd;
    const double ad = d < 0.0 ? -d : d;
    const double dd = d * d;
    s.se += dd;
    s.ae += ad;
    s.rel += dd / (rd * rd + kErrorRelEps);
    s.d += d;
    s.max_abs = ad > s.max_abs ? ad : s.max_abs;
    s.ref += rd;
}

// into += from, quantity by quantity (the tree's and the host's step)
ROMIS_ERROR_HD void error_merge(ErrorSums& into, const ErrorSums& from) {
    into.se += from.se;
    into.ae += from.ae;
    into.rel += from.rel;
    into.d += from.d;
    into.max_abs = from.max_abs > into.max_abs ? from.max_abs : into.max_abs;
    into.ref += from.ref;
    into.counted += from.counted;
    into.nonfinite += from.nonfinite;
}

// a block of k_error_stats owns this many consecutive floats and writes one partial (k_accum_stats' partition)
constexpr uint32_t kErrorBlock = 256;
constexpr uint32_t kErrorPerLane = 16;
constexpr uint32_t kErrorChunk = kErrorBlock * kErrorPerLane;
inline uint64_t error_blocks(uint64_t count) { return (count + kErrorChunk - 1u) / kErrorChunk; }

// lane t's sums over block b's range
ROMIS_ERROR_HD void error_lane(const float* a, const float* r, uint64_t count, uint64_t b, uint32_t t, ErrorSums& s) {
    error_zero(s);
    for (uint32_t k = 0; k < kErrorPerLane; k++) {
        const uint64_t e = b * kErrorChunk + (uint64_t)k * kErrorBlock + t;
        if (e >= count) break;
        error_term(a[e], r[e], s);
    }
}

// The whole reduction on the host: every block's lanes, its tree, the blocks in index order.
inline void error_measure_host(const float* a, const float* r, uint64_t count, ErrorSums& total) {
    error_zero(total);
    ErrorSums lane[kErrorBlock];
    for (uint64_t b = 0; b < error_blocks(count); b++) {
        for (uint32_t t = 0; t < kErrorBlock; t++) error_lane(a, r, count, b, t, lane[t]);
        for (uint32_t w = kErrorBlock / 2u; w > 0u; w >>= 1)
            for (uint32_t t = 0; t < w; t++) error_merge(lane[t], lane[t + w]);
        error_merge(total, lane[0]);
    }
}

#if defined(__HIPCC__)
struct SceneDev;
struct Region;
struct FeaturesDev;

// Both enqueue on `stream` and never synchronise.
// rgb (rg's rect, row 0 = its top) <- the exact image over the G-buffer planes n_t / p_mat of rg's view (s.gbuf_uv: its
// texCoord plane); s holds point lights only.  origin: the camera's.  The BVH is staged in LDS when it fits kLdsBudget
// together with the kernel's static LDS, else walked in global memory.
constexpr size_t kExactStaticLds = 1024;   // a bound on k_exact's static LDS: powf's tables and the vote, 768 B today
hipError_t launch_exact(const SceneDev& s, const Region& rg, const FeaturesDev& f, const float* origin, const float4* n_t,
                        const float4* p_mat, float* rgb, hipStream_t stream);
// partials[b] for b < error_blocks(count): block b's sums of a against r
hipError_t launch_error_stats(const float* a, const float* r, uint64_t count, ErrorSums* partials, hipStream_t stream);
#endif

}  // namespace romis
