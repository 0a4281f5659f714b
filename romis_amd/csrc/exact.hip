// exact.hip -- the kernels of restir_render_exact and restir_error_get (exact.h; DESIGN.md §6 "Exact image and error
// figures" has the semantics).  Compiled with -ffp-contract=off and correctly rounded divide / sqrt like every other
// kernel.
//
// k_exact<LDS_BVH>: one block per 32 x 8 tile of the rect (final shading's Region / work_pixel mapping), one lane per
// pixel.  A lane sums, over all L point lights in light-table order, shade() of its pixel times visible() -- the
// functions final shading calls, over the nodes it walks: the BVH staged in LDS when it fits, the global arrays
// otherwise.  The loop counter is wave-uniform, so light i's position and colour are uniform loads of the light_c2
// planes, once per wave, and every ray of a wave ends at the same light.  The sum is serial per lane: the light order
// is the sum's order by construction.  final_body's shortcut is kept -- a shade of +-0 in all three components casts no
// ray, the visible and the hidden answer adding the same bits to a colour that is never -0 -- and a NaN component is
// not zero, so it traces.  A block whose pixels all hold the miss material leaves before the BVH is staged under the
// final kernels' own condition (SceneDev::miss_shade_zero and a P that is not NaN: every light shades to +-0), writing
// the tone-mapped +0; the vote is the block's barrier, nothing crosses blocks.  No atomics, no inline assembly.
//
// k_error_stats: k_accum_stats' scheme over exact.h's terms.
#include "kernels_common.h"

#include "exact.h"

namespace romis {
namespace {

template <bool LDS_BVH>
__global__ __launch_bounds__(256) void k_exact(SceneDev s, Region rg, FeaturesDev f, float ox, float oy, float oz,
                                               const float4* __restrict__ n_t, const float4* __restrict__ p_mat,
                                               float* __restrict__ rgb) {
    uint32_t x = 0, y = 0;
    size_t p = 0;
    const bool valid = work_pixel(rg, blockIdx.x, x, y, p);
    const float4 pm = valid ? p_mat[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float* o = nullptr;
    if (valid) {
        const uint32_t row = rg.rh - 1u - (y - rg.ry0);
        o = rgb + 3 * ((size_t)row * rg.rw + (x - rg.rx0));
    }
    if (s.miss_shade_zero) {   // (uniform: a kernel argument)
        bool miss = true;
        if (valid) {
            const uint32_t m = min(__float_as_uint(pm.w), s.num_materials - 1u);
            miss = m == s.num_materials - 1u && !__builtin_isnan(pm.x + pm.y + pm.z);
        }
        if (__syncthreads_and(miss)) {   // block-uniform, before the BVH's barrier
            if (valid) {
                const v3 color = tone_map_rgb(f, mk(0.0f, 0.0f, 0.0f), gl_global_tabs());
                o[0] = color.x; o[1] = color.y; o[2] = color.z;
            }
            return;
        }
    }
    const Bvh bvh = LDS_BVH ? stage_bvh(s, g_lds) : global_bvh(s);
    const GlTabs tb = gl_stage_tables();
    if (!valid) return;   // (after the last barrier)
    const Px px = make_px(s, n_t[gidx(rg, p)], pm, mk(ox, oy, oz), p);
    const uint32_t L = s.num_lights;
    v3 color = mk(0.0f, 0.0f, 0.0f);
    for (uint32_t i = 0; i < L; i++) {
        const v3 lpos = xyz(s.light_c2[i]), lcol = xyz(s.light_c2[L + i]);
        v3 sc = shade(s, f, px, lpos, lcol, tb);
        if ((sc.x != 0.0f || sc.y != 0.0f || sc.z != 0.0f) && !visible(bvh, px.P, lpos)) sc = mk(0.0f, 0.0f, 0.0f);
        color = vadd(color, sc);
    }
    color = tone_map_rgb(f, color, tb);
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
}

__global__ __launch_bounds__(kErrorBlock) void k_error_stats(const float* __restrict__ a, const float* __restrict__ r,
                                                             uint64_t count, ErrorSums* __restrict__ partials) {
    __shared__ ErrorSums s_sums[kErrorBlock];
    ErrorSums mine;
    error_lane(a, r, count, blockIdx.x, threadIdx.x, mine);
    error_copy(s_sums[threadIdx.x], mine);   // (field by field: a struct assignment goes through scratch memory)
    for (uint32_t w = kErrorBlock / 2u; w > 0u; w >>= 1) {
        __syncthreads();
        if (threadIdx.x < w) error_merge(s_sums[threadIdx.x], s_sums[threadIdx.x + w]);
    }
    if (threadIdx.x == 0) error_copy(partials[blockIdx.x], s_sums[0]);
}

// Dynamic plus static LDS stay within kLdsBudget, the 64 KB a kernel gets without raising its limit: a BVH in the last
// kExactStaticLds bytes of the budget takes the global-memory instantiation instead of a launch that may be refused.
bool exact_bvh_in_lds(const SceneDev& s) { return bvh_lds_bytes(s) + kExactStaticLds <= kLdsBudget; }

}  // namespace

hipError_t launch_exact(const SceneDev& s, const Region& rg0, const FeaturesDev& f, const float* origin, const float4* n_t,
                        const float4* p_mat, float* rgb, hipStream_t stream) {
    if (rg0.rw == 0 || rg0.rh == 0) return hipSuccess;
    Region rg = rg0;
    rg.map2d = 1u; rg.xcd_rows = 0u; rg.xcd_cols = 0u;
    const uint64_t tiles = (uint64_t)((rg.rw + kTileW - 1) / kTileW) * ((rg.rh + kTileH - 1) / kTileH);
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const bool lds_bvh = exact_bvh_in_lds(s);
    const size_t lds = lds_bvh ? bvh_lds_bytes(s) : 0;
    if (lds_bvh)
        hipLaunchKernelGGL(k_exact<true>, dim3((uint32_t)tiles), dim3(256), lds, stream, s, rg, f, origin[0], origin[1], origin[2],
                           n_t, p_mat, rgb);
    else
        hipLaunchKernelGGL(k_exact<false>, dim3((uint32_t)tiles), dim3(256), 0, stream, s, rg, f, origin[0], origin[1], origin[2],
                           n_t, p_mat, rgb);
    return hipGetLastError();
}

hipError_t launch_error_stats(const float* a, const float* r, uint64_t count, ErrorSums* partials, hipStream_t stream) {
    if (!count) return hipSuccess;
    const uint64_t blocks = error_blocks(count);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_error_stats, dim3((uint32_t)blocks), dim3(kErrorBlock), 0, stream, a, r, count, partials);
    return hipGetLastError();
}

}  // namespace romis
