// denoise.hip -- the kernels of restir_denoise (denoise.h has the arithmetic, DESIGN.md §6 "Denoising a frame" the
// semantics and the measurements).  Compiled with -ffp-contract=off and correctly rounded divide / sqrt like every other
// kernel: each step is the host's single float32 operation.
//
// k_denoise_guides: one lane per pixel, once per view.  It turns the G-buffer record into the guide -- ga = (N / |N|,
// bits(material)) in a plane of its own, (P, flat) over p_mat in place; n_t keeps t for the plane term's scale.
//
// k_denoise_level: one kernel for every step s = 2^level.  The taps of a pixel lie on the stride-s lattice through it, so
// a block of 256 lanes owns a 32 x 8 tile of the lattice of one residue class (x mod s, y mod s) and stages the 36 x 12
// lattice records its taps reach -- guide normal and material, position and flat flag, colour and a "contributes" word:
// 48 B each, 20.7 KB -- into LDS once; all 25 taps of every lane then read LDS, at any step.  A record outside the image
// or with a colour that is not finite is staged as "skip".  The s^2 sibling blocks that cover one pixel region are
// consecutive work items, and xcd_banded_tile gives every XCD one contiguous run of items: siblings run back to back on
// one XCD, where their strided loads meet the same L2 lines.  Every lane sums its taps serially in the contract's order.
// No atomics, no inline assembly; a block whose class has no pixel in its tile leaves before the barrier as a whole.
//
// restir_denoise_lum's kernels (DESIGN.md §6 "Denoising with a luminance term").  k_denoise_level is one body,
// template <bool LUM>: LUM = false is restir_denoise's kernel, instruction for instruction what it was before the template
// (56 SGPRs, 33 VGPRs, no scratch, 20736 B of LDS, as before); LUM = true keeps the 48-byte record -- the variance takes
// the colour record's fourth word, "contributes" moves to bit 1 of the flat word -- computes a tap's luminance from its
// staged colour, reads the centre's nine pre-filter variances from global memory at unit offsets and writes a second
// plane (40 VGPRs, no scratch, the same LDS).  k_denoise_var_spatial lays its 7 x 7 window out like a level at step 1: a
// 32 x 8 pixel tile, the 38 x 14 apron staged once as (g, material), (P, flat), (luminance, contributes) -- 40 B a
// record, 21.3 KB --, 49 taps per lane from LDS, one barrier.  k_denoise_var_accum is elementwise.
#include "kernels_common.h"

#include "denoise.h"

namespace romis {
namespace {

constexpr uint32_t kDnBlock = 256;
constexpr uint32_t kDnTileW = 32, kDnTileH = 8;                 // lattice points a block owns
constexpr uint32_t kDnApronW = kDnTileW + 4, kDnApronH = kDnTileH + 4;
constexpr uint32_t kDnRecords = kDnApronW * kDnApronH;          // 432
static_assert(kDnTileW * kDnTileH == kDnBlock, "one lane per lattice point");
static_assert(3 * kDnRecords * sizeof(float4) <= kLdsBudget, "the staged records fit the LDS budget");

struct DenoiseLevelArgs {
    const float* in;      // w x h float3, image rows
    float* out;
    const float4* n_t;    // (.., t), G-buffer rows
    const float4* ga;     // (g, bits(material))
    const float4* pf;     // (P, flat)
    uint32_t w, h;
    uint32_t level;       // the step is 1 << level
    uint32_t ntx;         // lattice tiles per row of a class
    uint32_t normal_power_log2;
    float sigma_plane;
};
struct DenoiseLevelLumArgs : DenoiseLevelArgs {
    const float* var_in;  // w x h floats, image rows
    float* var_out;
    float sigma_lum;
};
template <bool LUM>
using DnArgs = std::conditional_t<LUM, DenoiseLevelLumArgs, DenoiseLevelArgs>;

// k_denoise_var_spatial: a 32 x 8 pixel tile and the 38 x 14 records its 7 x 7 windows reach
constexpr uint32_t kDvApronW = kDnTileW + 6, kDvApronH = kDnTileH + 6;
constexpr uint32_t kDvRecords = kDvApronW * kDvApronH;          // 532
static_assert(kDvRecords * (2 * sizeof(float4) + sizeof(float2)) <= kLdsBudget, "the staged records fit the LDS budget");

__global__ __launch_bounds__(kDnBlock) void k_denoise_guides(const float4* __restrict__ n_t, float4* __restrict__ p_mat,
                                                             float4* __restrict__ ga, uint64_t pixels, uint32_t miss_material) {
    const uint64_t p = (uint64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= pixels) return;
    const float4 n = n_t[p], pm = p_mat[p];
    DenoiseGuide g;
    denoise_guide(n.x, n.y, n.z, pm.x, pm.y, pm.z, __float_as_uint(pm.w), miss_material, g);
    ga[p] = make_float4(g.gx, g.gy, g.gz, __uint_as_float(g.mat));
    p_mat[p] = make_float4(g.px, g.py, g.pz, __uint_as_float(g.flat));
}

__device__ __forceinline__ DenoiseGuide dn_guide_of(float4 a, float4 b) {
    DenoiseGuide g;
    g.gx = a.x; g.gy = a.y; g.gz = a.z; g.mat = __float_as_uint(a.w);
    g.px = b.x; g.py = b.y; g.pz = b.z; g.flat = __float_as_uint(b.w);
    return g;
}
// ... of a record whose flat word carries "contributes" in bit 1
__device__ __forceinline__ DenoiseGuide dn_guide_of_lum(float4 a, float4 b) {
    DenoiseGuide g = dn_guide_of(a, b);
    g.flat &= 1u;
    return g;
}

// RESTIR_DENOISE_VAR_SPATIAL: one lane per pixel of a 32 x 8 tile, the 38 x 14 apron staged once, 49 taps from LDS
__global__ __launch_bounds__(kDnBlock) void k_denoise_var_spatial(const float* __restrict__ in, float* __restrict__ var,
                                                                  const float4* __restrict__ n_t, const float4* __restrict__ ga_p,
                                                                  const float4* __restrict__ pf_p, uint32_t w, uint32_t h,
                                                                  uint32_t ntx, uint32_t normal_power_log2, float sigma_plane) {
    __shared__ float4 s_ga[kDvRecords];
    __shared__ float4 s_pf[kDvRecords];
    __shared__ float2 s_l[kDvRecords];   // (luminance, 1: the tap contributes / 0: skipped)

    const uint32_t tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int64_t x0 = (int64_t)tx * kDnTileW, r0 = (int64_t)ty * kDnTileH;   // (inside the image: the grid is sized to it)
    for (uint32_t k = threadIdx.x; k < kDvRecords; k += kDnBlock) {
        const int64_t x = x0 + ((int)(k % kDvApronW) - 3), r = r0 + ((int)(k / kDvApronW) - 3);
        float4 ga = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pf = ga;
        float2 l = make_float2(0.0f, 0.0f);
        if (x >= 0 && r >= 0 && x < (int64_t)w && r < (int64_t)h) {
            const size_t pi = (size_t)r * w + (size_t)x, gi = (size_t)(h - 1u - (uint32_t)r) * w + (size_t)x;
            const float* cp = in + 3 * pi;
            const float cx = cp[0], cy = cp[1], cz = cp[2];
            ga = ga_p[gi];
            pf = pf_p[gi];
            l = make_float2(denoise_lum(cx, cy, cz), __uint_as_float(denoise_finite3(cx, cy, cz) ? 1u : 0u));
        }
        s_ga[k] = ga; s_pf[k] = pf; s_l[k] = l;
    }
    __syncthreads();

    const uint32_t li = threadIdx.x % kDnTileW, lj = threadIdx.x / kDnTileW;
    const int64_t x = x0 + li, r = r0 + lj;
    if (x >= (int64_t)w || r >= (int64_t)h) return;   // (after the last barrier)
    const uint32_t centre = (lj + 3u) * kDvApronW + li + 3u;
    float v = 0.0f;
    if (__float_as_uint(s_l[centre].y) != 0u) {
        const DenoiseGuide gp = dn_guide_of(s_ga[centre], s_pf[centre]);
        const size_t gi = (size_t)(h - 1u - (uint32_t)r) * w + (size_t)x;
        const float inv_s = denoise_inv_s(sigma_plane, n_t[gi].w);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int dy = -3; dy <= 3; dy++) {
#pragma unroll
            for (int dx = -3; dx <= 3; dx++) {
                const uint32_t q = (uint32_t)((int)centre + dy * (int)kDvApronW + dx);
                const float2 lq = s_l[q];
                if (__float_as_uint(lq.y) == 0u) continue;
                const float wt = (dx == 0 && dy == 0)
                                     ? 1.0f
                                     : denoise_tap_weight(gp, dn_guide_of(s_ga[q], s_pf[q]), 1.0f, inv_s, normal_power_log2);
                if (wt > 0.0f) denoise_var_tap_add(wt, lq.x, s0, s1, s2);
            }
        }
        v = denoise_var_spatial_result(s0, s1, s2);
    }
    var[(size_t)r * w + (size_t)x] = v;
}

// RESTIR_DENOISE_VAR_ACCUM: elementwise.  The accumulator's planes are the image's layout -- 3 floats per pixel, image
// rows (restir_accum_add folds the image float by float) --, so pixel p of mean / m2 is pixel p of rgb and of var
__global__ __launch_bounds__(kDnBlock) void k_denoise_var_accum(const float* __restrict__ mean, const float* __restrict__ m2,
                                                                float* __restrict__ rgb, float* __restrict__ var, uint64_t pixels,
                                                                float inv) {
    const uint64_t p = (uint64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= pixels) return;
    const float* m = mean + p * 3u;
    const float* q = m2 + p * 3u;
    float* o = rgb + p * 3u;
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
    var[p] = denoise_var_of_m2(q[0], q[1], q[2], inv);
}

template <bool LUM>
__global__ __launch_bounds__(kDnBlock) void k_denoise_level(DnArgs<LUM> a, FeaturesDev f) {
    __shared__ float4 s_ga[kDnRecords];
    __shared__ float4 s_pf[kDnRecords];   // LUM: bit 1 of the flat word says "the tap contributes its colour"
    __shared__ float4 s_c[kDnRecords];    // (colour, 1: the tap contributes its colour / 0: skipped); LUM: (colour, variance)

    const uint32_t s = 1u << a.level, smask = s - 1u;
    const uint32_t item = xcd_banded_tile();
    const uint32_t cls = item & (s * s - 1u), tile = item >> (2u * a.level);
    const uint32_t rx = cls & smask, ry = cls >> a.level;
    const uint32_t tx = tile % a.ntx, ty = tile / a.ntx;
    // the lattice tile's first point, in pixels
    const int64_t x0 = (int64_t)rx + (int64_t)s * (tx * kDnTileW), r0 = (int64_t)ry + (int64_t)s * (ty * kDnTileH);
    if (x0 >= (int64_t)a.w || r0 >= (int64_t)a.h) return;   // (block-uniform, before the barrier)

    for (uint32_t k = threadIdx.x; k < kDnRecords; k += kDnBlock) {
        const int64_t x = x0 + (int64_t)s * ((int)(k % kDnApronW) - 2), r = r0 + (int64_t)s * ((int)(k / kDnApronW) - 2);
        float4 ga = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pf = ga, c = ga;
        if (x >= 0 && r >= 0 && x < (int64_t)a.w && r < (int64_t)a.h) {
            const size_t pi = (size_t)r * a.w + (size_t)x, gi = (size_t)(a.h - 1u - (uint32_t)r) * a.w + (size_t)x;
            const float* cp = a.in + 3 * pi;
            const float cx = cp[0], cy = cp[1], cz = cp[2];
            ga = a.ga[gi];
            pf = a.pf[gi];
            if constexpr (LUM) {
                pf.w = __uint_as_float(__float_as_uint(pf.w) | (denoise_finite3(cx, cy, cz) ? 2u : 0u));
                c = make_float4(cx, cy, cz, a.var_in[pi]);
            } else {
                c = make_float4(cx, cy, cz, __uint_as_float(denoise_finite3(cx, cy, cz) ? 1u : 0u));
            }
        }
        s_ga[k] = ga; s_pf[k] = pf; s_c[k] = c;
    }
    __syncthreads();

    const uint32_t li = threadIdx.x % kDnTileW, lj = threadIdx.x / kDnTileW;
    const int64_t x = x0 + (int64_t)s * li, r = r0 + (int64_t)s * lj;
    if (x >= (int64_t)a.w || r >= (int64_t)a.h) return;   // (after the last barrier)
    const uint32_t centre = (lj + 2u) * kDnApronW + li + 2u;
    const size_t pi = (size_t)r * a.w + (size_t)x;
    const float4 cc = s_c[centre];
    v3 color = mk(cc.x, cc.y, cc.z);   // a centre that is not finite: its input's bits
    if constexpr (LUM) {
        float var = cc.w;              // ... and its variance
        const float4 pfc = s_pf[centre];
        if ((__float_as_uint(pfc.w) & 2u) != 0u) {
            // the centre's pre-filtered variance: nine unit-offset loads, whatever the step
            float gnum = 0.0f, gden = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int64_t qx = x + dx, qy = r + dy;
                    if (qx < 0 || qy < 0 || qx >= (int64_t)a.w || qy >= (int64_t)a.h) continue;
                    const float gw = denoise_g(dy) * denoise_g(dx);
                    gnum = gnum + gw * a.var_in[(size_t)qy * a.w + (size_t)qx];
                    gden = gden + gw;
                }
            }
            const float inv_den = denoise_inv_den(a.sigma_lum, gnum / gden);
            const float lp = denoise_lum(cc.x, cc.y, cc.z);
            const DenoiseGuide gp = dn_guide_of_lum(s_ga[centre], pfc);
            const size_t gi = (size_t)(a.h - 1u - (uint32_t)r) * a.w + (size_t)x;
            const float inv_s = denoise_inv_s(a.sigma_plane, a.n_t[gi].w);
            float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const uint32_t q = (uint32_t)((int)centre + dy * (int)kDnApronW + dx);
                    const float4 pfq = s_pf[q];
                    if ((__float_as_uint(pfq.w) & 2u) == 0u) continue;
                    const float4 cq = s_c[q];
                    const float hk = denoise_k(dy) * denoise_k(dx);
                    const float wt = (dx == 0 && dy == 0)
                                         ? hk
                                         : denoise_tap_weight(gp, dn_guide_of_lum(s_ga[q], pfq), hk, inv_s, a.normal_power_log2) *
                                               denoise_lum_weight(denoise_lum(cq.x, cq.y, cq.z), lp, inv_den);
                    if (wt > 0.0f) {
                        denoise_tap_add(wt, cq.x, cq.y, cq.z, sw, sx, sy, sz);
                        sv = sv + (wt * wt) * cq.w;
                    }
                }
            }
            color = mk(sx / sw, sy / sw, sz / sw);
            var = sv / (sw * sw);
        }
        a.var_out[pi] = var;
    } else {
        if (__float_as_uint(cc.w) != 0u) {
            const DenoiseGuide gp = dn_guide_of(s_ga[centre], s_pf[centre]);
            const size_t gi = (size_t)(a.h - 1u - (uint32_t)r) * a.w + (size_t)x;
            const float inv_s = denoise_inv_s(a.sigma_plane, a.n_t[gi].w);
            float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const uint32_t q = (uint32_t)((int)centre + dy * (int)kDnApronW + dx);
                    const float4 cq = s_c[q];
                    if (__float_as_uint(cq.w) == 0u) continue;
                    const float hk = denoise_k(dy) * denoise_k(dx);
                    const float wt = (dx == 0 && dy == 0)
                                         ? hk
                                         : denoise_tap_weight(gp, dn_guide_of(s_ga[q], s_pf[q]), hk, inv_s, a.normal_power_log2);
                    if (wt > 0.0f) denoise_tap_add(wt, cq.x, cq.y, cq.z, sw, sx, sy, sz);
                }
            }
            color = mk(sx / sw, sy / sw, sz / sw);
        }
    }
    color = tone_map_rgb(f, color, gl_global_tabs());   // (f.tone_map is set for the last level alone)
    float* o = a.out + 3 * pi;
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
}

}  // namespace

hipError_t launch_denoise_guides(const float4* n_t, float4* p_mat, float4* ga, uint64_t pixels, uint32_t miss_material,
                                 hipStream_t stream) {
    if (!pixels) return hipSuccess;
    const uint64_t blocks = (pixels + kDnBlock - 1u) / kDnBlock;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_denoise_guides, dim3((uint32_t)blocks), dim3(kDnBlock), 0, stream, n_t, p_mat, ga, pixels, miss_material);
    return hipGetLastError();
}

// the level's arguments and grid; false when they do not fit a launch
static bool denoise_level_shape(DenoiseLevelArgs& a, const float* in, float* out, const float4* n_t, const float4* ga,
                                const float4* pf, uint32_t w, uint32_t h, uint32_t level, uint32_t normal_power_log2,
                                float sigma_plane, uint32_t& grid) {
    if (level >= kDenoiseMaxIterations) return false;
    const uint32_t s = 1u << level;
    // the largest class (residue 0) has ceil(w / s) x ceil(h / s) lattice points
    const uint32_t lw = (w + s - 1u) / s, lh = (h + s - 1u) / s;
    a.in = in; a.out = out; a.n_t = n_t; a.ga = ga; a.pf = pf;
    a.w = w; a.h = h; a.level = level;
    a.ntx = (lw + kDnTileW - 1u) / kDnTileW;
    a.normal_power_log2 = normal_power_log2;
    a.sigma_plane = sigma_plane;
    const uint64_t items = (uint64_t)a.ntx * ((lh + kDnTileH - 1u) / kDnTileH) * s * s;
    if (items > 0x7FFFFFFFull) return false;
    grid = (uint32_t)items;
    return true;
}

hipError_t launch_denoise_level(const float* in, float* out, const float4* n_t, const float4* ga, const float4* pf, uint32_t w,
                                uint32_t h, uint32_t level, uint32_t normal_power_log2, float sigma_plane, const FeaturesDev* tone,
                                hipStream_t stream) {
    if (w == 0 || h == 0) return hipSuccess;
    DenoiseLevelArgs a;
    uint32_t grid;
    if (!denoise_level_shape(a, in, out, n_t, ga, pf, w, h, level, normal_power_log2, sigma_plane, grid)) return hipErrorInvalidValue;
    FeaturesDev f{};
    if (tone) f = *tone;
    hipLaunchKernelGGL(k_denoise_level<false>, dim3(grid), dim3(kDnBlock), 0, stream, a, f);
    return hipGetLastError();
}

hipError_t launch_denoise_level_lum(const float* in, float* out, const float* var_in, float* var_out, const float4* n_t,
                                    const float4* ga, const float4* pf, uint32_t w, uint32_t h, uint32_t level,
                                    uint32_t normal_power_log2, float sigma_plane, float sigma_lum, const FeaturesDev* tone,
                                    hipStream_t stream) {
    if (w == 0 || h == 0) return hipSuccess;
    DenoiseLevelLumArgs a;
    uint32_t grid;
    if (!denoise_level_shape(a, in, out, n_t, ga, pf, w, h, level, normal_power_log2, sigma_plane, grid)) return hipErrorInvalidValue;
    a.var_in = var_in; a.var_out = var_out; a.sigma_lum = sigma_lum;
    FeaturesDev f{};
    if (tone) f = *tone;
    hipLaunchKernelGGL(k_denoise_level<true>, dim3(grid), dim3(kDnBlock), 0, stream, a, f);
    return hipGetLastError();
}

hipError_t launch_denoise_var_spatial(const float* in, float* var, const float4* n_t, const float4* ga, const float4* pf, uint32_t w,
                                      uint32_t h, uint32_t normal_power_log2, float sigma_plane, hipStream_t stream) {
    if (w == 0 || h == 0) return hipSuccess;
    const uint32_t ntx = (w + kDnTileW - 1u) / kDnTileW;
    const uint64_t blocks = (uint64_t)ntx * ((h + kDnTileH - 1u) / kDnTileH);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_denoise_var_spatial, dim3((uint32_t)blocks), dim3(kDnBlock), 0, stream, in, var, n_t, ga, pf, w, h, ntx,
                       normal_power_log2, sigma_plane);
    return hipGetLastError();
}

hipError_t launch_denoise_var_accum(const float* mean, const float* m2, float* rgb, float* var, uint64_t pixels, float inv,
                                    hipStream_t stream) {
    if (!pixels) return hipSuccess;
    const uint64_t blocks = (pixels + kDnBlock - 1u) / kDnBlock;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_denoise_var_accum, dim3((uint32_t)blocks), dim3(kDnBlock), 0, stream, mean, m2, rgb, var, pixels, inv);
    return hipGetLastError();
}

}  // namespace romis
