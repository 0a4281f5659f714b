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

__global__ __launch_bounds__(kDnBlock) void k_denoise_level(DenoiseLevelArgs a, FeaturesDev f) {
    __shared__ float4 s_ga[kDnRecords];
    __shared__ float4 s_pf[kDnRecords];
    __shared__ float4 s_c[kDnRecords];   // (colour, 1: the tap contributes its colour / 0: skipped)

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
            c = make_float4(cx, cy, cz, __uint_as_float(denoise_finite3(cx, cy, cz) ? 1u : 0u));
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

hipError_t launch_denoise_level(const float* in, float* out, const float4* n_t, const float4* ga, const float4* pf, uint32_t w,
                                uint32_t h, uint32_t level, uint32_t normal_power_log2, float sigma_plane, const FeaturesDev* tone,
                                hipStream_t stream) {
    if (w == 0 || h == 0) return hipSuccess;
    if (level >= kDenoiseMaxIterations) return hipErrorInvalidValue;
    const uint32_t s = 1u << level;
    // the largest class (residue 0) has ceil(w / s) x ceil(h / s) lattice points
    const uint32_t lw = (w + s - 1u) / s, lh = (h + s - 1u) / s;
    DenoiseLevelArgs a;
    a.in = in; a.out = out; a.n_t = n_t; a.ga = ga; a.pf = pf;
    a.w = w; a.h = h; a.level = level;
    a.ntx = (lw + kDnTileW - 1u) / kDnTileW;
    a.normal_power_log2 = normal_power_log2;
    a.sigma_plane = sigma_plane;
    const uint64_t items = (uint64_t)a.ntx * ((lh + kDnTileH - 1u) / kDnTileH) * s * s;
    if (items > 0x7FFFFFFFull) return hipErrorInvalidValue;
    FeaturesDev f{};
    if (tone) f = *tone;
    hipLaunchKernelGGL(k_denoise_level, dim3((uint32_t)items), dim3(kDnBlock), 0, stream, a, f);
    return hipGetLastError();
}

}  // namespace romis
