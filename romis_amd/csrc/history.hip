// history.hip -- the kernels of restir_history_* (history.h has the arithmetic and the layout, DESIGN.md §6 "Image
// history" the semantics and the measurements).  Compiled with -ffp-contract=off and correctly rounded divide / sqrt like
// every other kernel: each step is the host's single float32 operation.
//
// k_history_advance: one lane per pixel, 32 x 8 blocks over the image like k_reproject, so the source pixels of a block
// stay within a few rows and columns of it under small camera motion and the gather's 16-byte records share cache lines
// in both axes.  A lane reads its 12 bytes of image, its three current guide records (48 B), the three kept records of
// its source pixel (48 B, under the lane mask: a rejected pixel reads none) and writes the three records of the other set
// (48 B), all as 16-byte loads and stores but the packed image.  Nothing is shared between lanes: no LDS, no barrier, no
// atomics.  Every index is below W * H: the lane's own by the bounds test, the source's by reproject_source's range test,
// a bilinear tap's by history_gather_bilinear's signed test before the index is formed.
// The guide planes and the map are in G-buffer rows (y = 0 bottom), the image and the state planes in image rows: lane
// (x, y) of the G-buffer is image pixel (x, H - 1 - y), and source (sx, sy) is state pixel (sx, H - 1 - sy).
//
// k_history_resolve writes the (optionally tone-mapped) mean as a packed float3 image through tone_map_rgb, the final
// kernels' own function; restir_history_denoise uses it without a tone map for the image its levels read.
// k_history_var is elementwise: it overwrites the variance plane's entry of every pixel whose history is long enough.
// The spatial estimate of the others is launch_denoise_var_spatial's, computed over the whole mean image before it.
#include "kernels_common.h"

#include "history.h"

#include "launch_shape.h"

namespace romis {
namespace {

constexpr uint32_t kHistBlock = 256;

// the kernel's Kept of history_gather_bilinear: the kept set's planes, image rows.  test reads the tap's (N, t) record and
// the two 4-byte words the test needs, load the two records of a contributing tap.
struct HistKeptDev {
    const float4* a;
    const float4* b;
    const float4* c;
    uint32_t W, H;
    __device__ __forceinline__ void test(uint32_t tx, uint32_t ty, float& nx, float& ny, float& nz, float& t, uint32_t& mat,
                                         uint32_t& n) const {
        const size_t qi = (size_t)(H - 1u - ty) * W + tx;
        const float4 ka = a[qi];
        nx = ka.x; ny = ka.y; nz = ka.z; t = ka.w;
        mat = __float_as_uint(c[qi].w);   // (stored clamped)
        n = __float_as_uint(b[qi].w);
    }
    __device__ __forceinline__ void load(uint32_t tx, uint32_t ty, HistState& s) const {
        const size_t qi = (size_t)(H - 1u - ty) * W + tx;
        const float4 kb = b[qi], kc = c[qi];
        s.mr = kb.x; s.mg = kb.y; s.mb = kb.z;
        s.sr = kc.x; s.sg = kc.y; s.sb = kc.z;
        s.n = __float_as_uint(kb.w);
    }
};

// kGather == kHistGatherNearest is the kernel as it was before the mode existed, instruction for instruction
// (scripts/device_code_diff.py).  kHistGatherBilinear: up to four taps per lane, each inside tap 24 bytes for its test and a
// contributing one 32 more, all under the lane mask; neighbouring lanes' footprints overlap almost completely.
template <uint32_t kGather>
__global__ __launch_bounds__(kBlock) void k_history_advance(HistoryDev a) {
    const uint32_t x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
    const uint32_t W = a.prev_cam.W, H = a.prev_cam.H;
    if (x >= W || y >= H) return;
    const size_t gi = (size_t)y * W + x, pi = (size_t)(H - 1u - y) * W + x;
    const float4 cnt = a.cur_nt[gi], cpf = a.cur_pf[gi], cga = a.cur_ga[gi];
    const uint32_t cur_mat = history_material(__float_as_uint(cga.w), a.miss_mat);
    const float* xp = a.x + 3 * pi;
    const float xr = xp[0], xg = xp[1], xb = xp[2];

    uint32_t why = kHistNoHistory, sx = 0u, sy = 0u;
    HistState s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    if constexpr (kGather == kHistGatherBilinear) {
        uint32_t src = 0u;
        if (a.fresh == 0u) {
            float d, cfx, cfy;
            why = history_source_at(a.prev_cam, cur_mat, a.miss_mat, cpf.x, cpf.y, cpf.z, sx, sy, d, cfx, cfy);
            if (why == kReprojOk)   // (loads under the lane mask)
                why = history_gather_bilinear(HistKeptDev{a.in_a, a.in_b, a.in_c, W, H}, W, H, sx, sy, cfx, cfy, d, cnt.x, cnt.y,
                                              cnt.z, cur_mat, a.miss_mat, s, src);
        }
        history_fold(xr, xg, xb, a.max_frames, s);
        a.out_a[pi] = cnt;
        a.out_b[pi] = make_float4(s.mr, s.mg, s.mb, __uint_as_float(s.n));
        a.out_c[pi] = make_float4(s.sr, s.sg, s.sb, __uint_as_float(cur_mat));
        if (a.map) a.map[gi] = why == kReprojOk ? src : 0xFFFFFFFFu - why;
    } else {
        if (a.fresh == 0u) {
            float d;
            why = history_source(a.prev_cam, cur_mat, a.miss_mat, cpf.x, cpf.y, cpf.z, sx, sy, d);
            if (why == kReprojOk) {   // (loads under the lane mask)
                const size_t qi = (size_t)(H - 1u - sy) * W + sx;
                const float4 ka = a.in_a[qi], kb = a.in_b[qi], kc = a.in_c[qi];
                why = history_accept(ka.x, ka.y, ka.z, ka.w, __float_as_uint(kc.w), __float_as_uint(kb.w), cnt.x, cnt.y, cnt.z,
                                     cur_mat, a.miss_mat, d);
                if (why == kReprojOk) {
                    s.mr = kb.x; s.mg = kb.y; s.mb = kb.z;
                    s.sr = kc.x; s.sg = kc.y; s.sb = kc.z;
                    s.n = __float_as_uint(kb.w);
                }
            }
        }
        history_fold(xr, xg, xb, a.max_frames, s);
        a.out_a[pi] = cnt;
        a.out_b[pi] = make_float4(s.mr, s.mg, s.mb, __uint_as_float(s.n));
        a.out_c[pi] = make_float4(s.sr, s.sg, s.sb, __uint_as_float(cur_mat));
        if (a.map) a.map[gi] = why == kReprojOk ? sy * W + sx : 0xFFFFFFFFu - why;
    }
}

__global__ __launch_bounds__(kHistBlock) void k_history_resolve(const float4* __restrict__ b, float* __restrict__ rgb,
                                                                uint64_t pixels, FeaturesDev f) {
    const uint64_t p = (uint64_t)blockIdx.x * kHistBlock + threadIdx.x;
    if (p >= pixels) return;
    const float4 m = b[p];
    const v3 color = tone_map_rgb(f, mk(m.x, m.y, m.z), gl_global_tabs());
    float* o = rgb + p * 3u;
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
}

__global__ __launch_bounds__(kHistBlock) void k_history_var(const float4* __restrict__ b, const float4* __restrict__ c,
                                                            float* __restrict__ var, uint64_t pixels, uint32_t spatial_below) {
    const uint64_t p = (uint64_t)blockIdx.x * kHistBlock + threadIdx.x;
    if (p >= pixels) return;
    const float4 m = b[p];
    if (__float_as_uint(m.w) < spatial_below) return;   // (before S is read: a short history costs 16 bytes)
    const float4 q = c[p];
    const HistState s{m.x, m.y, m.z, q.x, q.y, q.z, __float_as_uint(m.w)};
    float v;
    if (history_var_temporal(s, spatial_below, v)) var[p] = v;
}

__device__ __forceinline__ DenoiseGuide hist_guide_of(float4 a, float4 b) {
    DenoiseGuide g;
    g.gx = a.x; g.gy = a.y; g.gz = a.z; g.mat = __float_as_uint(a.w);
    g.px = b.x; g.py = b.y; g.pz = b.z; g.flat = __float_as_uint(b.w);
    return g;
}

// The variance plane and the packed mean image in one launch: one lane per pixel over 32 x 8 tiles of the image.  A lane
// whose history is long enough takes history_var_temporal's value; only the others run RESTIR_DENOISE_VAR_SPATIAL's 7 x 7
// window, k_denoise_var_spatial's text and tap order, reading their neighbours' means and guides from global memory --
// after a few frames those lanes are the disoccluded rims, too few to stage anything for.  Every index is inside the
// image by the tests below.
__global__ __launch_bounds__(kBlock) void k_history_var_fused(const float4* __restrict__ b, const float4* __restrict__ c,
                                                              float* __restrict__ rgb, float* __restrict__ var,
                                                              const float4* __restrict__ n_t, const float4* __restrict__ ga_p,
                                                              const float4* __restrict__ pf_p, uint32_t w, uint32_t h,
                                                              uint32_t spatial_below, uint32_t normal_power_log2, float sigma_plane) {
    const uint32_t x = blockIdx.x * kTileW + threadIdx.x, r = blockIdx.y * kTileH + threadIdx.y;
    if (x >= w || r >= h) return;
    const size_t pi = (size_t)r * w + x;
    const float4 m = b[pi];
    float* o = rgb + 3 * pi;
    o[0] = m.x; o[1] = m.y; o[2] = m.z;
    float v = 0.0f;
    bool temporal = false;
    if (__float_as_uint(m.w) >= spatial_below) {
        const float4 q = c[pi];
        const HistState s{m.x, m.y, m.z, q.x, q.y, q.z, __float_as_uint(m.w)};
        temporal = history_var_temporal(s, spatial_below, v);
    }
    if (!temporal && denoise_finite3(m.x, m.y, m.z)) {
        const size_t gi = (size_t)(h - 1u - r) * w + x;
        const DenoiseGuide gp = hist_guide_of(ga_p[gi], pf_p[gi]);
        const float inv_s = denoise_inv_s(sigma_plane, n_t[gi].w);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int dy = -3; dy <= 3; dy++)
            for (int dx = -3; dx <= 3; dx++) {
                const int64_t qx = (int64_t)x + dx, qr = (int64_t)r + dy;
                if (qx < 0 || qr < 0 || qx >= (int64_t)w || qr >= (int64_t)h) continue;
                const float4 cq = b[(size_t)qr * w + (size_t)qx];
                if (!denoise_finite3(cq.x, cq.y, cq.z)) continue;
                float wt = 1.0f;
                if (dx != 0 || dy != 0) {
                    const size_t gq = (size_t)(h - 1u - (uint32_t)qr) * w + (size_t)qx;
                    wt = denoise_tap_weight(gp, hist_guide_of(ga_p[gq], pf_p[gq]), 1.0f, inv_s, normal_power_log2);
                }
                if (wt > 0.0f) denoise_var_tap_add(wt, denoise_lum(cq.x, cq.y, cq.z), s0, s1, s2);
            }
        v = denoise_var_spatial_result(s0, s1, s2);
    }
    var[pi] = v;
}

bool hist_grid(uint64_t items, uint32_t& out) {
    const uint64_t blocks = (items + kHistBlock - 1u) / kHistBlock;
    if (blocks > 0x7FFFFFFFull) return false;
    out = (uint32_t)blocks;
    return true;
}

}  // namespace

hipError_t launch_history_advance(const HistoryDev& a, hipStream_t stream) {
    const uint32_t W = a.prev_cam.W, H = a.prev_cam.H;
    if (!W || !H) return hipSuccess;
    const uint32_t gy = (H + kTileH - 1u) / kTileH;
    if (gy > 65535u || (uint64_t)W * H > 0xFFFFFFF0ull - kHistReasons) return hipErrorInvalidValue;   // a flat index is a map word
    const dim3 grid((W + kTileW - 1u) / kTileW, gy), block(kTileW, kTileH);
    if (a.gather == kHistGatherBilinear) hipLaunchKernelGGL(k_history_advance<kHistGatherBilinear>, grid, block, 0, stream, a);
    else if (a.gather == kHistGatherNearest) hipLaunchKernelGGL(k_history_advance<kHistGatherNearest>, grid, block, 0, stream, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_history_resolve(const float4* b, float* rgb, uint64_t pixels, const FeaturesDev& f, hipStream_t stream) {
    if (!pixels) return hipSuccess;
    uint32_t grid;
    if (!hist_grid(pixels, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_history_resolve, dim3(grid), dim3(kHistBlock), 0, stream, b, rgb, pixels, f);
    return hipGetLastError();
}

hipError_t launch_history_var(const float4* b, const float4* c, float* var, uint64_t pixels, uint32_t spatial_below,
                              hipStream_t stream) {
    if (!pixels) return hipSuccess;
    uint32_t grid;
    if (!hist_grid(pixels, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_history_var, dim3(grid), dim3(kHistBlock), 0, stream, b, c, var, pixels, spatial_below);
    return hipGetLastError();
}

hipError_t launch_history_var_fused(const float4* b, const float4* c, float* rgb, float* var, const float4* n_t, const float4* ga,
                                    const float4* pf, uint32_t w, uint32_t h, uint32_t spatial_below, uint32_t normal_power_log2,
                                    float sigma_plane, hipStream_t stream) {
    if (!w || !h) return hipSuccess;
    const uint32_t gy = (h + kTileH - 1u) / kTileH;
    if (gy > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_history_var_fused, dim3((w + kTileW - 1u) / kTileW, gy), dim3(kTileW, kTileH), 0, stream, b, c, rgb, var, n_t,
                       ga, pf, w, h, spatial_below, normal_power_log2, sigma_plane);
    return hipGetLastError();
}

}  // namespace romis
