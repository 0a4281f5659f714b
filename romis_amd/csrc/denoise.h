// denoise.h -- the edge-avoiding a-trous wavelet filter of restir_denoise / restir_denoise_host (Dammertz et al. 2010)
// over the context's last image, guided by the normal, the position and the material of the view's G-buffer.  The
// per-pixel guide and the per-tap weight live here once: k_denoise_guides / k_denoise_level (denoise.hip) and the host's
// denoise_host compile the same text, both without contraction and with correctly rounded divide and sqrt, and visit the
// taps in the same order -- dy = -2..2 outside (image rows), dx = -2..2 inside -- so the two agree bit for bit
// (include/restir_c.h has the contract, DESIGN.md §6 "Denoising a frame" the mapping).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROMIS_DENOISE_HD __host__ __device__ __forceinline__
#else
#define ROMIS_DENOISE_HD inline
#endif

namespace romis {

constexpr uint32_t kDenoiseMaxIterations = 5;    // RESTIR_DENOISE_MAX_ITERATIONS
constexpr uint32_t kDenoiseMaxNormalPower = 7;   // normal_power_log2's largest value

// A pixel's guide: the normalised normal g, the material's bits, the position P and whether the pixel is flat -- a
// miss, or a normal without a direction --, two 16-byte records
struct DenoiseGuide {
    float gx, gy, gz;
    uint32_t mat;
    float px, py, pz;
    uint32_t flat;
};

ROMIS_DENOISE_HD uint32_t denoise_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

// |v| <= FLT_MAX <=> v is finite (a NaN fails the comparison)
ROMIS_DENOISE_HD bool denoise_finite(float v) {
    const float big = 3.402823466e+38f;
    const float a = v < 0.0f ? -v : v;
    return a <= big;
}
ROMIS_DENOISE_HD bool denoise_finite3(float x, float y, float z) {
    return denoise_finite(x) && denoise_finite(y) && denoise_finite(z);
}

// The guide of the G-buffer record n_t = (N unnormalised, t), p_mat = (P, bits(material)), once per pixel
ROMIS_DENOISE_HD void denoise_guide(float nx, float ny, float nz, float px, float py, float pz, uint32_t mat,
                                    uint32_t miss_material, DenoiseGuide& g) {
    const float l2 = (nx * nx + ny * ny) + nz * nz;   // vdot's order
    const bool flat = mat == miss_material || !(l2 > 0.0f) || !denoise_finite(l2);
    g.gx = 0.0f; g.gy = 0.0f; g.gz = 0.0f;
    if (!flat) {
        const float r = sqrtf(l2);
        g.gx = nx / r; g.gy = ny / r; g.gz = nz / r;
    }
    g.mat = mat;
    g.px = px; g.py = py; g.pz = pz;
    g.flat = flat ? 1u : 0u;
}

// 1.0f / (sigma_plane * t) of the centre pixel: the plane term's scale, once per pixel and level
ROMIS_DENOISE_HD float denoise_inv_s(float sigma_plane, float t) { return 1.0f / (sigma_plane * t); }

// The B3 kernel (1/16, 1/4, 3/8, 1/4, 1/16) at d = -2..2; a product of two entries is exact
ROMIS_DENOISE_HD float denoise_k(int d) {
    const int a = d < 0 ? -d : d;
    return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f);
}

// The weight of a tap q other than the centre, whose colour is finite, for centre p; h = k[dy] k[dx].  The tap
// contributes only when the result is > 0 (a NaN fails that test)
ROMIS_DENOISE_HD float denoise_tap_weight(const DenoiseGuide& p, const DenoiseGuide& q, float h, float inv_s,
                                          uint32_t normal_power_log2) {
    if (q.mat != p.mat) return 0.0f;
    if (p.flat != 0u && q.flat != 0u) return h;
    if (p.flat != 0u || q.flat != 0u) return 0.0f;
    float cn = (p.gx * q.gx + p.gy * q.gy) + p.gz * q.gz;
    cn = cn > 0.0f ? cn : 0.0f;
    for (uint32_t i = 0; i < normal_power_log2; i++) cn = cn * cn;
    const float dx = q.px - p.px, dy = q.py - p.py, dz = q.pz - p.pz;
    const float e = (p.gx * dx + p.gy * dy) + p.gz * dz;
    const float r = e * inv_s;
    const float wp = 1.0f - r * r;
    return h * (cn * wp);
}

// sw += w, sc += w c -- one contributing tap
ROMIS_DENOISE_HD void denoise_tap_add(float w, float cx, float cy, float cz, float& sw, float& sx, float& sy, float& sz) {
    sw = sw + w;
    sx = sx + w * cx;
    sy = sy + w * cy;
    sz = sz + w * cz;
}

// The whole filter on the host: rgb (w x h float3, row 0 = top), n_t / p_mat (w x h float4, row y = 0 at the bottom: the
// image row of G-buffer row y is h - 1 - y) -> out.  guides: w * h records, tmp: 2 * 3 * w * h floats of scratch.
inline void denoise_host(const float* rgb, const float* n_t, const float* p_mat, uint32_t w, uint32_t h, uint32_t miss_material,
                         uint32_t iterations, uint32_t normal_power_log2, float sigma_plane, float* out,
                         DenoiseGuide* guides, float* tvals, float* tmp) {
    const size_t npx = (size_t)w * h;
    // guides in image rows
    for (uint32_t r = 0; r < h; r++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t gi = (size_t)(h - 1u - r) * w + x, pi = (size_t)r * w + x;
            const float* n = n_t + 4 * gi;
            const float* pm = p_mat + 4 * gi;
            denoise_guide(n[0], n[1], n[2], pm[0], pm[1], pm[2], denoise_bits(pm[3]), miss_material, guides[pi]);
            tvals[pi] = n[3];
        }
    const float* in = rgb;
    for (uint32_t level = 0; level < iterations; level++) {
        float* o = level + 1u == iterations ? out : tmp + (size_t)(level & 1u) * 3 * npx;
        const int64_t s = (int64_t)1 << level;
        for (uint32_t r = 0; r < h; r++)
            for (uint32_t x = 0; x < w; x++) {
                const size_t pi = (size_t)r * w + x;
                const float* c = in + 3 * pi;
                float* op = o + 3 * pi;
                if (!denoise_finite3(c[0], c[1], c[2])) {   // the input's bits
                    memcpy(op, c, 12);
                    continue;
                }
                const DenoiseGuide& gp = guides[pi];
                const float inv_s = denoise_inv_s(sigma_plane, tvals[pi]);
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                for (int dy = -2; dy <= 2; dy++)
                    for (int dx = -2; dx <= 2; dx++) {
                        const int64_t qx = (int64_t)x + s * dx, qy = (int64_t)r + s * dy;
                        if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) continue;
                        const size_t qi = (size_t)qy * w + (size_t)qx;
                        const float* cq = in + 3 * qi;
                        if (!denoise_finite3(cq[0], cq[1], cq[2])) continue;
                        const float hk = denoise_k(dy) * denoise_k(dx);
                        const float wt = (dx == 0 && dy == 0) ? hk : denoise_tap_weight(gp, guides[qi], hk, inv_s, normal_power_log2);
                        if (wt > 0.0f) denoise_tap_add(wt, cq[0], cq[1], cq[2], sw, sx, sy, sz);
                    }
                op[0] = sx / sw; op[1] = sy / sw; op[2] = sz / sw;
            }
        in = o;
    }
}

// ---- restir_denoise_lum / restir_denoise_lum_host: the same filter with a variance-guided luminance term ----------------
// (include/restir_c.h "denoising with a variance-guided luminance term").  k_denoise_var_spatial, k_denoise_var_accum and
// k_denoise_level<true> (denoise.hip) and denoise_lum_host below compile this text.

// l(c) = (0.2126 r + 0.7152 g) + 0.0722 b
ROMIS_DENOISE_HD float denoise_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// A variance as the planes store it: a value that is not finite, or not > 0, is +0
ROMIS_DENOISE_HD float denoise_var_clean(float v) { return (v > 0.0f && denoise_finite(v)) ? v : 0.0f; }

// RESTIR_DENOISE_VAR_ACCUM's variance of a pixel from its three m2 entries; inv = 1.0f / ((float)n * (float)(n - 1)).
// The channels' standard errors are added before squaring: one contribution weight scales all three channels of a sample
ROMIS_DENOISE_HD float denoise_var_of_m2(float m2r, float m2g, float m2b, float inv) {
    const float sl = denoise_lum(sqrtf(m2r * inv), sqrtf(m2g * inv), sqrtf(m2b * inv));
    return denoise_var_clean(sl * sl);
}

// One tap of RESTIR_DENOISE_VAR_SPATIAL's 7 x 7 window: s0 += w, s1 += w l, s2 += w (l l)
ROMIS_DENOISE_HD void denoise_var_tap_add(float w, float l, float& s0, float& s1, float& s2) {
    s0 = s0 + w;
    s1 = s1 + w * l;
    s2 = s2 + w * (l * l);
}
ROMIS_DENOISE_HD float denoise_var_spatial_result(float s0, float s1, float s2) {
    const float m1 = s1 / s0;
    return denoise_var_clean(s2 / s0 - m1 * m1);
}

// The Gaussian (1/4, 1/2, 1/4) of the pre-filtered variance at d = -1..1; a product of two entries is exact
ROMIS_DENOISE_HD float denoise_g(int d) { return d == 0 ? 0.5f : 0.25f; }

// 1.0f / (sigma_lum sqrt(gv) + 1e-6f) of the centre pixel, once per pixel and level
ROMIS_DENOISE_HD float denoise_inv_den(float sigma_lum, float gv) { return 1.0f / (sigma_lum * sqrtf(gv) + 1e-6f); }

// The luminance factor of a tap other than the centre: 1 / (1 + r r), r = |l_q - l_p| inv_den.  An infinite r gives 0
ROMIS_DENOISE_HD float denoise_lum_weight(float lq, float lp, float inv_den) {
    const float r = fabsf(lq - lp) * inv_den;
    return 1.0f / (1.0f + r * r);
}

// The initial variance plane of RESTIR_DENOISE_VAR_SPATIAL on the host; rgb and var in image rows, guides as denoise_host's
inline void denoise_var_spatial_host(const float* rgb, const DenoiseGuide* guides, const float* tvals, uint32_t w, uint32_t h,
                                     uint32_t normal_power_log2, float sigma_plane, float* var) {
    for (uint32_t r = 0; r < h; r++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t pi = (size_t)r * w + x;
            const float* c = rgb + 3 * pi;
            var[pi] = 0.0f;
            if (!denoise_finite3(c[0], c[1], c[2])) continue;
            const DenoiseGuide& gp = guides[pi];
            const float inv_s = denoise_inv_s(sigma_plane, tvals[pi]);
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int dy = -3; dy <= 3; dy++)
                for (int dx = -3; dx <= 3; dx++) {
                    const int64_t qx = (int64_t)x + dx, qy = (int64_t)r + dy;
                    if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) continue;
                    const size_t qi = (size_t)qy * w + (size_t)qx;
                    const float* cq = rgb + 3 * qi;
                    if (!denoise_finite3(cq[0], cq[1], cq[2])) continue;
                    const float wt = (dx == 0 && dy == 0) ? 1.0f : denoise_tap_weight(gp, guides[qi], 1.0f, inv_s, normal_power_log2);
                    if (wt > 0.0f) denoise_var_tap_add(wt, denoise_lum(cq[0], cq[1], cq[2]), s0, s1, s2);
                }
            var[pi] = denoise_var_spatial_result(s0, s1, s2);
        }
}

// The whole luminance filter on the host.  var (nullable): the initial variance plane in image rows, cleaned as it is
// read; NULL: the spatial estimate.  out_var (nullable): the last level's variance plane.  guides / tvals as
// denoise_host's, tmp: 2 * 3 * w * h floats, vtmp: 2 * w * h floats of scratch.
inline void denoise_lum_host(const float* rgb, const float* var, const float* n_t, const float* p_mat, uint32_t w, uint32_t h,
                             uint32_t miss_material, uint32_t iterations, uint32_t normal_power_log2, float sigma_plane,
                             float sigma_lum, float* out, float* out_var, DenoiseGuide* guides, float* tvals, float* tmp,
                             float* vtmp) {
    const size_t npx = (size_t)w * h;
    for (uint32_t r = 0; r < h; r++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t gi = (size_t)(h - 1u - r) * w + x, pi = (size_t)r * w + x;
            const float* n = n_t + 4 * gi;
            const float* pm = p_mat + 4 * gi;
            denoise_guide(n[0], n[1], n[2], pm[0], pm[1], pm[2], denoise_bits(pm[3]), miss_material, guides[pi]);
            tvals[pi] = n[3];
        }
    if (var)
        for (size_t i = 0; i < npx; i++) vtmp[i] = denoise_var_clean(var[i]);
    else
        denoise_var_spatial_host(rgb, guides, tvals, w, h, normal_power_log2, sigma_plane, vtmp);
    const float* in = rgb;
    const float* vin = vtmp;
    for (uint32_t level = 0; level < iterations; level++) {
        float* o = level + 1u == iterations ? out : tmp + (size_t)(level & 1u) * 3 * npx;
        float* vo = vtmp + (size_t)((level + 1u) & 1u) * npx;
        const int64_t s = (int64_t)1 << level;
        for (uint32_t r = 0; r < h; r++)
            for (uint32_t x = 0; x < w; x++) {
                const size_t pi = (size_t)r * w + x;
                const float* c = in + 3 * pi;
                float* op = o + 3 * pi;
                if (!denoise_finite3(c[0], c[1], c[2])) {   // the input's bits, and its variance
                    memcpy(op, c, 12);
                    vo[pi] = vin[pi];
                    continue;
                }
                float gnum = 0.0f, gden = 0.0f;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int64_t qx = (int64_t)x + dx, qy = (int64_t)r + dy;
                        if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) continue;
                        const float gw = denoise_g(dy) * denoise_g(dx);
                        gnum = gnum + gw * vin[(size_t)qy * w + (size_t)qx];
                        gden = gden + gw;
                    }
                const float inv_den = denoise_inv_den(sigma_lum, gnum / gden);
                const float lp = denoise_lum(c[0], c[1], c[2]);
                const DenoiseGuide& gp = guides[pi];
                const float inv_s = denoise_inv_s(sigma_plane, tvals[pi]);
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
                for (int dy = -2; dy <= 2; dy++)
                    for (int dx = -2; dx <= 2; dx++) {
                        const int64_t qx = (int64_t)x + s * dx, qy = (int64_t)r + s * dy;
                        if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) continue;
                        const size_t qi = (size_t)qy * w + (size_t)qx;
                        const float* cq = in + 3 * qi;
                        if (!denoise_finite3(cq[0], cq[1], cq[2])) continue;
                        const float hk = denoise_k(dy) * denoise_k(dx);
                        const float wt = (dx == 0 && dy == 0)
                                             ? hk
                                             : denoise_tap_weight(gp, guides[qi], hk, inv_s, normal_power_log2) *
                                                   denoise_lum_weight(denoise_lum(cq[0], cq[1], cq[2]), lp, inv_den);
                        if (wt > 0.0f) {
                            denoise_tap_add(wt, cq[0], cq[1], cq[2], sw, sx, sy, sz);
                            sv = sv + (wt * wt) * vin[qi];
                        }
                    }
                op[0] = sx / sw; op[1] = sy / sw; op[2] = sz / sw;
                vo[pi] = sv / (sw * sw);
            }
        in = o;
        vin = vo;
    }
    if (out_var) memcpy(out_var, vin, npx * sizeof(float));
}

#if defined(__HIPCC__)
struct FeaturesDev;

// Both enqueue on `stream` and never synchronise.  Planes hold w x h pixels of the owned rectangle; n_t / p_mat and the
// guide planes are in G-buffer rows (y = 0 bottom), images in image rows (row 0 = top).
// ga <- (g, bits(material)), p_mat <- (P, flat) in place; n_t keeps t
hipError_t launch_denoise_guides(const float4* n_t, float4* p_mat, float4* ga, uint64_t pixels, uint32_t miss_material,
                                 hipStream_t stream);
// out <- level `level` (step 2^level) of in; tone (nullable): tone_map_rgb of the result, the last level's
hipError_t launch_denoise_level(const float* in, float* out, const float4* n_t, const float4* ga, const float4* pf, uint32_t w,
                                uint32_t h, uint32_t level, uint32_t normal_power_log2, float sigma_plane, const FeaturesDev* tone,
                                hipStream_t stream);
// restir_denoise_lum's.  Variance planes: one float per pixel, image rows.
// var <- RESTIR_DENOISE_VAR_SPATIAL's estimate over the image in
hipError_t launch_denoise_var_spatial(const float* in, float* var, const float4* n_t, const float4* ga, const float4* pf, uint32_t w,
                                      uint32_t h, uint32_t normal_power_log2, float sigma_plane, hipStream_t stream);
// rgb <- mean, var <- RESTIR_DENOISE_VAR_ACCUM's plane of m2; the accumulator's planes are in image rows like the image
hipError_t launch_denoise_var_accum(const float* mean, const float* m2, float* rgb, float* var, uint64_t pixels, float inv,
                                    hipStream_t stream);
// launch_denoise_level with the luminance term: reads var_in, writes var_out
hipError_t launch_denoise_level_lum(const float* in, float* out, const float* var_in, float* var_out, const float4* n_t,
                                    const float4* ga, const float4* pf, uint32_t w, uint32_t h, uint32_t level,
                                    uint32_t normal_power_log2, float sigma_plane, float sigma_lum, const FeaturesDev* tone,
                                    hipStream_t stream);
#endif

}  // namespace romis
