// history.h -- the reprojected image history (restir_history_*): per pixel a running mean, the population variance S of
// the samples and a sample count n, carried from one camera to the next -- the temporal half of SVGF (Schied et al.
// 2017).  One text for the kernel (history.hip k_history_advance / k_history_var), the host functions
// (restir_history_map_host / _fold / _variance_host, history_host.cpp) and tests/history_spec.py's numpy restatement:
// every step is a single float32 operation in a fixed order, compiled with -ffp-contract=off and correctly rounded
// divide / sqrt on both sides, so the three agree bit for bit (include/restir_c.h "a reprojected image history",
// DESIGN.md §6 "Image history").
//
// The record a pixel keeps: (N unnormalised, t) as the G-buffer's n_t holds it, the material's bits clamped to the miss
// material like k_reproject's is_miss, mean.rgb, S.rgb and n.  Two sets, since an advance gathers from other pixels:
// three 16-byte planes per set -- (N, t), (mean, bits n), (S, bits material) -- 96 bytes per pixel for both, 190 MiB at
// 1920 x 1080.
//
// Rows.  The G-buffer records -- the current view's guide planes, the host functions' n_t / p_mat / kept_n_t /
// kept_material and the map, entries and indices alike -- are in G-buffer rows (y = 0 at the bottom), as
// restir_frame_reproject's are.  The image and every state plane (mean, S, n; the device's own copy of N, t and the
// material too) are in image rows (row 0 = top): image row r is G-buffer row h - 1 - r.
//
// The variance of the mean the filter reads is S / (n - 1).  While n is below max_frames that is Welford's m2 / (n (n - 1))
// exactly; once the cap is reached mean and S are exponential averages with alpha = a = 1 / max_frames, whose variance
// of the mean is S a / (2 - a) in the steady state, so S / (n - 1) over-states it by (2 - a) / (a (n - 1)) -- up to
// about 2 x.  The bias is conservative (the luminance term opens wider); README "Image history" has what it costs.
#pragma once

#include "denoise.h"
#include "reproject.h"

namespace romis {

// restir_history_advance's reasons beyond restir_frame_reproject's 0 .. 5
constexpr uint32_t kHistMaterial = 6u;    // the kept material at the source pixel is not the current pixel's
constexpr uint32_t kHistNoHistory = 7u;   // nothing kept: the first advance, one after a reset, a record with n == 0
constexpr uint32_t kHistReasons = 8u;

constexpr uint32_t kHistMaxFrames = (1u << 24) - 1u;   // RESTIR_ACCUM_MAX_FRAMES: (float)n is exact

struct HistState {
    float mr, mg, mb;
    float sr, sg, sb;
    uint32_t n;
};

// make_px's clamp: every index at or above the miss material's is the miss material
ROMIS_HD uint32_t history_material(uint32_t bits, uint32_t miss_material) { return bits < miss_material ? bits : miss_material; }

// Steps 1 - 3 of restir_frame_reproject for a current record: kReprojOk with the source pixel (sx, sy) (G-buffer
// coordinates of the predecessor's image) and the depth d it must show, else kReprojMiss / Behind / OffScreen
ROMIS_HD uint32_t history_source(const ReprojCam& cam, uint32_t cur_mat, uint32_t miss_material, float Px, float Py, float Pz,
                                 uint32_t& sx, uint32_t& sy, float& d) {
    sx = sy = 0u;
    d = 0.0f;
    if (cur_mat == miss_material) return kReprojMiss;
    return reproject_source(cam, Px, Py, Pz, sx, sy, d);
}

// Steps 4 - 5 against the record kept at the source pixel, then the material (6) and the count (7).  Materials clamped.
ROMIS_HD uint32_t history_accept(float knx, float kny, float knz, float kt, uint32_t kept_mat, uint32_t kept_n, float cnx,
                                 float cny, float cnz, uint32_t cur_mat, uint32_t miss_material, float d) {
    if (kept_mat == miss_material) return kReprojPrevMiss;
    const uint32_t why = reproject_similar(knx, kny, knz, kt, cnx, cny, cnz, d);
    if (why != kReprojOk) return why;
    if (kept_mat != cur_mat) return kHistMaterial;
    if (kept_n == 0u) return kHistNoHistory;
    return kReprojOk;
}

// The gathered state s takes the image value x.  A finite x: n' = min(n + 1, max_frames), a = 1.0f / (float)n', and per
// channel d = x - mean; mean' = mean + d a; dd = d d; t = a dd; u = S + t; om = 1.0f - a; S' = om u.  With a = 1 / n
// that is accum_fold_mean's mean and Welford's m2' / n.  An x that is not finite leaves s as it is; an empty s (n == 0)
// then shows x's bits with S = +0 and stays empty.
ROMIS_HD void history_fold(float xr, float xg, float xb, uint32_t max_frames, HistState& s) {
    if (!denoise_finite3(xr, xg, xb)) {
        if (s.n == 0u) {
            s.mr = xr; s.mg = xg; s.mb = xb;
            s.sr = 0.0f; s.sg = 0.0f; s.sb = 0.0f;
        }
        return;
    }
    const uint32_t n1 = s.n < max_frames ? s.n + 1u : max_frames;
    const float a = 1.0f / (float)n1;
    const float om = 1.0f - a;
    {
        const float d = xr - s.mr;
        s.mr = s.mr + d * a;
        const float dd = d * d;
        const float t = a * dd;
        const float u = s.sr + t;
        s.sr = om * u;
    }
    {
        const float d = xg - s.mg;
        s.mg = s.mg + d * a;
        const float dd = d * d;
        const float t = a * dd;
        const float u = s.sg + t;
        s.sg = om * u;
    }
    {
        const float d = xb - s.mb;
        s.mb = s.mb + d * a;
        const float dd = d * d;
        const float t = a * dd;
        const float u = s.sb + t;
        s.sb = om * u;
    }
    s.n = n1;
}

// The variance plane's entry of a pixel whose mean is finite and whose n >= spatial_below (>= 2): denoise_var_of_m2 of S
// with inv = 1.0f / (float)(n - 1).  false: the pixel takes RESTIR_DENOISE_VAR_SPATIAL's estimate over the mean image.
ROMIS_HD bool history_var_temporal(const HistState& s, uint32_t spatial_below, float& v) {
    if (s.n < spatial_below || !denoise_finite3(s.mr, s.mg, s.mb)) return false;
    const float inv = 1.0f / (float)(s.n - 1u);
    v = denoise_var_of_m2(s.sr, s.sg, s.sb, inv);
    return true;
}

// ---- the whole-image host functions (history_host.cpp) ---------------------------------------------------------------
// The map of an advance.  cur_n_t / cur_p_mat: the current camera's G-buffer; kept_n_t / kept_material / kept_n: what the
// history kept from the advance before (kept_n in image rows), all three nullptr: nothing kept, every entry is reason 7.
inline void history_map_host(const ReprojCam& cam, const float* cur_n_t, const float* cur_p_mat, const float* kept_n_t,
                             const uint32_t* kept_material, const uint32_t* kept_n, uint32_t miss_material, uint32_t* map) {
    const uint32_t w = cam.W, h = cam.H;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            uint32_t why = kHistNoHistory;
            size_t q = 0;
            if (kept_n) {
                const float* cn = cur_n_t + 4 * p;
                const float* cp = cur_p_mat + 4 * p;
                const uint32_t cur_mat = history_material(denoise_bits(cp[3]), miss_material);
                uint32_t sx, sy;
                float d;
                why = history_source(cam, cur_mat, miss_material, cp[0], cp[1], cp[2], sx, sy, d);
                if (why == kReprojOk) {
                    q = (size_t)sy * w + sx;
                    const float* kn = kept_n_t + 4 * q;
                    why = history_accept(kn[0], kn[1], kn[2], kn[3], history_material(kept_material[q], miss_material),
                                         kept_n[(size_t)(h - 1u - sy) * w + sx], cn[0], cn[1], cn[2], cur_mat, miss_material, d);
                }
            }
            map[p] = why == kReprojOk ? (uint32_t)q : 0xFFFFFFFFu - why;
        }
}

// false: a map entry names a pixel outside the image (nothing is written)
inline bool history_fold_host(const float* mean_in, const float* S_in, const uint32_t* n_in, const uint32_t* map, const float* x,
                              uint32_t w, uint32_t h, uint32_t max_frames, float* mean_out, float* S_out, uint32_t* n_out) {
    const size_t npx = (size_t)w * h;
    for (size_t i = 0; i < npx; i++)
        if (map[i] <= 0xFFFFFFFFu - kHistReasons && map[i] >= npx) return false;
    for (uint32_t r = 0; r < h; r++)
        for (uint32_t px = 0; px < w; px++) {
            const size_t pi = (size_t)r * w + px;
            const uint32_t m = map[(size_t)(h - 1u - r) * w + px];
            HistState s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
            if (m <= 0xFFFFFFFFu - kHistReasons) {
                const size_t qi = (size_t)(h - 1u - m / w) * w + m % w;
                s.mr = mean_in[3 * qi]; s.mg = mean_in[3 * qi + 1]; s.mb = mean_in[3 * qi + 2];
                s.sr = S_in[3 * qi]; s.sg = S_in[3 * qi + 1]; s.sb = S_in[3 * qi + 2];
                s.n = n_in[qi];
            }
            history_fold(x[3 * pi], x[3 * pi + 1], x[3 * pi + 2], max_frames, s);
            mean_out[3 * pi] = s.mr; mean_out[3 * pi + 1] = s.mg; mean_out[3 * pi + 2] = s.mb;
            S_out[3 * pi] = s.sr; S_out[3 * pi + 1] = s.sg; S_out[3 * pi + 2] = s.sb;
            n_out[pi] = s.n;
        }
    return true;
}

// The initial variance plane of restir_history_denoise.  guides / tvals: w * h entries of scratch, as denoise_host's.
inline void history_variance_host(const float* mean, const float* S, const uint32_t* n, const float* n_t, const float* p_mat,
                                  uint32_t w, uint32_t h, uint32_t miss_material, uint32_t spatial_below,
                                  uint32_t normal_power_log2, float sigma_plane, float* var, DenoiseGuide* guides, float* tvals) {
    for (uint32_t r = 0; r < h; r++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t gi = (size_t)(h - 1u - r) * w + x, pi = (size_t)r * w + x;
            const float* nn = n_t + 4 * gi;
            const float* pm = p_mat + 4 * gi;
            denoise_guide(nn[0], nn[1], nn[2], pm[0], pm[1], pm[2], denoise_bits(pm[3]), miss_material, guides[pi]);
            tvals[pi] = nn[3];
        }
    denoise_var_spatial_host(mean, guides, tvals, w, h, normal_power_log2, sigma_plane, var);
    const size_t npx = (size_t)w * h;
    for (size_t i = 0; i < npx; i++) {
        const HistState s{mean[3 * i], mean[3 * i + 1], mean[3 * i + 2], S[3 * i], S[3 * i + 1], S[3 * i + 2], n[i]};
        float v;
        if (history_var_temporal(s, spatial_below, v)) var[i] = v;
    }
}

#if defined(__HIPCC__)
struct FeaturesDev;

// One launch of k_history_advance over W x H pixels (prev_cam.W x prev_cam.H)
struct HistoryDev {
    ReprojCam prev_cam;            // the camera of the advance before
    uint32_t miss_mat;
    uint32_t max_frames;
    uint32_t fresh;                // 1: nothing kept, every pixel is reason 7 and no kept plane is read
    const float4* cur_nt;          // the current view's guide planes, G-buffer rows: (N, t)
    const float4* cur_pf;          // (P, flat)
    const float4* cur_ga;          // (g, bits(material))
    const float* x;                // the image, 3 floats per pixel, image rows
    const float4* in_a;            // the kept set, image rows: (N, t)
    const float4* in_b;            // (mean, bits(n))
    const float4* in_c;            // (S, bits(material))
    float4* out_a;                 // the other set
    float4* out_b;
    float4* out_c;
    uint32_t* map;                 // nullable, G-buffer rows: the source's flat G-buffer index, or 0xFFFFFFFF - reason
};

// All enqueue on `stream` and never synchronise.
hipError_t launch_history_advance(const HistoryDev& a, hipStream_t stream);
// rgb <- tone_map_rgb(f, mean) per pixel (f.tone_map == 0: the mean's bits); b: the (mean, n) plane
hipError_t launch_history_resolve(const float4* b, float* rgb, uint64_t pixels, const FeaturesDev& f, hipStream_t stream);
// var[p] <- history_var_temporal's value where it applies; every other entry stays (the spatial estimate, written before)
hipError_t launch_history_var(const float4* b, const float4* c, float* var, uint64_t pixels, uint32_t spatial_below,
                              hipStream_t stream);
// The same plane and the packed mean image (rgb <- mean's bits) in one launch: the spatial estimate is computed only for
// the pixels that take it.  Planes as launch_denoise_var_spatial's; w x h pixels.
hipError_t launch_history_var_fused(const float4* b, const float4* c, float* rgb, float* var, const float4* n_t, const float4* ga,
                                    const float4* pf, uint32_t w, uint32_t h, uint32_t spatial_below, uint32_t normal_power_log2,
                                    float sigma_plane, hipStream_t stream);
#endif

}  // namespace romis
