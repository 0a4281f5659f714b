// history.h -- the reprojected image history (restir_history_*): per pixel a running mean, the population variance S of
// the samples and a sample count n, carried from one camera to the next -- the temporal half of SVGF (Schied et al.
// 2017).  One text for the kernel (history.hip k_history_advance / k_history_var), the host functions
// (restir_history_map_host / _fold / _advance_host / _variance_host, history_host.cpp) and the numpy restatements
// (tests/history_spec.py, tests/history_bilinear_spec.py):
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
// After an advance in the bilinear mode S is no longer the samples' population variance but the number whose S / (n - 1)
// estimates the variance of the blended mean ("the bilinear gather" below).
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

// ---- the bilinear gather (restir_history_gather_set(RESTIR_HISTORY_GATHER_BILINEAR)) ----------------------------------
// The nearest source pixel displaces the history by up to half a pixel per advance, and the displacements add up (README
// "Image history": a longer history is worse).  SVGF gathers its history through the 2 x 2 footprint around the continuous
// source position with a geometry test per tap; this is that gather.  Reasons 0 - 2 stay history_source's, range test on
// the nearest pixel included, so they mark the same pixels in both modes.
constexpr uint32_t kHistGatherNearest = 0u, kHistGatherBilinear = 1u;

// history_source with the continuous position (cfx, cfy) reproject_source gives (+0 where it gives none)
ROMIS_HD uint32_t history_source_at(const ReprojCam& cam, uint32_t cur_mat, uint32_t miss_material, float Px, float Py, float Pz,
                                    uint32_t& sx, uint32_t& sy, float& d, float& cfx, float& cfy) {
    sx = sy = 0u;
    d = 0.0f;
    float at[2] = {0.0f, 0.0f};
    const uint32_t why = cur_mat == miss_material ? kReprojMiss : reproject_source(cam, Px, Py, Pz, sx, sy, d, at);
    cfx = at[0];
    cfy = at[1];
    return why;
}

// The gathered state of a pixel whose history_source_at returned kReprojOk with (sx, sy, d, cfx, cfy).  Kept gives the
// record the history kept at pixel (tx, ty), G-buffer coordinates inside the image:
//     void test(tx, ty, nx, ny, nz, t, mat, n)   (N, t), the clamped material and the count: what history_accept reads
//     void load(tx, ty, HistState&)              mean, S and n
// x0 = floorf(cfx); fx = cfx - x0; gx = 1.0f - fx, the same for y.  Taps j = 0 .. 3 at (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
// (x0 + 1, y0 + 1) with w0 = gx gy, w1 = fx gy, w2 = gx fy, w3 = fx fy.  A tap contributes when it lies inside the image
// (tested on signed integers before any address is formed: x0 may be -1, x0 + 1 may be W), w_j > 0 and history_accept of
// its record returns kReprojOk; no other tap is load()ed, and one outside or of no weight is not test()ed either.  The
// nearest pixel (sx, sy) is one of the four, inside, with a weight of about 0.25 or more.
// No tap contributes: the reason history_accept gives for the nearest pixel is returned and s stays as it is -- so every
// pixel the nearest mode accepts is accepted here, and one both reject carries the same reason.
// Else kReprojOk.  sum = the contributing w_j added in tap order; v_j = w_j / sum (a division: a single tap has v = 1
// exactly); per channel mean = sum_j v_j mean_j and S = sum_j (v_j v_j) S_j, each accumulated in tap order from its first
// term; nf = sum_j v_j (float)n_j the same way, n = (uint32_t)floorf(nf + 0.5f), raised to 1 from 0.  A pixel with one
// contributing tap so carries that tap's record verbatim.  src is the map's entry: the flat G-buffer index of the nearest
// pixel when it contributes, else of the contributing tap of the largest weight, the first in tap order on a tie.
// What S means afterwards.  restir_history_denoise reads S / (n - 1) as the variance of the kept mean.  A blend of
// independent means with weights v_j has variance sum_j v_j^2 S_j / (n_j - 1), with equal counts (sum_j v_j^2 S_j) / (n - 1):
// after a bilinear advance S is the number whose S / (n - 1) estimates the variance of the mean, no longer the population
// variance of the samples, and the fold continues from it.  The rule ignores the correlation the blend creates between
// neighbouring pixels.  The plain average sum_j v_j S_j was tried in a CPU prototype and made the filtered result worse
// than this rule did (DESIGN.md §6 "Bilinear gather").
template <class Kept>
ROMIS_HD uint32_t history_gather_bilinear(const Kept& kept, uint32_t W, uint32_t H, uint32_t sx, uint32_t sy, float cfx, float cfy,
                                          float d, float cnx, float cny, float cnz, uint32_t cur_mat, uint32_t miss_material,
                                          HistState& s, uint32_t& src) {
    const float x0f = floorf(cfx), y0f = floorf(cfy);
    const float fx = cfx - x0f, fy = cfy - y0f;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const int64_t x0 = (int64_t)x0f, y0 = (int64_t)y0f;   // within [-1, W - 1] x [-1, H - 1] by the nearest pixel's range test
    const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    const uint32_t jn = (uint32_t)((int64_t)sx - x0) + 2u * (uint32_t)((int64_t)sy - y0);
    uint32_t mask = 0u, why_n = kHistNoHistory;
    float sum = 0.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 4u; j++) {
        const int64_t tx = x0 + (int64_t)(j & 1u), ty = y0 + (int64_t)(j >> 1);
        if (tx < 0 || ty < 0 || tx >= (int64_t)W || ty >= (int64_t)H || !(w[j] > 0.0f)) continue;
        float knx, kny, knz, kt;
        uint32_t kmat, kn;
        kept.test((uint32_t)tx, (uint32_t)ty, knx, kny, knz, kt, kmat, kn);
        const uint32_t why = history_accept(knx, kny, knz, kt, kmat, kn, cnx, cny, cnz, cur_mat, miss_material, d);
        if (j == jn) why_n = why;
        if (why == kReprojOk) {
            mask |= 1u << j;
            sum = sum + w[j];
        }
    }
    if (mask == 0u) return why_n;
    bool first = true;
    float nf = 0.0f, best = 0.0f;
    uint32_t bj = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 4u; j++) {
        if (!(mask & (1u << j))) continue;
        HistState k;
        kept.load((uint32_t)(x0 + (int64_t)(j & 1u)), (uint32_t)(y0 + (int64_t)(j >> 1)), k);
        const float v = w[j] / sum;
        const float vv = v * v;
        if (first) {
            s.mr = v * k.mr; s.mg = v * k.mg; s.mb = v * k.mb;
            s.sr = vv * k.sr; s.sg = vv * k.sg; s.sb = vv * k.sb;
            nf = v * (float)k.n;
            first = false;
        } else {
            s.mr = s.mr + v * k.mr; s.mg = s.mg + v * k.mg; s.mb = s.mb + v * k.mb;
            s.sr = s.sr + vv * k.sr; s.sg = s.sg + vv * k.sg; s.sb = s.sb + vv * k.sb;
            nf = nf + v * (float)k.n;
        }
        if (w[j] > best) {
            best = w[j];
            bj = j;
        }
    }
    const uint32_t n = (uint32_t)floorf(nf + 0.5f);
    s.n = n == 0u ? 1u : n;
    const uint32_t pick = (mask & (1u << jn)) ? jn : bj;
    src = (uint32_t)(y0 + (int64_t)(pick >> 1)) * W + (uint32_t)(x0 + (int64_t)(pick & 1u));
    return kReprojOk;
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

// the host's Kept of history_gather_bilinear: the planes of restir_history_advance_host
struct HistKeptHost {
    const float* n_t;           // G-buffer rows
    const uint32_t* material;   // G-buffer rows, not clamped
    const float* mean;          // image rows
    const float* S;
    const uint32_t* n;
    uint32_t w, h, miss_material;
    void test(uint32_t tx, uint32_t ty, float& nx, float& ny, float& nz, float& t, uint32_t& mat, uint32_t& cnt) const {
        const size_t q = (size_t)ty * w + tx;
        nx = n_t[4 * q]; ny = n_t[4 * q + 1]; nz = n_t[4 * q + 2]; t = n_t[4 * q + 3];
        mat = history_material(material[q], miss_material);
        cnt = n[(size_t)(h - 1u - ty) * w + tx];
    }
    void load(uint32_t tx, uint32_t ty, HistState& s) const {
        const size_t qi = (size_t)(h - 1u - ty) * w + tx;
        s.mr = mean[3 * qi]; s.mg = mean[3 * qi + 1]; s.mb = mean[3 * qi + 2];
        s.sr = S[3 * qi]; s.sg = S[3 * qi + 1]; s.sb = S[3 * qi + 2];
        s.n = n[qi];
    }
};

// One whole advance in either mode, k_history_advance's text: the map (nullable), the gather and the fold.  kept_n_t ==
// nullptr: nothing kept.  The outputs must not overlap the inputs.
inline void history_advance_host(const ReprojCam& cam, const float* cur_n_t, const float* cur_p_mat, const float* kept_n_t,
                                 const uint32_t* kept_material, const float* mean_in, const float* S_in, const uint32_t* n_in,
                                 const float* x, uint32_t miss_material, uint32_t max_frames, uint32_t gather, float* mean_out,
                                 float* S_out, uint32_t* n_out, uint32_t* map) {
    const uint32_t w = cam.W, h = cam.H;
    const HistKeptHost kept{kept_n_t, kept_material, mean_in, S_in, n_in, w, h, miss_material};
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t px = 0; px < w; px++) {
            const size_t gi = (size_t)y * w + px, pi = (size_t)(h - 1u - y) * w + px;
            uint32_t why = kHistNoHistory, src = 0u;
            HistState s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
            if (kept_n_t) {
                const float* cn = cur_n_t + 4 * gi;
                const float* cp = cur_p_mat + 4 * gi;
                const uint32_t cur_mat = history_material(denoise_bits(cp[3]), miss_material);
                uint32_t sx, sy;
                float d, cfx, cfy;
                why = history_source_at(cam, cur_mat, miss_material, cp[0], cp[1], cp[2], sx, sy, d, cfx, cfy);
                if (why == kReprojOk && gather == kHistGatherBilinear) {
                    why = history_gather_bilinear(kept, w, h, sx, sy, cfx, cfy, d, cn[0], cn[1], cn[2], cur_mat, miss_material, s, src);
                } else if (why == kReprojOk) {
                    float knx, kny, knz, kt;
                    uint32_t kmat, kn;
                    kept.test(sx, sy, knx, kny, knz, kt, kmat, kn);
                    why = history_accept(knx, kny, knz, kt, kmat, kn, cn[0], cn[1], cn[2], cur_mat, miss_material, d);
                    if (why == kReprojOk) {
                        kept.load(sx, sy, s);
                        src = sy * w + sx;
                    }
                }
            }
            history_fold(x[3 * pi], x[3 * pi + 1], x[3 * pi + 2], max_frames, s);
            mean_out[3 * pi] = s.mr; mean_out[3 * pi + 1] = s.mg; mean_out[3 * pi + 2] = s.mb;
            S_out[3 * pi] = s.sr; S_out[3 * pi + 1] = s.sg; S_out[3 * pi + 2] = s.sb;
            n_out[pi] = s.n;
            if (map) map[gi] = why == kReprojOk ? src : 0xFFFFFFFFu - why;
        }
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
    uint32_t gather;               // kHistGatherNearest / kHistGatherBilinear: which instantiation is launched (last: no kernel reads it)
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
