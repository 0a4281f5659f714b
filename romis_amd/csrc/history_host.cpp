// history_host.cpp -- restir_history_params_default and the pure host side of the image history: restir_history_fold,
// restir_history_map_host, restir_history_advance_host and restir_history_variance_host, the kernels' own text
// (history.h) compiled without contraction.  No HIP header and no HIP call: a stand-alone program links this unit,
// denoise_host.cpp and abi_error.cpp alone (tests/cpp/history_host_check.cpp, history_advance_host_check.cpp).
#include "abi_error.h"
#include "history.h"

#include <cmath>
#include <new>
#include <vector>

using namespace romis;

namespace romis {

restir_status denoise_params_check(const restir_denoise_params* p, const char* who);   // denoise_host.cpp

// the parameter checks restir_history_begin and restir_history_variance_host share
restir_status history_params_check(const restir_history_params* p, const char* who) {
    if (!p) return fail(RESTIR_ERR_INVALID, "%s: params is NULL", who);
    if (p->max_frames < 1u || p->max_frames > kHistMaxFrames)
        return fail(RESTIR_ERR_INVALID, "%s: max_frames %u outside 1..%u", who, p->max_frames, kHistMaxFrames);
    if (p->spatial_below < 2u) return fail(RESTIR_ERR_INVALID, "%s: spatial_below %u below 2", who, p->spatial_below);
    if (p->flags != 0u || p->reserved != 0u)
        return fail(RESTIR_ERR_INVALID, "%s: flags %u, reserved %u (none is defined)", who, p->flags, p->reserved);
    return RESTIR_OK;
}

}  // namespace romis

extern "C" {

void restir_history_params_default(restir_history_params* out) {
    if (!out) return;
    out->max_frames = 8;
    out->spatial_below = 4;
    out->flags = 0;
    out->reserved = 0;
}

restir_status restir_history_fold(const float* mean_in, const float* S_in, const uint32_t* n_in, const uint32_t* map,
                                  const float* x, uint32_t w, uint32_t h, uint32_t max_frames, float* mean_out, float* S_out,
                                  uint32_t* n_out) {
    if (!mean_in || !S_in || !n_in || !map || !x || !mean_out || !S_out || !n_out)
        return fail(RESTIR_ERR_INVALID, "restir_history_fold: null argument");
    if (w == 0 || h == 0) return fail(RESTIR_ERR_INVALID, "restir_history_fold: empty image %ux%u", w, h);
    if (max_frames < 1u || max_frames > kHistMaxFrames)
        return fail(RESTIR_ERR_INVALID, "restir_history_fold: max_frames %u outside 1..%u", max_frames, kHistMaxFrames);
    if (!history_fold_host(mean_in, S_in, n_in, map, x, w, h, max_frames, mean_out, S_out, n_out))
        return fail(RESTIR_ERR_INVALID, "restir_history_fold: a map entry names a pixel outside the %ux%u image", w, h);
    return RESTIR_OK;
}

restir_status restir_history_map_host(const restir_camera_frame* prev_cam, uint32_t w, uint32_t h, const float* cur_n_t,
                                      const float* cur_p_mat, const float* kept_n_t, const uint32_t* kept_material,
                                      const uint32_t* kept_n, uint32_t miss_material, uint32_t* map) {
    if (!prev_cam || !cur_n_t || !cur_p_mat || !map) return fail(RESTIR_ERR_INVALID, "restir_history_map_host: null argument");
    const int kept = (kept_n_t ? 1 : 0) + (kept_material ? 1 : 0) + (kept_n ? 1 : 0);
    if (kept != 0 && kept != 3)
        return fail(RESTIR_ERR_INVALID, "restir_history_map_host: kept_n_t, kept_material and kept_n are given together or not at all");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFF0ull - kHistReasons)
        return fail(RESTIR_ERR_INVALID, "restir_history_map_host: image %ux%u", w, h);
    ReprojCam cam{};
    cam.qx = prev_cam->quat[0]; cam.qy = prev_cam->quat[1]; cam.qz = prev_cam->quat[2]; cam.qw = prev_cam->quat[3];
    cam.ox = prev_cam->origin[0]; cam.oy = prev_cam->origin[1]; cam.oz = prev_cam->origin[2];
    cam.half_w = prev_cam->half_w; cam.half_h = prev_cam->half_h;
    cam.W = w; cam.H = h;
    history_map_host(cam, cur_n_t, cur_p_mat, kept_n_t, kept_material, kept_n, miss_material, map);
    return RESTIR_OK;
}

restir_status restir_history_advance_host(const restir_camera_frame* prev_cam, uint32_t w, uint32_t h, const float* cur_n_t,
                                          const float* cur_p_mat, const float* kept_n_t, const uint32_t* kept_material,
                                          const float* mean_in, const float* S_in, const uint32_t* n_in, const float* x,
                                          uint32_t miss_material, uint32_t max_frames, uint32_t gather, float* mean_out,
                                          float* S_out, uint32_t* n_out, uint32_t* out_map) {
    if (!prev_cam || !cur_n_t || !cur_p_mat || !mean_in || !S_in || !n_in || !x || !mean_out || !S_out || !n_out)
        return fail(RESTIR_ERR_INVALID, "restir_history_advance_host: null argument");
    if ((kept_n_t == nullptr) != (kept_material == nullptr))
        return fail(RESTIR_ERR_INVALID, "restir_history_advance_host: kept_n_t and kept_material are given together or not at all");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFF0ull - kHistReasons)
        return fail(RESTIR_ERR_INVALID, "restir_history_advance_host: image %ux%u", w, h);
    if (max_frames < 1u || max_frames > kHistMaxFrames)
        return fail(RESTIR_ERR_INVALID, "restir_history_advance_host: max_frames %u outside 1..%u", max_frames, kHistMaxFrames);
    if (gather > RESTIR_HISTORY_GATHER_BILINEAR) return fail(RESTIR_ERR_INVALID, "restir_history_advance_host: gather %u (0 or 1)", gather);
    if (gather == RESTIR_HISTORY_GATHER_BILINEAR && kept_n_t) {   // (float)n must be exact for the blended count
        const size_t npx = (size_t)w * h;
        for (size_t i = 0; i < npx; i++)
            if (n_in[i] > kHistMaxFrames)
                return fail(RESTIR_ERR_INVALID, "restir_history_advance_host: n_in[%zu] = %u above %u", i, n_in[i], kHistMaxFrames);
    }
    ReprojCam cam{};
    cam.qx = prev_cam->quat[0]; cam.qy = prev_cam->quat[1]; cam.qz = prev_cam->quat[2]; cam.qw = prev_cam->quat[3];
    cam.ox = prev_cam->origin[0]; cam.oy = prev_cam->origin[1]; cam.oz = prev_cam->origin[2];
    cam.half_w = prev_cam->half_w; cam.half_h = prev_cam->half_h;
    cam.W = w; cam.H = h;
    history_advance_host(cam, cur_n_t, cur_p_mat, kept_n_t, kept_material, mean_in, S_in, n_in, x, miss_material, max_frames, gather,
                         mean_out, S_out, n_out, out_map);
    return RESTIR_OK;
}

restir_status restir_history_variance_host(const float* mean, const float* S, const uint32_t* n, const float* n_t,
                                           const float* p_mat, uint32_t w, uint32_t h, uint32_t miss_material,
                                           const restir_history_params* params, const restir_denoise_params* geo, float* var) {
    if (!mean || !S || !n || !n_t || !p_mat || !var) return fail(RESTIR_ERR_INVALID, "restir_history_variance_host: null argument");
    if (w == 0 || h == 0) return fail(RESTIR_ERR_INVALID, "restir_history_variance_host: empty image %ux%u", w, h);
    ST_TRY(history_params_check(params, "restir_history_variance_host"));
    ST_TRY(denoise_params_check(geo, "restir_history_variance_host"));
    const size_t npx = (size_t)w * h;
    try {
        std::vector<DenoiseGuide> guides(npx);
        std::vector<float> tvals(npx);
        history_variance_host(mean, S, n, n_t, p_mat, w, h, miss_material, params->spatial_below, geo->normal_power_log2,
                              geo->sigma_plane, var, guides.data(), tvals.data());
    } catch (const std::bad_alloc&) {
        return fail(RESTIR_ERR_INVALID, "restir_history_variance_host: no memory for a %ux%u image", w, h);
    }
    return RESTIR_OK;
}

}  // extern "C"
