// denoise_host.cpp -- restir_denoise_params_default and restir_denoise_host, restir_denoise_lum_params_default and
// restir_denoise_lum_host: the filters of restir_denoise and restir_denoise_lum on the host, the same text (denoise.h)
// compiled without contraction.  No HIP header and no HIP call: a stand-alone program links this
// unit and abi_error.cpp alone (tests/cpp/denoise_host_check.cpp).
#include "abi_error.h"
#include "denoise.h"

#include <cmath>
#include <new>
#include <vector>

using namespace romis;

namespace romis {

// the parameter checks restir_denoise and restir_denoise_host share
restir_status denoise_params_check(const restir_denoise_params* p, const char* who) {
    if (!p) return fail(RESTIR_ERR_INVALID, "%s: params is NULL", who);
    if (p->iterations < 1u || p->iterations > kDenoiseMaxIterations)
        return fail(RESTIR_ERR_INVALID, "%s: iterations %u outside 1..%u", who, p->iterations, kDenoiseMaxIterations);
    if (p->normal_power_log2 > kDenoiseMaxNormalPower)
        return fail(RESTIR_ERR_INVALID, "%s: normal_power_log2 %u above %u", who, p->normal_power_log2, kDenoiseMaxNormalPower);
    if (!std::isfinite(p->sigma_plane) || !(p->sigma_plane > 0.0f))
        return fail(RESTIR_ERR_INVALID, "%s: sigma_plane must be finite and > 0", who);
    if (p->flags != 0u) return fail(RESTIR_ERR_INVALID, "%s: flags %u (none is defined)", who, p->flags);
    return RESTIR_OK;
}

// ... restir_denoise_lum and restir_denoise_lum_host share
restir_status denoise_lum_params_check(const restir_denoise_lum_params* p, const char* who) {
    if (!p) return fail(RESTIR_ERR_INVALID, "%s: params is NULL", who);
    ST_TRY(denoise_params_check(&p->geo, who));
    if (p->variance_source != RESTIR_DENOISE_VAR_SPATIAL && p->variance_source != RESTIR_DENOISE_VAR_ACCUM)
        return fail(RESTIR_ERR_INVALID, "%s: unknown variance_source %u", who, p->variance_source);
    if (!std::isfinite(p->sigma_lum) || !(p->sigma_lum > 0.0f))
        return fail(RESTIR_ERR_INVALID, "%s: sigma_lum must be finite and > 0", who);
    if (p->flags != 0u) return fail(RESTIR_ERR_INVALID, "%s: flags %u (none is defined)", who, p->flags);
    return RESTIR_OK;
}

}  // namespace romis

extern "C" {

void restir_denoise_params_default(restir_denoise_params* out) {
    if (!out) return;
    out->iterations = 2;
    out->normal_power_log2 = 5;
    out->sigma_plane = 0.01f;
    out->flags = 0;
}

restir_status restir_denoise_host(const float* rgb, const float* n_t, const float* p_mat, uint32_t w, uint32_t h,
                                  uint32_t miss_material, const restir_denoise_params* params, float* out) {
    if (!rgb || !n_t || !p_mat || !out) return fail(RESTIR_ERR_INVALID, "restir_denoise_host: null argument");
    if (w == 0 || h == 0) return fail(RESTIR_ERR_INVALID, "restir_denoise_host: empty image %ux%u", w, h);
    ST_TRY(denoise_params_check(params, "restir_denoise_host"));
    const size_t npx = (size_t)w * h;
    try {
        std::vector<DenoiseGuide> guides(npx);
        std::vector<float> tvals(npx), tmp(params->iterations > 1u ? 6 * npx : 0);
        denoise_host(rgb, n_t, p_mat, w, h, miss_material, params->iterations, params->normal_power_log2, params->sigma_plane,
                     out, guides.data(), tvals.data(), tmp.data());
    } catch (const std::bad_alloc&) {
        return fail(RESTIR_ERR_INVALID, "restir_denoise_host: no memory for a %ux%u image", w, h);
    }
    return RESTIR_OK;
}

void restir_denoise_lum_params_default(restir_denoise_lum_params* out) {
    if (!out) return;
    restir_denoise_params_default(&out->geo);
    out->variance_source = RESTIR_DENOISE_VAR_SPATIAL;
    out->sigma_lum = 4.0f;
    out->flags = 0;
}

restir_status restir_denoise_lum_host(const float* rgb, const float* var, const float* n_t, const float* p_mat, uint32_t w,
                                      uint32_t h, uint32_t miss_material, const restir_denoise_lum_params* params, float* out_rgb,
                                      float* out_var) {
    if (!rgb || !n_t || !p_mat || !out_rgb) return fail(RESTIR_ERR_INVALID, "restir_denoise_lum_host: null argument");
    if (w == 0 || h == 0) return fail(RESTIR_ERR_INVALID, "restir_denoise_lum_host: empty image %ux%u", w, h);
    ST_TRY(denoise_lum_params_check(params, "restir_denoise_lum_host"));
    const size_t npx = (size_t)w * h;
    try {
        std::vector<DenoiseGuide> guides(npx);
        std::vector<float> tvals(npx), tmp(params->geo.iterations > 1u ? 6 * npx : 0), vtmp(2 * npx);
        denoise_lum_host(rgb, var, n_t, p_mat, w, h, miss_material, params->geo.iterations, params->geo.normal_power_log2,
                         params->geo.sigma_plane, params->sigma_lum, out_rgb, out_var, guides.data(), tvals.data(), tmp.data(),
                         vtmp.data());
    } catch (const std::bad_alloc&) {
        return fail(RESTIR_ERR_INVALID, "restir_denoise_lum_host: no memory for a %ux%u image", w, h);
    }
    return RESTIR_OK;
}

}  // extern "C"
