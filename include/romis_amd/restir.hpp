// restir.hpp -- header-only C++ wrapper over the C ABI (include/restir_c.h) that keeps the reference's
// render surface:
//
//   reference  ReservoirGrid renderReSTIR(std::shared_ptr<ReservoirGrid> previousFrameGrid, const Scene&,
//                                         const Trackball&, const EmbreeInterface&, Screen&, const Features&)
//              (src/rendering/render.h:25-28, render.cpp:28-62)
//   here       std::shared_ptr<ReservoirGrid> romis::renderReSTIR(Renderer&, std::shared_ptr<ReservoirGrid> prev,
//                                         const Camera&, Screen&, const Features&)
//
// Errors throw romis::RestirError (a std::runtime_error, as render.cpp:99/278 do).  The grid stays on the GPU
// (a reference-counted device handle, the replacement for the caller's std::shared_ptr<ReservoirGrid>).
// The Scene / EmbreeInterface pair becomes Renderer::setScene (uploads materials, lights and the BVH once).
#pragma once

#include <ctime>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../restir_c.h"

namespace romis {

struct RestirError : std::runtime_error {
    explicit RestirError(const std::string& what) : std::runtime_error(what) {}
};

inline void check(restir_status s, const char* what) {
    if (s != RESTIR_OK) throw RestirError(std::string(what) + ": " + restir_last_error());
}

// struct Features (src/utils/common.h:89-136): the fields the ReSTIR path reads.
struct Features : restir_features {
    Features() { restir_features_default(this); }
};

// restir_denoise_params with its defaults (2 levels, normal exponent 2^5, plane support 0.01 t)
struct DenoiseParams : restir_denoise_params {
    DenoiseParams() { restir_denoise_params_default(this); }
};

// restir_denoise_lum_params with its defaults (DenoiseParams', the spatial variance estimate, sigma_lum 4)
struct DenoiseLumParams : restir_denoise_lum_params {
    DenoiseLumParams() { restir_denoise_lum_params_default(this); }
};

// restir_history_params with its defaults (a cap of 8 samples, the spatial variance estimate below 4)
struct HistoryParams : restir_history_params {
    HistoryParams() { restir_history_params_default(this); }
};

// restir_history_gather: the nearest source pixel, or the 2 x 2 records around the continuous source position
enum class HistoryGather : uint32_t { Nearest = RESTIR_HISTORY_GATHER_NEAREST, Bilinear = RESTIR_HISTORY_GATHER_BILINEAR };

// The reference's own struct Features (src/utils/common.h:89-136) -> Features, field by field by the reference's
// member names (any type with those members works, so the reference's header is not needed here).  The enums
// keep their values: RayTraceMode {ReSTIR, RMIS, ROMIS} (common.h:25-29) = restir_mode,
// NeighbourSelectionStrategy (common.h:36-41) = restir_neighbour_strategy, MISWeightRMIS (common.h:31-34) =
// restir_mis_weight.  Fields off the path (enableRecursive, enableHardShadow, maxReflectionRecursion, ...) are
// not read by renderReSTIR / renderRMIS / renderROMIS and have no counterpart.
template <class RefFeatures>
Features fromReferenceFeatures(const RefFeatures& rf) {
    Features f;
    f.ray_trace_mode = static_cast<uint32_t>(rf.rayTraceMode);
    f.initial_light_samples = rf.initialLightSamples;
    f.num_samples_in_reservoir = rf.numSamplesInReservoir;
    f.num_neighbours_to_sample = rf.numNeighboursToSample;
    f.spatial_resample_radius = rf.spatialResampleRadius;
    f.spatial_resampling_passes = rf.spatialResamplingPasses;
    f.temporal_clamp_m = rf.temporalClampM;
    f.initial_samples_visibility_check = rf.initialSamplesVisibilityCheck ? 1 : 0;
    f.unbiased_combination = rf.unbiasedCombination ? 1 : 0;
    f.spatial_reuse = rf.spatialReuse ? 1 : 0;
    f.spatial_reuse_visibility_check = rf.spatialReuseVisibilityCheck ? 1 : 0;
    f.temporal_reuse = rf.temporalReuse ? 1 : 0;
    f.enable_shading = rf.enableShading ? 1 : 0;
    f.enable_texture_mapping = rf.enableTextureMapping ? 1 : 0;
    f.enable_tone_mapping = rf.enableToneMapping ? 1 : 0;
    f.gamma = rf.gamma;
    f.exposure = rf.exposure;
    f.neighbour_same_geometry = rf.neighbourSameGeometry ? 1 : 0;
    f.use_progressive_romis = rf.useProgressiveROMIS ? 1 : 0;
    f.save_alphas_visualisation = rf.saveAlphasVisualisation ? 1 : 0;
    f.neighbour_max_depth_difference_fraction = rf.neighbourMaxDepthDifferenceFraction;
    f.neighbour_max_normal_angle_difference_radians = rf.neighbourMaxNormalAngleDifferenceRadians;
    f.max_iterations_mis = rf.maxIterationsMIS;
    f.neighbour_selection_strategy = static_cast<uint32_t>(rf.neighbourSelectionStrategy);
    f.mis_weight_rmis = static_cast<uint32_t>(rf.misWeightRMIS);
    f.progressive_update_mod = rf.progressiveUpdateMod;
    return f;
}

// Trackball state after Trackball(window, glm::radians(fov), dist) + setCamera(lookAt, glm::radians(rot), dist)
struct Camera : restir_camera {
    Camera() : restir_camera{} {}
    static Camera fromDegrees(float fovDeg, float aspect, const float lookAt[3], float dist, const float rotDeg[3]) {
        constexpr float rad = 0.01745329251994329576923690768489f;   // glm::radians
        Camera c;
        c.fovy = fovDeg * rad;
        c.aspect = aspect;
        for (int i = 0; i < 3; i++) { c.look_at[i] = lookAt[i]; c.rotation[i] = rotDeg[i] * rad; }
        c.distance = dist;
        return c;
    }
};

// One mesh of the Scene (framework/include/framework/mesh.h:36-43) as flat arrays.
struct Mesh {
    std::vector<float> positions;    // 3 per vertex
    std::vector<float> normals;      // 3 per vertex
    std::vector<uint32_t> triangles; // 3 per triangle
    restir_material material{};
};

struct Scene {
    std::vector<Mesh> meshes;
    std::vector<restir_light> lights;   // Point / Segment / Parallelogram (common.h:72-87)
};

// Screen (src/rendering/screen.h): float RGB, row 0 = top, as Screen::setPixel stores it (screen.cpp:37-43).
struct Screen {
    int width = 0, height = 0;
    std::vector<float> rgb;
    Screen(int w, int h) : width(w), height(h), rgb(size_t(w) * size_t(h) * 3, 0.0f) {}
    float* pixel(int x, int yFromTop) { return &rgb[(size_t(yFromTop) * width + x) * 3]; }
    // Screen::writeBitmapToFile (screen.cpp:45-56): clamp, x255, truncate, stbi_write_bmp byte for byte
    void writeBitmapToFile(const std::filesystem::path& filePath) const {
        check(restir_write_bmp(filePath.string().c_str(), rgb.data(), uint32_t(width), uint32_t(height)),
              "restir_write_bmp");
    }
};

// The configuration record renderRayTraced saves per render (render.cpp:281-287): <dir>/<currentTime()>.json,
// currentTime() = "%d-%m-%Y %H-%M-%S" local time (utils.cpp:16-22), cereal's bytes (restir_features_json).
inline std::filesystem::path saveFeaturesRecord(const restir_features& features, const std::filesystem::path& dir,
                                                const restir_features_record_extra* extra = nullptr) {
    size_t n = 0;
    check(restir_features_json(&features, extra, nullptr, 0, &n), "restir_features_json");
    std::string json(n + 1, '\0');
    check(restir_features_json(&features, extra, json.data(), json.size(), &n), "restir_features_json");
    json.resize(n);
    if (!std::filesystem::exists(dir)) std::filesystem::create_directory(dir);
    const std::time_t t = std::time(nullptr);
    std::ostringstream name;
    name << std::put_time(std::localtime(&t), "%d-%m-%Y %H-%M-%S") << ".json";
    const std::filesystem::path path = dir / name.str();
    std::ofstream out(path, std::ios::binary);
    out << json;
    if (!out) throw RestirError("saveFeaturesRecord: cannot write " + path.string());
    return path;
}

// One sub-reservoir's state as reservoir.h:18-32 keeps it: outputSamples[j] = {position, color, W},
// sampleNums[j] = M.
struct ReservoirSample {
    float position[3], color[3], W;
    uint32_t M;
};

// Device-resident ReservoirGrid (reservoir.h:75).
class ReservoirGrid {
public:
    explicit ReservoirGrid(restir_frame* f) : frame_(f) {}
    ~ReservoirGrid() { restir_frame_release(frame_); }
    ReservoirGrid(const ReservoirGrid&) = delete;
    ReservoirGrid& operator=(const ReservoirGrid&) = delete;
    restir_frame* handle() const { return frame_; }
    // host copy, [N][vh][vw] (rows y = 0 bottom): the per-pixel state renderReSTIR returns (render.cpp:61)
    std::vector<ReservoirSample> download(uint32_t* n = nullptr, uint32_t* vw = nullptr, uint32_t* vh = nullptr) const {
        uint32_t N = 0, w = 0, h = 0;
        check(restir_frame_info(frame_, nullptr, nullptr, nullptr, nullptr, &w, &h, &N), "restir_frame_info");
        const size_t cnt = size_t(N) * w * h;
        std::vector<float> pos(3 * cnt), col(3 * cnt), W(cnt);
        std::vector<uint32_t> M(cnt);
        check(restir_frame_download(frame_, pos.data(), col.data(), W.data(), M.data()), "restir_frame_download");
        std::vector<ReservoirSample> out(cnt);
        for (size_t i = 0; i < cnt; i++) {
            for (int a = 0; a < 3; a++) { out[i].position[a] = pos[3 * i + a]; out[i].color[a] = col[3 * i + a]; }
            out[i].W = W[i];
            out[i].M = M[i];
        }
        if (n) *n = N;
        if (vw) *vw = w;
        if (vh) *vh = h;
        return out;
    }

private:
    restir_frame* frame_;
};

// A snapshot of a Renderer's last image on its way to pinned host memory (restir_image_begin): the next frame may be
// enqueued at once.  Released by the destructor; must not outlive its Renderer (restir_destroy frees the slots).
class PresentedImage {
public:
    explicit PresentedImage(restir_image* image) : image_(image) {
        check(restir_image_info(image_, &width_, &height_, &format_, &bytes_), "restir_image_info");
    }
    ~PresentedImage() { restir_image_release(image_); }
    PresentedImage(PresentedImage&& o) noexcept
        : image_(o.image_), width_(o.width_), height_(o.height_), format_(o.format_), bytes_(o.bytes_) { o.image_ = nullptr; }
    PresentedImage(const PresentedImage&) = delete;
    PresentedImage& operator=(const PresentedImage&) = delete;
    PresentedImage& operator=(PresentedImage&&) = delete;
    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    restir_image_format format() const { return restir_image_format(format_); }
    size_t bytes() const { return bytes_; }
    bool ready() const {   // never blocks
        int r = 0;
        check(restir_image_ready(image_, &r), "restir_image_ready");
        return r != 0;
    }
    // blocks on this snapshot's copy only; bytes() bytes of pinned memory, valid while this object lives
    const void* wait() const {
        const void* p = nullptr;
        check(restir_image_wait(image_, &p), "restir_image_wait");
        return p;
    }
    // a BGRA8_BOTTOM_UP snapshot as the BMP file Screen::writeBitmapToFile writes: the header + the bytes
    void writeBitmapToFile(const std::filesystem::path& filePath) const {
        if (format_ != RESTIR_IMAGE_BGRA8_BOTTOM_UP) throw RestirError("writeBitmapToFile: the snapshot is not BGRA8_BOTTOM_UP");
        const void* body = wait();
        size_t n = 0;
        check(restir_bmp_header(width_, height_, nullptr, 0, &n), "restir_bmp_header");
        std::vector<uint8_t> header(n);
        check(restir_bmp_header(width_, height_, header.data(), n, &n), "restir_bmp_header");
        std::ofstream out(filePath, std::ios::binary);
        out.write(reinterpret_cast<const char*>(header.data()), std::streamsize(n));
        out.write(static_cast<const char*>(body), std::streamsize(bytes_));
        if (!out) throw RestirError("writeBitmapToFile: cannot write " + filePath.string());
    }

private:
    restir_image* image_;
    uint32_t width_ = 0, height_ = 0, format_ = 0;
    size_t bytes_ = 0;
};

// Owns a HIP device context: the EmbreeInterface + OpenMP loops of the reference become this object.
class Renderer {
public:
    explicit Renderer(int device = 0) { check(restir_create(device, &ctx_), "restir_create"); }
    ~Renderer() { restir_destroy(ctx_); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    void setScene(const Scene& scene) {
        std::vector<restir_mesh> m(scene.meshes.size());
        for (size_t i = 0; i < m.size(); i++) {
            const Mesh& src = scene.meshes[i];
            m[i].positions = src.positions.data();
            m[i].normals = src.normals.data();
            m[i].num_vertices = uint32_t(src.positions.size() / 3);
            m[i].triangles = src.triangles.data();
            m[i].num_triangles = uint32_t(src.triangles.size() / 3);
            m[i].material = src.material;
        }
        check(restir_set_scene(ctx_, m.data(), uint32_t(m.size()), scene.lights.data(), uint32_t(scene.lights.size())),
              "restir_set_scene");
    }
    // New vertex positions (normals too when meshes[i].normals is not empty) for meshes of the scene set: mesh index ->
    // a Mesh whose positions have the uploaded count; its triangles and material are not read (restir_update_meshes)
    void updateMeshes(const std::vector<std::pair<uint32_t, const Mesh*>>& meshes) {
        std::vector<restir_mesh_update> u(meshes.size());
        for (size_t i = 0; i < u.size(); i++) {
            const Mesh& src = *meshes[i].second;
            u[i].mesh = meshes[i].first;
            u[i].num_vertices = uint32_t(src.positions.size() / 3);
            u[i].positions = src.positions.data();
            u[i].normals = src.normals.size() == src.positions.size() && !src.normals.empty() ? src.normals.data() : nullptr;
        }
        check(restir_update_meshes(ctx_, u.data(), uint32_t(u.size())), "restir_update_meshes");
    }
    // Another light list over the same geometry (restir_set_lights)
    void setLights(const std::vector<restir_light>& lights) {
        check(restir_set_lights(ctx_, lights.data(), uint32_t(lights.size())), "restir_set_lights");
    }
    void setSeed(uint32_t seed, uint32_t frameIndex = 0) { check(restir_set_seed(ctx_, seed, frameIndex), "restir_set_seed"); }
    // RENDERS_DIR for the file side outputs the library writes itself (R-OMIS alpha visualisation); empty = none
    void setRendersDir(const std::filesystem::path& dir) {
        check(restir_set_renders_dir(ctx_, dir.empty() ? nullptr : dir.c_str()), "restir_set_renders_dir");
        rendersDir_ = dir;
    }
    const std::filesystem::path& rendersDir() const { return rendersDir_; }
    // renderRMIS / renderROMIS of one screen tile of a width x height image (restir_render_mis_tile; the tile's ghost
    // zone = the resample radius, restir_tile_plan / restir_layout_tile): the owned rectangle, tile.width x tile.height
    // x 3 floats, row 0 = its top -- bit for bit the whole image's pixels
    std::vector<float> renderMISTile(const Camera& camera, const Features& features, uint32_t width, uint32_t height,
                                     const restir_tile& tile) {
        std::vector<float> rgb(size_t(tile.width) * tile.height * 3);
        check(restir_render_mis_tile(ctx_, &camera, &features, width, height, &tile, rgb.data()), "restir_render_mis_tile");
        return rgb;
    }
    // Frames so far whose fused last pass traced its shadow rays over the view's triangle lists (restir_shadow_list_frames)
    uint64_t shadowListFrames() const {
        uint64_t n = 0;
        check(restir_shadow_list_frames(ctx_, &n), "restir_shadow_list_frames");
        return n;
    }
    // Test hook (restir_debug_shadow_lists): width x height bytes each, the last frame's owned rectangle (another size
    // is refused)
    void debugShadowLists(uint32_t light, std::vector<uint8_t>& byBvh, std::vector<uint8_t>& byList, uint32_t width,
                          uint32_t height) const {
        byBvh.assign(size_t(width) * height, 0);
        byList.assign(size_t(width) * height, 0);
        check(restir_debug_shadow_lists(ctx_, light, width, height, byBvh.data(), byList.data()), "restir_debug_shadow_lists");
    }
    // Frames so far whose last pass read its shadow rays' answers from the view's visibility bits, and the builds of
    // those bits (restir_shadow_vis_frames, restir_shadow_vis_builds)
    uint64_t shadowVisFrames() const {
        uint64_t n = 0;
        check(restir_shadow_vis_frames(ctx_, &n), "restir_shadow_vis_frames");
        return n;
    }
    uint64_t shadowVisBuilds() const {
        uint64_t n = 0;
        check(restir_shadow_vis_builds(ctx_, &n), "restir_shadow_vis_builds");
        return n;
    }
    // Test hook (restir_debug_shadow_vis): width x height bytes, the last frame's owned rectangle (another size is refused)
    void debugShadowVis(uint32_t light, std::vector<uint8_t>& bits, uint32_t width, uint32_t height) const {
        bits.assign(size_t(width) * height, 0);
        check(restir_debug_shadow_vis(ctx_, light, width, height, bits.data()), "restir_debug_shadow_vis");
    }
    // Frames so far whose RIS read its candidates' target pdfs from the view's p-hat table, and the builds of that
    // table (restir_phat_frames, restir_phat_builds)
    uint64_t phatFrames() const {
        uint64_t n = 0;
        check(restir_phat_frames(ctx_, &n), "restir_phat_frames");
        return n;
    }
    uint64_t phatBuilds() const {
        uint64_t n = 0;
        check(restir_phat_builds(ctx_, &n), "restir_phat_builds");
        return n;
    }
    // Frames so far that took their RIS result from the look-ahead the frame before launched, and the results no frame
    // took (restir_ahead_frames, restir_ahead_discards)
    uint64_t aheadFrames() const {
        uint64_t n = 0;
        check(restir_ahead_frames(ctx_, &n), "restir_ahead_frames");
        return n;
    }
    uint64_t aheadDiscards() const {
        uint64_t n = 0;
        check(restir_ahead_discards(ctx_, &n), "restir_ahead_discards");
        return n;
    }
    // Test hook (restir_debug_phat): width x height floats, the last frame's view (another size is refused)
    void debugPhat(uint32_t light, std::vector<float>& phat, uint32_t width, uint32_t height) const {
        phat.assign(size_t(width) * height, 0.0f);
        check(restir_debug_phat(ctx_, light, width, height, phat.data()), "restir_debug_phat");
    }
    // A snapshot of the last image (restir_image_begin): converted on the device, copied to pinned memory behind the
    // frame that produced it; returns without synchronising, so the next frame may be rendered at once
    PresentedImage present(restir_image_format format = RESTIR_IMAGE_RGBA8) {
        restir_image* im = nullptr;
        check(restir_image_begin(ctx_, uint32_t(format), &im), "restir_image_begin");
        return PresentedImage(im);
    }
    // The last image as restir_rgb_to_rgba8's bytes, converted on the device: a snapshot, waited for and copied
    std::vector<uint8_t> downloadRgba8() {
        PresentedImage im = present(RESTIR_IMAGE_RGBA8);
        const uint8_t* p = static_cast<const uint8_t*>(im.wait());
        return std::vector<uint8_t>(p, p + im.bytes());
    }
    // Screen::writeBitmapToFile (screen.cpp:45-56) of the last image, without the floats leaving the device
    void writeBitmapToFile(const std::filesystem::path& filePath) {
        check(restir_write_image_bmp(ctx_, filePath.string().c_str()), "restir_write_image_bmp");
    }
    // Accumulating frames on the device (restir_accum_*): begin an empty state -- a running mean per float of the image
    // and, with `variance`, the squared deviations the stats need --, add the last image after each render (render with
    // enable_tone_mapping = 0), resolve the mean as the last image (tone mapped by `tone`'s enable_tone_mapping / gamma /
    // exposure; nullptr: its own bits), which present / downloadRgba8 / writeBitmapToFile then serve
    void accumBegin(bool variance = true) { check(restir_accum_begin(ctx_, variance ? RESTIR_ACCUM_VARIANCE : 0u), "restir_accum_begin"); }
    void accumAdd() { check(restir_accum_add(ctx_), "restir_accum_add"); }
    void accumResolve(const Features* tone = nullptr) { check(restir_accum_resolve(ctx_, tone), "restir_accum_resolve"); }
    // needs the variance and two frames; synchronises
    restir_accum_stats accumStats() {
        restir_accum_stats s{};
        check(restir_accum_stats_get(ctx_, &s), "restir_accum_stats_get");
        return s;
    }
    // Test hook (restir_accum_download): the state as it stands, width x height x 3 floats each
    void accumState(std::vector<float>& mean, std::vector<float>& m2, uint32_t width, uint32_t height) {
        mean.assign(size_t(width) * height * 3, 0.0f);
        m2.assign(size_t(width) * height * 3, 0.0f);
        check(restir_accum_download(ctx_, mean.data(), m2.data(), mean.size()), "restir_accum_download");
    }
    void accumEnd() { check(restir_accum_end(ctx_), "restir_accum_end"); }
    // The exact direct-lighting image of a point-light scene (restir_render_exact) as the last image: per pixel the
    // float32 sum over every light, in table order, of computeShading times visibility, tone mapped by `features`.  A
    // producer like a frame; rgb (nullable): width x height x 3 floats, row 0 = top; nullptr only enqueues
    void renderExact(const Camera& camera, const Features& features, uint32_t width, uint32_t height, float* rgb = nullptr) {
        check(restir_render_exact(ctx_, &camera, &features, width, height, nullptr, rgb), "restir_render_exact");
    }
    // Keep a device copy of the last image as the reference (a snapshot; referenceClear frees it), and the error figures
    // of the last image (RESTIR_ERROR_SRC_IMAGE) or the open accumulation's mean (RESTIR_ERROR_SRC_ACCUM_MEAN) against
    // it, reduced on the device; error() synchronises
    void referenceSet() { check(restir_reference_set(ctx_), "restir_reference_set"); }
    void referenceClear() { check(restir_reference_clear(ctx_), "restir_reference_clear"); }
    restir_error_stats error(uint32_t source = RESTIR_ERROR_SRC_IMAGE) {
        restir_error_stats s{};
        check(restir_error_get(ctx_, source, &s), "restir_error_get");
        return s;
    }
    // The edge-avoiding a-trous filter over the last image, in place (restir_denoise): guided by the normal, position and
    // material of camera's G-buffer, traced once per view and kept.  tone (nullable): its tone-mapping fields are applied
    // after the last level -- render with enable_tone_mapping = 0, denoise with the tone fields, present.  The result is
    // marked like a resolve.  rgb (nullable): width x height x 3 floats, row 0 = top; nullptr only enqueues
    void denoise(const Camera& camera, uint32_t width, uint32_t height, const DenoiseParams& params = DenoiseParams(),
                 const Features* tone = nullptr, float* rgb = nullptr) {
        check(restir_denoise(ctx_, &camera, width, height, nullptr, &params, tone, rgb), "restir_denoise");
    }
    // denoise with a variance-guided luminance term (restir_denoise_lum).  With params.variance_source =
    // RESTIR_DENOISE_VAR_ACCUM the image is the open accumulation's mean (two frames at least, with the variance) and the
    // variance its m2's; otherwise the last image, with a variance estimated from it
    void denoiseLum(const Camera& camera, uint32_t width, uint32_t height, const DenoiseLumParams& params = DenoiseLumParams(),
                    const Features* tone = nullptr, float* rgb = nullptr) {
        check(restir_denoise_lum(ctx_, &camera, width, height, nullptr, &params, tone, rgb), "restir_denoise_lum");
    }
    uint64_t denoiseGuideBuilds() const {
        uint64_t n = 0;
        check(restir_denoise_guide_builds(ctx_, &n), "restir_denoise_guide_builds");
        return n;
    }
    // a reprojected image history (restir_history_*): a per-pixel mean, variance and sample count that follow the camera.
    // The viewer loop, tone mapping off until the last step: render, historyAdvance(camera the frame was rendered with),
    // historyDenoise(params, &tone), present
    void historyBegin(const HistoryParams& params = HistoryParams()) { check(restir_history_begin(ctx_, &params), "restir_history_begin"); }
    // only enqueues; with map (width x height words, rows y = 0 bottom: the source pixel's flat index or 0xFFFFFFFF - reason)
    // it synchronises
    void historyAdvance(const Camera& camera, uint32_t width, uint32_t height, uint32_t* map = nullptr) {
        check(restir_history_advance(ctx_, &camera, width, height, map), "restir_history_advance");
    }
    // how historyAdvance gathers the kept state (restir_history_gather_set): context state, Nearest by default, kept across
    // historyBegin / historyEnd and resets
    void historyGather(HistoryGather mode) { check(restir_history_gather_set(ctx_, static_cast<uint32_t>(mode)), "restir_history_gather_set"); }
    HistoryGather historyGather() const {
        uint32_t g = 0;
        check(restir_history_gather_get(ctx_, &g), "restir_history_gather_get");
        return static_cast<HistoryGather>(g);
    }
    void historyResolve(const Features* tone = nullptr) { check(restir_history_resolve(ctx_, tone), "restir_history_resolve"); }
    void historyDenoise(const DenoiseLumParams& params = DenoiseLumParams(), const Features* tone = nullptr, float* rgb = nullptr) {
        check(restir_history_denoise(ctx_, &params, tone, rgb), "restir_history_denoise");
    }
    // Test hook (restir_history_download): mean and S width x height x 3 floats, n width x height words, image rows
    void historyState(std::vector<float>& mean, std::vector<float>& S, std::vector<uint32_t>& n, uint32_t width, uint32_t height) {
        const size_t px = size_t(width) * height;
        mean.assign(px * 3, 0.0f);
        S.assign(px * 3, 0.0f);
        n.assign(px, 0u);
        check(restir_history_download(ctx_, mean.data(), S.data(), n.data(), px), "restir_history_download");
    }
    // (advances, resets) since historyBegin
    std::pair<uint64_t, uint64_t> historyFrames() const {
        uint64_t a = 0, r = 0;
        check(restir_history_frames(ctx_, &a, &r), "restir_history_frames");
        return {a, r};
    }
    void historyEnd() { check(restir_history_end(ctx_), "restir_history_end"); }
    restir_ctx* handle() const { return ctx_; }

private:
    restir_ctx* ctx_ = nullptr;
    std::filesystem::path rendersDir_;
};

// Contexts for callers that render concurrently: the reference's CLI renders one std::thread per camera through
// renderRayTraced with a shared Scene and EmbreeInterface (main.cpp:213-230).  Each calling thread gets its own
// Renderer -- its own HIP stream, buffers and scene upload -- created on first use, so the threads never
// serialise on one context's mutex, and each camera keeps its own previous-frame grid (the caller's
// std::shared_ptr<ReservoirGrid>, as in the reference).  Thread-safe.
class RendererPool {
public:
    RendererPool(int device, Scene scene, uint32_t seed = RESTIR_DEFAULT_SEED)
        : device_(device), scene_(std::move(scene)), seed_(seed) {}
    RendererPool(const RendererPool&) = delete;
    RendererPool& operator=(const RendererPool&) = delete;
    // this thread's renderer (frame index 0 at creation, advancing by one per render)
    Renderer& local() {
        std::lock_guard<std::mutex> lk(mu_);
        std::unique_ptr<Renderer>& r = per_thread_[std::this_thread::get_id()];
        if (!r) {
            r = std::make_unique<Renderer>(device_);
            r->setScene(scene_);
            r->setSeed(seed_, 0);
        }
        return *r;
    }

private:
    int device_;
    Scene scene_;
    uint32_t seed_;
    std::mutex mu_;
    std::map<std::thread::id, std::unique_ptr<Renderer>> per_thread_;
};

// renderReSTIR (render.cpp:28-62): primary hits, initial RIS, [temporal if prev], [spatial x passes], final
// shading + tone mapping into `screen`; returns the frame's final grid for the next frame's temporal reuse.
inline std::shared_ptr<ReservoirGrid> renderReSTIR(Renderer& r, const std::shared_ptr<ReservoirGrid>& prev,
                                                   const Camera& camera, Screen& screen, const Features& features) {
    restir_frame* next = nullptr;
    check(restir_render(r.handle(), &camera, &features, uint32_t(screen.width), uint32_t(screen.height), nullptr,
                        prev ? prev->handle() : nullptr, &next, screen.rgb.data()),
          "restir_render");
    return std::make_shared<ReservoirGrid>(next);
}

// restir_render_accumulate: up to `frames` frames of one view rendered without tone mapping and averaged on the device
// (with temporal_reuse each frame's grid is the next one's predecessor), the mean tone mapped by `features` into
// `screen`.  With targetMse > 0 the loop checks the stats after frame minFrames and then every checkEvery frames and
// stops once est_mse <= targetMse.  Returns the stats (zeros but for the size and the frame count with one frame or
// without `variance`); the Renderer's accumulation stays open.
inline restir_accum_stats renderAccumulated(Renderer& r, const Camera& camera, Screen& screen, const Features& features,
                                            uint32_t frames, double targetMse = 0.0, uint32_t minFrames = 0,
                                            uint32_t checkEvery = 8, bool variance = true) {
    restir_accum_request req{};
    req.flags = variance ? RESTIR_ACCUM_VARIANCE : 0u;
    req.min_frames = minFrames;
    req.max_frames = frames;
    req.check_every = checkEvery;
    req.target_mse = targetMse;
    restir_accum_stats stats{};
    check(restir_render_accumulate(r.handle(), &camera, &features, uint32_t(screen.width), uint32_t(screen.height), nullptr,
                                   &req, &stats, screen.rgb.data()),
          "restir_render_accumulate");
    return stats;
}

// restir_denoise_host: Renderer::denoise's arithmetic on the host, bit for bit, without the tone-mapping step.  rgb: w x h x
// 3 floats, row 0 = top; n_t, p_mat: w x h x 4 floats as restir_stage_primary gives them (row y = 0 at the bottom);
// missMaterial: the scene's material count (the miss material's index)
inline std::vector<float> denoiseHost(const std::vector<float>& rgb, const std::vector<float>& n_t, const std::vector<float>& p_mat,
                                      uint32_t w, uint32_t h, uint32_t missMaterial, const DenoiseParams& params = DenoiseParams()) {
    const size_t npx = size_t(w) * h;
    if (rgb.size() != 3 * npx || n_t.size() != 4 * npx || p_mat.size() != 4 * npx)
        throw std::runtime_error("denoiseHost: rgb, n_t and p_mat must hold 3, 4 and 4 floats per pixel");
    std::vector<float> out(3 * npx);
    check(restir_denoise_host(rgb.data(), n_t.data(), p_mat.data(), w, h, missMaterial, &params, out.data()), "restir_denoise_host");
    return out;
}

// restir_render_exact into `screen`: the exact image every estimator configuration here estimates (point lights only)
inline void renderExact(Renderer& r, const Camera& camera, Screen& screen, const Features& features) {
    r.renderExact(camera, features, uint32_t(screen.width), uint32_t(screen.height), screen.rgb.data());
}

// Motion-compensated temporal reuse (restir_frame_reproject): the predecessor grid `prev`, rendered from prevCamera,
// gathered to where `camera` sees its surface points -- pass the result to renderReSTIR as `prev` when the camera
// moved between the frames.  map (nullable): per pixel (rows y = 0 bottom) the source pixel's flat index or
// 0xFFFFFFFF - reason, which makes the call synchronise.
inline std::shared_ptr<ReservoirGrid> reprojectGrid(Renderer& r, const std::shared_ptr<ReservoirGrid>& prev,
                                                    const Camera& prevCamera, const Camera& camera,
                                                    std::vector<uint32_t>* map = nullptr) {
    if (!prev) return nullptr;
    if (map) {
        uint32_t w = 0, h = 0;
        check(restir_frame_info(prev->handle(), &w, &h, nullptr, nullptr, nullptr, nullptr, nullptr), "restir_frame_info");
        map->assign(size_t(w) * h, 0u);
    }
    restir_frame* out = nullptr;
    check(restir_frame_reproject(r.handle(), prev->handle(), &prevCamera, &camera, &out, map ? map->data() : nullptr),
          "restir_frame_reproject");
    return std::make_shared<ReservoirGrid>(out);
}

// renderRMIS / renderROMIS (render.cpp:64-265): maxIterationsMIS rounds of initial samples combined over each
// pixel's neighbourhood into `screen` (features.ray_trace_mode selects the estimator).
inline void renderMIS(Renderer& r, const Camera& camera, Screen& screen, const Features& features) {
    check(restir_render(r.handle(), &camera, &features, uint32_t(screen.width), uint32_t(screen.height), nullptr, nullptr,
                        nullptr, screen.rgb.data()),
          "restir_render");
}

// renderRayTraced (render.cpp:268-290): the grid for temporal reuse in ReSTIR mode, nullptr (std::nullopt) for
// R-MIS / R-OMIS.  Like the reference, every render then saves its configuration record to
// <rendersDir>/<currentTime()>.json (render.cpp:281-287, saveFeaturesRecord), and R-OMIS with
// saveAlphasVisualisation writes its alpha bitmaps to <rendersDir>/<currentTime()>/ after every iteration; the
// reference's RENDERS_DIR is a build-time constant, here the caller passes it.  A non-empty rendersDir applies to
// this render only (the Renderer's own setRendersDir is restored afterwards); an empty one writes no record and
// leaves the alpha bitmaps to whatever the Renderer was given with setRendersDir.
inline std::shared_ptr<ReservoirGrid> renderRayTraced(Renderer& r, const std::shared_ptr<ReservoirGrid>& prev,
                                                      const Camera& camera, Screen& screen, const Features& features,
                                                      const std::filesystem::path& rendersDir = {},
                                                      const restir_features_record_extra* extra = nullptr) {
    std::shared_ptr<ReservoirGrid> next;
    // R-OMIS's per-iteration alpha visualisation (render.cpp:227-229) goes to rendersDir for this call
    struct DirScope {
        Renderer& r;
        std::filesystem::path saved;
        bool set;
        DirScope(Renderer& rr, const std::filesystem::path& d) : r(rr), saved(rr.rendersDir()), set(!d.empty()) {
            if (set) r.setRendersDir(d);
        }
        ~DirScope() {
            if (!set) return;
            try { r.setRendersDir(saved); } catch (...) {}   // never throws from a destructor
        }
    } scope(r, rendersDir);
    switch (features.ray_trace_mode) {
        case RESTIR_MODE_RESTIR: next = renderReSTIR(r, prev, camera, screen, features); break;
        case RESTIR_MODE_RMIS:
        case RESTIR_MODE_ROMIS: renderMIS(r, camera, screen, features); break;
        default: throw RestirError("Unsupported ray-tracing render mode requested from entry point");
    }
    if (!rendersDir.empty()) saveFeaturesRecord(features, rendersDir, extra);
    return next;
}
// ... from any thread: the calling thread's context of the pool
inline std::shared_ptr<ReservoirGrid> renderRayTraced(RendererPool& pool, const std::shared_ptr<ReservoirGrid>& prev,
                                                      const Camera& camera, Screen& screen, const Features& features,
                                                      const std::filesystem::path& rendersDir = {},
                                                      const restir_features_record_extra* extra = nullptr) {
    return renderRayTraced(pool.local(), prev, camera, screen, features, rendersDir, extra);
}

}  // namespace romis
