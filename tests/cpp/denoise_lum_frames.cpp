// "Render a few frames, filter the mean by its own measured noise" through the C++ wrapper: four C2 frames of a still view
// accumulated with the variance, Renderer::denoiseLum with RESTIR_DENOISE_VAR_ACCUM and the tone fields, write the file.
// Used by tests/test_cpp_denoise_lum.py (compiled on CPU; run on the GPU box), which compares the file written here with
// the Python binding's of the same scene and frames.
//
//   denoise_lum_frames <scene.bin> <out.bmp> <width> <height>
//
// Exit 0 when the file is written, one frame filtered with the spatial estimate equals restir_denoise_lum_host over the
// frame and the G-buffer of the stage API bit for bit, ACCUM with one frame throws and leaves the accumulation open, and
// the accumulation still holds four frames after the call.  scene.bin: render_scene.cpp's format.
#include "scene_io.h"

#include <vector>

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: %s scene.bin out.bmp W H\n", argv[0]); return 2; }
    const uint32_t W = uint32_t(std::atoi(argv[3])), H = uint32_t(std::atoi(argv[4]));
    romis::Camera camera;
    romis::Scene scene = read_scene(argv[1], &camera);
    const size_t npx = size_t(W) * H;

    romis::Features features;   // bench.py's C2
    features.num_samples_in_reservoir = 1;
    features.initial_light_samples = 32;
    features.num_neighbours_to_sample = 5;
    features.spatial_resample_radius = 10;
    features.spatial_resampling_passes = 1;
    features.temporal_reuse = 0;
    features.enable_tone_mapping = 0;
    romis::Features tone;
    tone.enable_tone_mapping = 1;
    tone.exposure = 1.5f;
    tone.gamma = 2.2f;
    try {
        romis::Renderer renderer(0);
        renderer.setScene(scene);
        std::vector<float> n_t(4 * npx), p_mat(4 * npx);
        romis::check(restir_stage_configure(renderer.handle(), W, H, 1), "restir_stage_configure");
        romis::check(restir_stage_primary(renderer.handle(), &camera), "restir_stage_primary");
        romis::check(restir_stage_download(renderer.handle(), RESTIR_BUF_GBUF_N_T, n_t.data(), n_t.size() * 4), "restir_stage_download");
        romis::check(restir_stage_download(renderer.handle(), RESTIR_BUF_GBUF_P_MAT, p_mat.data(), p_mat.size() * 4), "restir_stage_download");

        // one frame, the spatial estimate, against the host function
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        std::vector<float> raw(3 * npx), got(3 * npx), want(3 * npx);
        romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, raw.data()), "restir_render");
        const romis::DenoiseLumParams spatial;
        renderer.denoiseLum(camera, W, H, spatial, nullptr, got.data());
        romis::check(restir_denoise_lum_host(raw.data(), nullptr, n_t.data(), p_mat.data(), W, H, uint32_t(scene.meshes.size()), &spatial,
                                             want.data(), nullptr), "restir_denoise_lum_host");
        if (std::memcmp(got.data(), want.data(), got.size() * 4)) {
            std::fprintf(stderr, "the filtered frame is not restir_denoise_lum_host's\n");
            return 1;
        }

        // four frames accumulated with the variance; ACCUM needs two of them
        romis::DenoiseLumParams accum;
        accum.variance_source = RESTIR_DENOISE_VAR_ACCUM;
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        renderer.accumBegin(true);
        for (int k = 0; k < 4; k++) {
            romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, nullptr), "restir_render");
            renderer.accumAdd();
            if (k == 0) {
                try {
                    renderer.denoiseLum(camera, W, H, accum);
                    std::fprintf(stderr, "expected an exception from ACCUM over one frame\n");
                    return 1;
                } catch (const std::runtime_error&) {
                }
            }
        }
        renderer.denoiseLum(camera, W, H, accum, &tone);
        restir_accum_stats stats{};
        romis::check(restir_accum_stats_get(renderer.handle(), &stats), "restir_accum_stats_get");
        if (stats.frames != 4u) {
            std::fprintf(stderr, "%u frames in the accumulation after the call\n", stats.frames);
            return 1;
        }
        if (renderer.denoiseGuideBuilds() != 1u) {
            std::fprintf(stderr, "%llu guide traces for one still view\n", (unsigned long long)renderer.denoiseGuideBuilds());
            return 1;
        }
        renderer.writeBitmapToFile(argv[2]);
        renderer.accumEnd();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
