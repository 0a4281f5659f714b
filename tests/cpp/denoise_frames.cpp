// The viewer's loop with the denoiser through the C++ wrapper: render a C2 frame with tone mapping off, denoise it with the
// tone fields (Renderer::denoise), write the file.  Used by tests/test_cpp_denoise.py (compiled on CPU; run on the GPU
// box), which compares the file written here with the Python binding's of the same scene and frame.
//
//   denoise_frames <scene.bin> <out.bmp> <width> <height>
//
// Exit 0 when the file is written, the linear denoised image equals romis::denoiseHost over the frame and the G-buffer
// of the stage API bit for bit, three denoised frames of a still view trace their guides once, the denoised image is
// refused by accumAdd, and parameters out of range throw.  scene.bin: render_scene.cpp's format.
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
        // the G-buffer of the view, as the stage API gives it
        std::vector<float> n_t(4 * npx), p_mat(4 * npx);
        romis::check(restir_stage_configure(renderer.handle(), W, H, 1), "restir_stage_configure");
        romis::check(restir_stage_primary(renderer.handle(), &camera), "restir_stage_primary");
        romis::check(restir_stage_download(renderer.handle(), RESTIR_BUF_GBUF_N_T, n_t.data(), n_t.size() * 4), "restir_stage_download");
        romis::check(restir_stage_download(renderer.handle(), RESTIR_BUF_GBUF_P_MAT, p_mat.data(), p_mat.size() * 4), "restir_stage_download");

        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        std::vector<float> raw(3 * npx), got(3 * npx);
        romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, raw.data()), "restir_render");
        const romis::DenoiseParams params;
        renderer.denoise(camera, W, H, params, nullptr, got.data());
        const std::vector<float> want = romis::denoiseHost(raw, n_t, p_mat, W, H, uint32_t(scene.meshes.size()), params);
        if (std::memcmp(got.data(), want.data(), got.size() * 4)) {
            std::fprintf(stderr, "the denoised frame is not denoiseHost's\n");
            return 1;
        }
        if (!std::memcmp(got.data(), raw.data(), got.size() * 4)) {
            std::fprintf(stderr, "the denoised frame is the raw frame\n");
            return 1;
        }
        renderer.accumBegin(false);
        try {
            renderer.accumAdd();   // throws: a denoised image is no frame
            std::fprintf(stderr, "expected an exception from accumAdd\n");
            return 1;
        } catch (const std::runtime_error&) {
        }
        renderer.accumEnd();
        romis::DenoiseParams bad;
        bad.iterations = RESTIR_DENOISE_MAX_ITERATIONS + 1u;
        try {
            renderer.denoise(camera, W, H, bad);
            std::fprintf(stderr, "expected an exception from six iterations\n");
            return 1;
        } catch (const std::runtime_error&) {
        }
        // the loop: render, denoise with the tone fields, (present); the guides are traced once
        for (int i = 0; i < 2; i++) {
            romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, nullptr), "restir_render");
            renderer.denoise(camera, W, H, params, &tone);
        }
        if (renderer.denoiseGuideBuilds() != 1u) {
            std::fprintf(stderr, "%llu guide traces for one still view\n", (unsigned long long)renderer.denoiseGuideBuilds());
            return 1;
        }
        // the file: frame 0 again, denoised and tone mapped
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, nullptr), "restir_render");
        renderer.denoise(camera, W, H, params, &tone);
        renderer.writeBitmapToFile(argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
