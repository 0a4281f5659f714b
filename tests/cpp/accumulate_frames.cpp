// A still view accumulated on the device through the C++ wrapper: renderAccumulated averages `frames` independent
// frames, tone maps the mean and hands it back; the resolved image, which is then the Renderer's last image, is written
// as a BMP file without its floats being converted on the host.  Used by tests/test_cpp_accumulate.py (compiled on CPU;
// run on the GPU box), which compares the file with the Python binding's of the same scene and seed.
//
//   accumulate_frames <scene.bin> <out.bmp> <width> <height> <frames>
//
// Frames 0 .. frames - 1 of the scene as read (no temporal reuse, two passes, N = 1), tone mapped after the mean with
// exposure 1.5 and gamma 2.2.  Exit 0 when the file is written, the stats name `frames` frames of that size, the image
// handed back is the last image, an add of the resolved image throws, two more frames added by hand are counted and a
// resolve without tone mapping hands back the mean's bits.  scene.bin: render_scene.cpp's format.
#include "scene_io.h"

#include <vector>

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: %s scene.bin out.bmp W H frames\n", argv[0]); return 2; }
    const uint32_t W = uint32_t(std::atoi(argv[3])), H = uint32_t(std::atoi(argv[4])), frames = uint32_t(std::atoi(argv[5]));
    romis::Camera camera;
    romis::Scene scene = read_scene(argv[1], &camera);

    romis::Features features;
    features.num_samples_in_reservoir = 1;
    features.spatial_resampling_passes = 2;
    features.temporal_reuse = 0;
    features.enable_tone_mapping = 1;
    features.exposure = 1.5f;
    features.gamma = 2.2f;
    try {
        romis::Renderer renderer(0);
        renderer.setScene(scene);
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        romis::Screen screen(static_cast<int>(W), static_cast<int>(H));
        const restir_accum_stats stats = romis::renderAccumulated(renderer, camera, screen, features, frames);
        if (stats.width != W || stats.height != H || stats.frames != frames || !(stats.est_mse >= 0.0)) {
            std::fprintf(stderr, "stats: %ux%u, %u frames, est_mse %g\n", stats.width, stats.height, stats.frames, stats.est_mse);
            return 1;
        }
        renderer.writeBitmapToFile(argv[2]);   // the resolved image is the last image
        std::vector<float> last(size_t(W) * H * 3);
        romis::check(restir_download_rgb(renderer.handle(), last.data(), last.size()), "restir_download_rgb");
        if (std::memcmp(last.data(), screen.rgb.data(), last.size() * 4)) {
            std::fprintf(stderr, "the image handed back is not the last image\n");
            return 1;
        }
        try {
            renderer.accumAdd();   // throws: the last image is the resolve's
            std::fprintf(stderr, "expected an exception\n");
            return 1;
        } catch (const std::runtime_error&) {
        }
        // the accumulation stays open: two more frames by hand
        romis::Features linear = features;
        linear.enable_tone_mapping = 0;
        for (int i = 0; i < 2; i++) {
            romis::check(restir_render(renderer.handle(), &camera, &linear, W, H, nullptr, nullptr, nullptr, nullptr), "restir_render");
            renderer.accumAdd();
        }
        if (renderer.accumStats().frames != frames + 2u) { std::fprintf(stderr, "accumStats: wrong frame count\n"); return 1; }
        std::vector<float> mean, m2;
        renderer.accumState(mean, m2, W, H);
        renderer.accumResolve();
        romis::check(restir_download_rgb(renderer.handle(), last.data(), last.size()), "restir_download_rgb");
        if (std::memcmp(last.data(), mean.data(), last.size() * 4)) {
            std::fprintf(stderr, "a resolve without tone mapping is not the mean\n");
            return 1;
        }
        renderer.accumEnd();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
