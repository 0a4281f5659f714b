// The exact direct-lighting image and the error figures against it through the C++ wrapper: romis::renderExact renders
// the exact image of a point-light scene into a Screen, the Renderer keeps it as the reference, and a frame and a short
// accumulation are measured against it on the device.  Used by tests/test_cpp_exact.py (compiled on CPU; run on the GPU
// box), which compares the file written here with the Python binding's of the same scene.
//
//   exact_image <scene.bin> <out.bmp> <width> <height>
//
// Exit 0 when the file is written (the exact image, tone mapped with exposure 1.5 and gamma 2.2), the linear exact image
// handed back is the last image, its error against itself is zero in every figure, a frame's figures equal
// restir_error_measure's over the downloaded arrays, the accumulated mean's name their frame count, and an error without a
// reference throws.  scene.bin: render_scene.cpp's format.
#include "scene_io.h"

#include <vector>

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: %s scene.bin out.bmp W H\n", argv[0]); return 2; }
    const uint32_t W = uint32_t(std::atoi(argv[3])), H = uint32_t(std::atoi(argv[4]));
    romis::Camera camera;
    romis::Scene scene = read_scene(argv[1], &camera);

    romis::Features features;
    features.num_samples_in_reservoir = 1;
    features.spatial_resampling_passes = 2;
    features.temporal_reuse = 0;
    features.enable_tone_mapping = 0;
    try {
        romis::Renderer renderer(0);
        renderer.setScene(scene);
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        try {
            (void)renderer.error();   // throws: no reference
            std::fprintf(stderr, "expected an exception\n");
            return 1;
        } catch (const std::runtime_error&) {
        }
        romis::Screen screen(static_cast<int>(W), static_cast<int>(H));
        romis::renderExact(renderer, camera, screen, features);
        std::vector<float> last(size_t(W) * H * 3);
        romis::check(restir_download_rgb(renderer.handle(), last.data(), last.size()), "restir_download_rgb");
        if (std::memcmp(last.data(), screen.rgb.data(), last.size() * 4)) {
            std::fprintf(stderr, "the image handed back is not the last image\n");
            return 1;
        }
        renderer.referenceSet();
        const restir_error_stats self = renderer.error();
        if (self.width != W || self.height != H || self.counted + self.nonfinite != uint64_t(W) * H * 3 || self.mse != 0.0 ||
            self.mae != 0.0 || self.rel_mse != 0.0 || self.bias != 0.0 || self.max_abs != 0.0) {
            std::fprintf(stderr, "the exact image against itself: mse %g, max %g\n", self.mse, self.max_abs);
            return 1;
        }
        // a frame, then the mean of three, against the exact image
        renderer.accumBegin(false);
        for (int i = 0; i < 3; i++) {
            romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, nullptr), "restir_render");
            renderer.accumAdd();
        }
        const restir_error_stats frame = renderer.error(RESTIR_ERROR_SRC_IMAGE);
        romis::check(restir_download_rgb(renderer.handle(), last.data(), last.size()), "restir_download_rgb");
        restir_error_stats host{};
        romis::check(restir_error_measure(last.data(), screen.rgb.data(), last.size(), &host), "restir_error_measure");
        if (frame.counted != host.counted || frame.nonfinite != host.nonfinite || frame.mse != host.mse || frame.mae != host.mae ||
            frame.rel_mse != host.rel_mse || frame.bias != host.bias || frame.max_abs != host.max_abs ||
            frame.ref_mean != host.ref_mean || !(frame.mse > 0.0)) {
            std::fprintf(stderr, "a frame's figures: device mse %.17g, host %.17g\n", frame.mse, host.mse);
            return 1;
        }
        const restir_error_stats mean = renderer.error(RESTIR_ERROR_SRC_ACCUM_MEAN);
        if (mean.frames != 3u || mean.source != RESTIR_ERROR_SRC_ACCUM_MEAN || !(mean.mse > 0.0)) {
            std::fprintf(stderr, "the mean's figures: %u frames, mse %g\n", mean.frames, mean.mse);
            return 1;
        }
        renderer.accumEnd();
        renderer.referenceClear();
        // the file: the exact image tone mapped
        romis::Features toned = features;
        toned.enable_tone_mapping = 1;
        toned.exposure = 1.5f;
        toned.gamma = 2.2f;
        renderer.renderExact(camera, toned, W, H);
        renderer.writeBitmapToFile(argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
