// Two frames rendered back to back through the C++ wrapper, a snapshot taken of each (Renderer::present) while the
// next is already enqueued, both written as BMP files.  Used by tests/test_gpu_present.py (compiled on CPU; run on the
// GPU box), which compares the files with Renderer.write_bmp's of the same frames.
//
//   present_frames <scene.bin> <out0.bmp> <out1.bmp> <width> <height>
//
// Frames 0 and 1 of the scene as read (no temporal reuse, two passes, N = 1, tone mapping off), neither read back as
// floats: frame 1 is enqueued before frame 0's snapshot is waited for.  Exit 0 when both files are written, the two
// snapshots differ and a fifth unreleased snapshot throws.  scene.bin: render_scene.cpp's format.
#include "scene_io.h"

#include <vector>

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: %s scene.bin out0.bmp out1.bmp W H\n", argv[0]); return 2; }
    const uint32_t W = uint32_t(std::atoi(argv[4])), H = uint32_t(std::atoi(argv[5]));
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
        auto render = [&] {   // enqueues only: no host image, no grid
            romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, nullptr),
                         "restir_render");
        };
        render();
        romis::PresentedImage first = renderer.present(RESTIR_IMAGE_BGRA8_BOTTOM_UP);
        render();   // overwrites the image at once: the first snapshot lives in its staging buffer
        romis::PresentedImage second = renderer.present(RESTIR_IMAGE_BGRA8_BOTTOM_UP);
        if (first.width() != W || first.height() != H || first.bytes() != size_t(W) * H * 4 || second.bytes() != first.bytes()) {
            std::fprintf(stderr, "snapshot of another size\n");
            return 1;
        }
        first.writeBitmapToFile(argv[2]);
        second.writeBitmapToFile(argv[3]);
        if (!std::memcmp(first.wait(), second.wait(), first.bytes())) {
            std::fprintf(stderr, "the two frames' snapshots are equal\n");
            return 1;
        }
        if (!first.ready() || !second.ready()) { std::fprintf(stderr, "a waited snapshot is not ready\n"); return 1; }
        {
            romis::PresentedImage third = renderer.present(), fourth = renderer.present(RESTIR_IMAGE_RGB32F);
            try {
                romis::PresentedImage fifth = renderer.present();   // throws: RESTIR_MAX_IMAGES_IN_FLIGHT are unreleased
                std::fprintf(stderr, "expected an exception\n");
                return 1;
            } catch (const std::runtime_error&) {
            }
        }
        if (renderer.downloadRgba8().size() != size_t(W) * H * 4) { std::fprintf(stderr, "downloadRgba8: wrong size\n"); return 1; }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
