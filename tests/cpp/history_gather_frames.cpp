// "Render while the camera turns, show the history's filtered mean" with the bilinear gather, through the C++ wrapper:
// Renderer::historyGather(HistoryGather::Bilinear), then history_frames.cpp's loop -- four C2 frames of a yawing camera, each
// folded into the image history, Renderer::historyDenoise with the tone fields, write the file.  Used by
// tests/test_cpp_history_gather.py (compiled on CPU; run on the GPU box), which compares the file written here with the
// Python binding's of the same scene, cameras and frames in the same mode.
//
//   history_gather_frames <scene.bin> <out.bmp> <width> <height> <yaw step>
//
// Exit 0 when the file is written, the mode reads Nearest before it is set and Bilinear after -- across historyBegin and
// historyEnd too --, a mode above 1 throws and changes nothing, and every advance but the first keeps some pixels.
// scene.bin: render_scene.cpp's format; the yaw step is added to the camera's rotation[1] before every frame but the first.
#include "scene_io.h"

#include <vector>

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: %s scene.bin out.bmp W H yaw_step\n", argv[0]); return 2; }
    const uint32_t W = uint32_t(std::atoi(argv[3])), H = uint32_t(std::atoi(argv[4]));
    const float step = float(std::atof(argv[5]));
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
        if (renderer.historyGather() != romis::HistoryGather::Nearest) { std::fprintf(stderr, "the default mode is not Nearest\n"); return 1; }
        renderer.historyGather(romis::HistoryGather::Bilinear);   // before a scene and before a history: context state
        renderer.setScene(scene);
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        try {
            renderer.historyGather(static_cast<romis::HistoryGather>(2));
            std::fprintf(stderr, "expected an exception from mode 2\n");
            return 1;
        } catch (const std::runtime_error&) {
        }
        const romis::HistoryParams params;
        renderer.historyBegin(params);
        if (renderer.historyGather() != romis::HistoryGather::Bilinear) { std::fprintf(stderr, "the mode did not survive\n"); return 1; }
        std::vector<float> raw(3 * npx);
        std::vector<uint32_t> map(npx);
        for (int k = 0; k < 4; k++) {
            if (k) camera.rotation[1] += step;
            romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, raw.data()), "restir_render");
            renderer.historyAdvance(camera, W, H, map.data());
            size_t kept = 0;
            for (uint32_t m : map) kept += m <= 0xFFFFFFFFu - 8u;
            if ((k == 0) != (kept == 0)) { std::fprintf(stderr, "advance %d keeps %zu pixels\n", k, kept); return 1; }
        }
        const auto frames = renderer.historyFrames();
        if (frames.first != 4u || frames.second != 0u) {
            std::fprintf(stderr, "%llu advances, %llu resets\n", (unsigned long long)frames.first, (unsigned long long)frames.second);
            return 1;
        }
        renderer.historyDenoise(romis::DenoiseLumParams(), &tone);
        renderer.writeBitmapToFile(argv[2]);
        renderer.historyEnd();
        if (renderer.historyGather() != romis::HistoryGather::Bilinear) { std::fprintf(stderr, "historyEnd changed the mode\n"); return 1; }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
