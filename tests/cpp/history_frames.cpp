// "Render while the camera turns, show the history's filtered mean" through the C++ wrapper: four C2 frames of a yawing
// camera, each folded into the image history (Renderer::historyAdvance), then Renderer::historyDenoise with the tone
// fields, write the file.  Used by tests/test_cpp_history.py (compiled on CPU; run on the GPU box), which compares the file
// written here with the Python binding's of the same scene, cameras and frames.
//
//   history_frames <scene.bin> <out.bmp> <width> <height> <yaw step>
//
// Exit 0 when the file is written, the first advance's map is all "no history", the state after every advance equals
// restir_history_fold of the state before, the advance's map and the frame bit for bit, an advance of the same image twice
// throws and leaves the history as it was, and one view is traced once across historyAdvance and historyDenoise.
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
        renderer.setScene(scene);
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        const romis::HistoryParams params;
        renderer.historyBegin(params);
        std::vector<float> mean(3 * npx, 0.0f), S(3 * npx, 0.0f), mean1(3 * npx), S1(3 * npx), raw(3 * npx), gm, gs;
        std::vector<uint32_t> n(npx, 0u), n1(npx), map(npx), gn;
        for (int k = 0; k < 4; k++) {
            if (k) camera.rotation[1] += step;
            romis::check(restir_render(renderer.handle(), &camera, &features, W, H, nullptr, nullptr, nullptr, raw.data()), "restir_render");
            renderer.historyAdvance(camera, W, H, map.data());
            if (k == 0)
                for (uint32_t m : map)
                    if (m != 0xFFFFFFFFu - 7u) { std::fprintf(stderr, "the first advance's map holds %08x\n", m); return 1; }
            romis::check(restir_history_fold(mean.data(), S.data(), n.data(), map.data(), raw.data(), W, H, params.max_frames, mean1.data(),
                                             S1.data(), n1.data()), "restir_history_fold");
            mean.swap(mean1); S.swap(S1); n.swap(n1);
            renderer.historyState(gm, gs, gn, W, H);
            if (std::memcmp(gm.data(), mean.data(), npx * 12) || std::memcmp(gs.data(), S.data(), npx * 12) ||
                std::memcmp(gn.data(), n.data(), npx * 4)) {
                std::fprintf(stderr, "the state after advance %d is not restir_history_fold's\n", k);
                return 1;
            }
        }
        try {
            renderer.historyAdvance(camera, W, H);
            std::fprintf(stderr, "expected an exception from a second advance of one image\n");
            return 1;
        } catch (const std::runtime_error&) {
        }
        const auto frames = renderer.historyFrames();
        if (frames.first != 4u || frames.second != 0u) {
            std::fprintf(stderr, "%llu advances, %llu resets\n", (unsigned long long)frames.first, (unsigned long long)frames.second);
            return 1;
        }
        renderer.historyDenoise(romis::DenoiseLumParams(), &tone);
        if (renderer.denoiseGuideBuilds() != 4u) {
            std::fprintf(stderr, "%llu guide traces for four views\n", (unsigned long long)renderer.denoiseGuideBuilds());
            return 1;
        }
        renderer.writeBitmapToFile(argv[2]);
        renderer.historyEnd();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
