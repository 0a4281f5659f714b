// Moves a mesh and replaces the lights through the C++ wrapper (Renderer::updateMeshes / setLights) and compares the
// next frame with a second Renderer's setScene of the moved scene.  Used by tests/test_cpp_dynamic_scene.py (compiled
// on CPU; run on the GPU box), which also compares the written frame with the oracle's.
//
//   update_scene <scene.bin> <out.rgb> <width> <height> <mesh> <dx> <dy> <dz> <lights kept>
//
// Frame 0 of the scene as read; then mesh <mesh> moves by (dx, dy, dz) and only the first <lights kept> lights stay;
// frame 1 (no temporal reuse, two passes, N = 1) goes to out.rgb.  Exit 0 when it equals the fresh upload's frame 1
// bit for bit and a bad mesh index throws.  scene.bin: render_scene.cpp's format.
#include "scene_io.h"

#include <vector>

int main(int argc, char** argv) {
    if (argc < 10) { std::fprintf(stderr, "usage: %s scene.bin out.rgb W H mesh dx dy dz lights\n", argv[0]); return 2; }
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
    const uint32_t mesh = uint32_t(std::atoi(argv[5]));
    const float d[3] = {float(std::atof(argv[6])), float(std::atof(argv[7])), float(std::atof(argv[8]))};
    const size_t kept = size_t(std::atoi(argv[9]));
    romis::Camera camera;
    romis::Scene scene = read_scene(argv[1], &camera);
    if (mesh >= scene.meshes.size() || kept > scene.lights.size()) { std::fprintf(stderr, "bad mesh / light count\n"); return 2; }

    romis::Features features;
    features.num_samples_in_reservoir = 1;
    features.spatial_resampling_passes = 2;
    features.temporal_reuse = 0;
    try {
        romis::Renderer renderer(0);
        renderer.setScene(scene);
        renderer.setSeed(RESTIR_DEFAULT_SEED, 0);
        romis::Screen first(W, H), updated(W, H), fresh(W, H);
        romis::renderRayTraced(renderer, nullptr, camera, first, features);

        romis::Scene moved = scene;
        romis::Mesh& m = moved.meshes[mesh];
        for (size_t i = 0; i < m.positions.size(); i++) m.positions[i] = m.positions[i] + d[i % 3];
        moved.lights.resize(kept);
        romis::Mesh only_positions;
        only_positions.positions = m.positions;   // no normals: the uploaded ones stay
        renderer.updateMeshes({{mesh, &only_positions}});
        renderer.setLights(moved.lights);
        romis::renderRayTraced(renderer, nullptr, camera, updated, features);

        romis::Renderer other(0);
        other.setScene(moved);
        other.setSeed(RESTIR_DEFAULT_SEED, 1);
        romis::renderRayTraced(other, nullptr, camera, fresh, features);
        if (updated.rgb.size() != fresh.rgb.size() ||
            std::memcmp(updated.rgb.data(), fresh.rgb.data(), updated.rgb.size() * sizeof(float)) != 0) {
            std::fprintf(stderr, "the updated scene's frame differs from the fresh upload's\n");
            return 1;
        }
        if (!std::memcmp(updated.rgb.data(), first.rgb.data(), updated.rgb.size() * sizeof(float))) {
            std::fprintf(stderr, "the update changed nothing\n");
            return 1;
        }
        FILE* o = std::fopen(argv[2], "wb");
        std::fwrite(updated.rgb.data(), sizeof(float), updated.rgb.size(), o);
        std::fclose(o);
        try {
            renderer.updateMeshes({{uint32_t(scene.meshes.size()), &only_positions}});   // throws, as the rest do
            std::fprintf(stderr, "expected an exception\n");
            return 1;
        } catch (const std::runtime_error&) {
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
