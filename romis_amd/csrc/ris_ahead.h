// ris_ahead.h -- the key of a RIS look-ahead result (restir.cpp Frame::ris_stage, DESIGN.md §6 "RIS look-ahead").
// On a still view without temporal reuse, frame f + 1's RIS (k_gbuf_ris_n1_lds_pt_phat) reads nothing frame f writes, so
// restir_render launches it on a second stream beside frame f's last pass, into a second set of handle and pdf-cache
// planes.  The key names everything that launch's output is a function of; the next restir_render call takes the
// result only when the key of the frame it is about to render is equal, field for field.  Host only, no HIP include: a
// CPU test compiles it (tests/cpp/ris_ahead_key.cpp).
#pragma once

#include <cstdint>
#include <cstring>

namespace romis {

struct RisAheadKey {
    // the RNG key's inputs: restir_rng_key(seed, frame, RESTIR_STAGE_RIS, 0)
    uint32_t seed = 0, frame = 0;
    // what the launch read: the kept G-buffer (restir_ctx::gbuf_epoch names one), the light table and materials
    // (scene_gen), the geometry the G-buffer was traced over (geom_gen), one build of the p-hat table (phat_builds)
    uint64_t gbuf_epoch = 0, scene_gen = 0, geom_gen = 0, phat_build = 0;
    // the GbufView: CameraDev as bits (quat, origin, half_w, half_h), the image size, the restir_tile's ten words
    uint32_t cam[9] = {};
    uint32_t width = 0, height = 0;
    uint32_t tile[10] = {};
    uint32_t tex_on = 0;
    // FeaturesDev, whole: ris_pixel takes M, N, shading, initial_vis and texture; the frame's plan (handles, tile flags,
    // what RIS may skip) takes the passes' K, R, unbiased and spatial_vis, so a result is not kept across any of them
    uint32_t features[22] = {};
    uint32_t passes = 0;
    // the launch as routed: Route::grid, ::lds, and its buffer decisions (ris_ahead_route_bits)
    uint32_t route_grid = 0, route_lds = 0, route_bits = 0;
    // counts the restir_set_tuning calls of knobs that clear the kept G-buffer
    uint64_t tuning_gen = 0;
};

constexpr uint32_t kRisAheadKeyFields = 17;   // members above; the test has one case per member
static_assert(sizeof(RisAheadKey) == 4 * (2 + 9 + 2 + 10 + 1 + 22 + 1 + 3) + 8 * 5,
              "RisAheadKey changed: compare the new member in ris_ahead_key_equal, count it in kRisAheadKeyFields and "
              "give it a case in tests/cpp/ris_ahead_key.cpp");

inline bool ris_ahead_key_equal(const RisAheadKey& a, const RisAheadKey& b) {
    return a.seed == b.seed && a.frame == b.frame && a.gbuf_epoch == b.gbuf_epoch && a.scene_gen == b.scene_gen &&
           a.geom_gen == b.geom_gen && a.phat_build == b.phat_build && !std::memcmp(a.cam, b.cam, sizeof(a.cam)) &&
           a.width == b.width && a.height == b.height && !std::memcmp(a.tile, b.tile, sizeof(a.tile)) &&
           a.tex_on == b.tex_on && !std::memcmp(a.features, b.features, sizeof(a.features)) && a.passes == b.passes &&
           a.route_grid == b.route_grid && a.route_lds == b.route_lds && a.route_bits == b.route_bits &&
           a.tuning_gen == b.tuning_gen;
}

// The key of the frame after `k` on the same view: what a look-ahead launched beside frame k.frame is keyed by
inline RisAheadKey ris_ahead_next(RisAheadKey k) {
    k.frame += 1u;
    return k;
}

// Which of two plane sets a frame's grid 0 reads its handles and pdf cache from, and the one the look-ahead beside it
// writes: the other
inline int ris_ahead_other_set(int set) { return set ^ 1; }

}  // namespace romis
