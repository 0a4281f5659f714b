// ris_ahead_key.cpp -- csrc/ris_ahead.h on the CPU (tests/test_ris_ahead_key.py): the look-ahead key compares equal to
// itself and unequal when any one member differs.  Prints one line per case, "<member> <equal-to-base>", after a head
// line with the header's own member count and size; a member added to the struct without a case here changes the size
// the test pins.  Plain C++, no HIP header.
#include <cstdio>
#include <cstring>

#include "ris_ahead.h"

using romis::RisAheadKey;

static RisAheadKey base() {
    RisAheadKey k;
    k.seed = 0x5EED0001u; k.frame = 41u;
    k.gbuf_epoch = 3; k.scene_gen = 7; k.geom_gen = 5; k.phat_build = 2;
    for (int i = 0; i < 9; i++) k.cam[i] = 0x3f800000u + (uint32_t)i;
    k.width = 1920; k.height = 1080;
    for (int i = 0; i < 10; i++) k.tile[i] = 100u + (uint32_t)i;
    k.tex_on = 1;
    for (int i = 0; i < 22; i++) k.features[i] = 1000u + (uint32_t)i;
    k.passes = 1;
    k.route_grid = 8160; k.route_lds = 8192; k.route_bits = 0x1234;
    k.tuning_gen = 9;
    return k;
}

int main() {
    const RisAheadKey b = base();
    std::printf("fields %u %zu\n", romis::kRisAheadKeyFields, sizeof(RisAheadKey));
    std::printf("self %d\n", romis::ris_ahead_key_equal(b, b) ? 1 : 0);
    RisAheadKey copy;
    std::memcpy(&copy, &b, sizeof(b));
    std::printf("copy %d\n", romis::ris_ahead_key_equal(b, copy) ? 1 : 0);
    unsigned cases = 0;
#define CASE(name, change)                                                                \
    do {                                                                                  \
        RisAheadKey k = base();                                                           \
        change;                                                                           \
        std::printf("%s %d\n", name, romis::ris_ahead_key_equal(b, k) ? 1 : 0);            \
        std::printf("%s_swapped %d\n", name, romis::ris_ahead_key_equal(k, b) ? 1 : 0);    \
        cases++;                                                                          \
    } while (0)
    CASE("seed", k.seed ^= 1u);
    CASE("frame", k.frame += 2u);
    CASE("gbuf_epoch", k.gbuf_epoch += 1);
    CASE("scene_gen", k.scene_gen += 1);
    CASE("geom_gen", k.geom_gen += 1);
    CASE("phat_build", k.phat_build += 1);
    CASE("cam", k.cam[8] ^= 1u);            // the last word: the comparison covers the whole array
    CASE("width", k.width -= 1);
    CASE("height", k.height += 1);
    CASE("tile", k.tile[9] += 1);
    CASE("tex_on", k.tex_on = 0);
    CASE("features", k.features[21] += 1);
    CASE("passes", k.passes = 2);
    CASE("route_grid", k.route_grid += 1);
    CASE("route_lds", k.route_lds += 16);
    CASE("route_bits", k.route_bits ^= 0x10000u);
    CASE("tuning_gen", k.tuning_gen += 1);
    // every word of the arrays, not only the last
    for (int i = 0; i < 9; i++) { RisAheadKey k = base(); k.cam[i] ^= 0x80000000u; std::printf("cam_word %d\n", romis::ris_ahead_key_equal(b, k) ? 1 : 0); }
    for (int i = 0; i < 10; i++) { RisAheadKey k = base(); k.tile[i] += 1; std::printf("tile_word %d\n", romis::ris_ahead_key_equal(b, k) ? 1 : 0); }
    for (int i = 0; i < 22; i++) { RisAheadKey k = base(); k.features[i] += 1; std::printf("features_word %d\n", romis::ris_ahead_key_equal(b, k) ? 1 : 0); }
    std::printf("cases %u\n", cases);
    // the key a look-ahead is stored under is the next frame's, and nothing else of the frame's own
    const RisAheadKey n = romis::ris_ahead_next(b);
    RisAheadKey want = base();
    want.frame += 1u;
    std::printf("next %d %d\n", romis::ris_ahead_key_equal(n, want) ? 1 : 0, romis::ris_ahead_key_equal(n, b) ? 1 : 0);
    RisAheadKey wrap = base();
    wrap.frame = 0xFFFFFFFFu;
    std::printf("next_wraps %u\n", romis::ris_ahead_next(wrap).frame);
    std::printf("other_set %d %d\n", romis::ris_ahead_other_set(0), romis::ris_ahead_other_set(1));
    return 0;
}
