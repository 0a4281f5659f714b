// shadow_vis_layout -- csrc/shadow_vis.h's indices on the host, for tests/test_shadow_vis_layout.py:
//
//     shadow_vis_layout RW RH L
//
// prints "words W size S", then for every pixel (x, y) of the RW x RH rect, row-major, one line "x y slot first last" --
// the pixel's slot and sv_index of its words 0 and W - 1 -- and for every light i < L one line "light i word bit" (the
// bit as a mask).
#include <cstdio>
#include <cstdlib>

#include "shadow_vis.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: shadow_vis_layout RW RH L\n");
        return 2;
    }
    const uint32_t rw = (uint32_t)std::strtoul(argv[1], nullptr, 10), rh = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const uint32_t L = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    const uint32_t words = romis::sv_words(L);
    std::printf("words %u size %zu\n", words, romis::sv_size(rw, rh, L));
    for (uint32_t y = 0; y < rh; y++)
        for (uint32_t x = 0; x < rw; x++) {
            const size_t slot = romis::sv_slot(rw, x, y);
            std::printf("%u %u %zu %zu %zu\n", x, y, slot, romis::sv_index(slot, words, 0u), romis::sv_index(slot, words, words - 1u));
        }
    for (uint32_t i = 0; i < L; i++) std::printf("light %u %u %u\n", i, romis::sv_word_of(i), romis::sv_bit(i));
    return 0;
}
