// phat_layout -- csrc/phat_table.h's indices on the host, for tests/test_phat_layout.py:
//
//     phat_layout VW VH L M
//
// prints "row_floats R rows N size S lds B fast F" (F: the consumer kernel serves L lights and M candidates), then for
// every pixel (x, y) of the VW x VH view, row-major, one line
// "x y row first last" -- the pixel's row and pt_index of its lights 0 and L - 1 -- then for every (tile, wave, step) one
// line "span tile wave step row" (the first of the kPtStepPx rows the wave reads in that step).  Before it prints, it marks
// every (row, light) entry in a table-sized bitmap of its own: an entry marked twice, or outside the table, ends the
// program with status 1 (the check a sanitizer build repeats on the bitmap's accesses).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "phat_table.h"

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: phat_layout VW VH L M\n");
        return 2;
    }
    const uint32_t vw = (uint32_t)std::strtoul(argv[1], nullptr, 10), vh = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const uint32_t L = (uint32_t)std::strtoul(argv[3], nullptr, 10), M = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    if (!vw || !vh || !L || L > romis::kPtMaxLights) return 2;
    const uint32_t rf = romis::pt_row_floats(L);
    const size_t size = romis::pt_size(vw, vh, L);
    std::vector<bool> seen(size, false);
    for (uint32_t y = 0; y < vh; y++)
        for (uint32_t x = 0; x < vw; x++)
            for (uint32_t i = 0; i < L; i++) {
                const size_t idx = romis::pt_index(romis::pt_row(vw, x, y), rf, i);
                if (idx >= size || seen[idx]) {
                    std::fprintf(stderr, "entry (%u, %u, light %u) at %zu: %s\n", x, y, i, idx, idx >= size ? "outside" : "twice");
                    return 1;
                }
                seen[idx] = true;
            }
    std::printf("row_floats %u rows %zu size %zu lds %zu fast %d\n", rf, romis::pt_rows(vw, vh), size, romis::pt_lds_bytes(L),
                romis::pt_fast(L, M) ? 1 : 0);
    for (uint32_t y = 0; y < vh; y++)
        for (uint32_t x = 0; x < vw; x++) {
            const size_t row = romis::pt_row(vw, x, y);
            std::printf("%u %u %zu %zu %zu\n", x, y, row, romis::pt_index(row, rf, 0u), romis::pt_index(row, rf, L - 1u));
        }
    for (uint32_t tile = 0; tile < romis::pt_tiles(vw, vh); tile++)
        for (uint32_t wave = 0; wave < 4u; wave++)
            for (uint32_t step = 0; step < 64u / romis::kPtStepPx; step++)
                std::printf("span %u %u %u %zu\n", tile, wave, step, romis::pt_step_row(tile, wave, step));
    return 0;
}
