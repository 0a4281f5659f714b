// shadow_vis.h -- the answers of the fused last pass's shadow rays, one bit per (pixel, point light) of a still view
// (DESIGN.md §6 "Visibility bits").  Whether the segment from a pixel's hit point to light i is blocked depends on the
// kept G-buffer, the light table and the geometry alone -- what the shadow lists' key names -- so once the lists stand,
// shadow_vis.hip k_shadow_vis asks visible_listed() that question once for every pixel and light, with the operands the
// frame kernel passes, and every later frame's ray (k_spatial1hg_t2_final_vis) is one 4-byte load.  A stored bit is that
// call's return value, nothing derived.
//
// Layout: per-pixel records of sv_words(L) 32-bit words, the pixels in the frame kernel's own order -- the 32 x 16 tiles
// of the pass's rect row-major (lean_tile<2>'s numbering), inside a tile the 512 threads of the block (eight 8 x 8
// waves, spatial1h_body's pixel of thread t) -- so a wave's 64 records are one contiguous run of 64 * 4 * words bytes
// and thread t of tile k reads record 512 k + t.  A ragged tile's slots outside the rect exist and are never read.
//
// One text for the host (tests/test_shadow_vis_layout.py compiles it) and the kernels.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef ROMIS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROMIS_HD __host__ __device__ __forceinline__
#else
#define ROMIS_HD inline
#endif
#endif

namespace romis {

constexpr uint32_t kSvTileW = 32u, kSvTileH = 16u;   // the fused pass's tile (lean_tile<2>, shadow_lists.h kSlTile*)
constexpr uint32_t kSvTilePx = kSvTileW * kSvTileH;  // slots per tile: the block's threads
constexpr uint32_t kSvMaxWords = 8u;                 // L <= 254 (the handle path's light index) -> at most 8 words

ROMIS_HD uint32_t sv_words(uint32_t num_lights) { return (num_lights + 31u) / 32u; }
ROMIS_HD uint32_t sv_tiles(uint32_t rw, uint32_t rh) {
    return ((rw + kSvTileW - 1u) / kSvTileW) * ((rh + kSvTileH - 1u) / kSvTileH);
}
// 32-bit words of the plane of an rw x rh rect
ROMIS_HD size_t sv_size(uint32_t rw, uint32_t rh, uint32_t num_lights) {
    return (size_t)sv_tiles(rw, rh) * kSvTilePx * sv_words(num_lights);
}
// The slot of thread t of tile `tile`, and of the rect's pixel (x, y) (0-based in the rect): thread t = wave << 6 | lane
// holds the tile's pixel ((wave & 3) * 8 + (lane & 7), (wave >> 2) * 8 + (lane >> 3))
ROMIS_HD size_t sv_slot_of_thread(uint32_t tile, uint32_t t) { return (size_t)tile * kSvTilePx + t; }
ROMIS_HD uint32_t sv_thread(uint32_t lx, uint32_t ly) {   // lx < 32, ly < 16
    return ((((ly >> 3) << 2) | (lx >> 3)) << 6) | ((ly & 7u) << 3) | (lx & 7u);
}
ROMIS_HD size_t sv_slot(uint32_t rw, uint32_t x, uint32_t y) {
    const uint32_t ntx = (rw + kSvTileW - 1u) / kSvTileW;
    return sv_slot_of_thread((y / kSvTileH) * ntx + x / kSvTileW, sv_thread(x % kSvTileW, y % kSvTileH));
}
// The index of word w (< words) of the pixel in `slot`, the word that holds light i and the light's bit in it
ROMIS_HD size_t sv_index(size_t slot, uint32_t words, uint32_t w) { return slot * words + w; }
ROMIS_HD uint32_t sv_word_of(uint32_t light) { return light >> 5; }
ROMIS_HD uint32_t sv_bit(uint32_t light) { return 1u << (light & 31u); }

}  // namespace romis

#if defined(__HIPCC__)
#include "shadow_lists.h"

namespace romis {

// The plane of one build: `lists` is the build of the shadow lists it asks (their scene, rect, G-buffer plane and tile
// flags are the plane's own), `bits` sv_size(rect, L) words.
struct ShadowVisDev {
    ShadowListsDev lists;
    uint32_t* bits;
};
hipError_t launch_shadow_vis(const ShadowVisDev& d, hipStream_t stream);
// Per pixel of the rect (row-major, one byte each): the stored bit of light `light` (< L) as 0 / 1; 0xFF where the plane
// holds none -- a pixel of a background RIS tile, or one with the miss material
hipError_t launch_debug_shadow_vis(const ShadowVisDev& d, uint32_t light, uint8_t* out, hipStream_t stream);

}  // namespace romis
#endif
