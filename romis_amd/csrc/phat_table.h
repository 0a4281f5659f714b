// phat_table.h -- RIS's target pdfs of a still view, one f32 per (pixel, point light) (DESIGN.md §6 "P-hat table").  For
// point lights a candidate is a light index, so the p-hat ris_pixel evaluates for it, target_pdf(px, lights[i],
// lights[L + i]), depends on the kept G-buffer, the light table, the materials and Features::shading alone -- not on the
// frame's RNG key.  phat_table.hip k_phat_table evaluates it once for every pixel and light with the frame kernel's own
// operands and functions, and k_gbuf_ris_n1_lds_pt_phat runs RIS's candidate loop over the stored values: a stored entry
// is that call's return value, nothing derived.
//
// Layout: one row of pt_row_floats(L) floats (L padded to a multiple of 4: 16-byte rows) per thread of the RIS kernel's
// launch, the rows in the consumer's own reading order -- the 32 x 8 tiles of the view row-major (the block index of
// k_gbuf_ris), inside a tile the block's thread t = wave << 6 | step << 4 | pixel-in-step, which holds the tile's pixel
// (t % 32, t / 32).  A wave reads its 64 rows in four steps of 16 rows: one contiguous span of 16 rows each.  A ragged
// tile's rows outside the view exist and are never read; nor are the rows of background tiles.
//
// One text for the host (tests/test_phat_layout.py compiles it) and the kernels.
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

constexpr uint32_t kPtTileW = 32u, kPtTileH = 8u;     // the RIS kernels' tile (launch_shape.h kTileW x kTileH)
constexpr uint32_t kPtTilePx = kPtTileW * kPtTileH;   // rows per tile: the block's threads
constexpr uint32_t kPtStepPx = 16u;                   // pixels a wave takes per step
constexpr uint32_t kPtLanesPerPx = 64u / kPtStepPx;   // ... with this many lanes each
constexpr uint32_t kPtMaxLights = 254u;               // the handle planes' light index

ROMIS_HD uint32_t pt_row_floats(uint32_t num_lights) { return (num_lights + 3u) & ~3u; }
ROMIS_HD uint32_t pt_tiles(uint32_t vw, uint32_t vh) {
    return ((vw + kPtTileW - 1u) / kPtTileW) * ((vh + kPtTileH - 1u) / kPtTileH);
}
ROMIS_HD size_t pt_rows(uint32_t vw, uint32_t vh) { return (size_t)pt_tiles(vw, vh) * kPtTilePx; }
// floats of the table of a vw x vh view
ROMIS_HD size_t pt_size(uint32_t vw, uint32_t vh, uint32_t num_lights) { return pt_rows(vw, vh) * pt_row_floats(num_lights); }
// The row of thread t of tile `tile`, and its parts: wave, step, pixel-in-step
ROMIS_HD size_t pt_row_of_thread(uint32_t tile, uint32_t t) { return (size_t)tile * kPtTilePx + t; }
ROMIS_HD uint32_t pt_thread(uint32_t wave, uint32_t step, uint32_t q) { return (wave << 6) | (step * kPtStepPx) | q; }
// The first row of the span wave `wave` of tile `tile` reads in step `step` (kPtStepPx rows)
ROMIS_HD size_t pt_step_row(uint32_t tile, uint32_t wave, uint32_t step) { return pt_row_of_thread(tile, pt_thread(wave, step, 0u)); }
// The row of the view's pixel (x, y) (0-based in the view)
ROMIS_HD size_t pt_row(uint32_t vw, uint32_t x, uint32_t y) {
    const uint32_t ntx = (vw + kPtTileW - 1u) / kPtTileW;
    return pt_row_of_thread((y / kPtTileH) * ntx + x / kPtTileW, (y % kPtTileH) * kPtTileW + x % kPtTileW);
}
// The index of light i's entry in `row`
ROMIS_HD size_t pt_index(size_t row, uint32_t row_floats, uint32_t light) { return row * row_floats + light; }

// The shapes the consumer kernel serves: at most 8 candidates per lane and 8 float4s of a step's rows per lane.  Other
// shapes keep the table-free kernel (an LDS-based member for them measured slower than it: profiles/phat_table/forms.json)
ROMIS_HD bool pt_fast(uint32_t num_lights, uint32_t M) {
    return M >= 1u && M <= 8u * kPtLanesPerPx && num_lights >= 1u && pt_row_floats(num_lights) <= 128u;
}
// Dynamic LDS of the consumer kernel: per wave kPtStepPx rows
ROMIS_HD size_t pt_lds_bytes(uint32_t num_lights) { return (size_t)4u * kPtStepPx * pt_row_floats(num_lights) * 4u; }

}  // namespace romis

#if defined(__HIPCC__)
#include "restir_types.h"

namespace romis {

// The table of one build: what the entries were computed from (the scene words, the view's region with its tile
// order, the G-buffer planes and the tile flags) and the entries, pt_size(view, L) floats.
struct PhatTableDev {
    SceneDev s;
    Region rg;
    FeaturesDev f;
    float origin[3];
    const float4* n_t;
    const float4* p_mat;
    const uint8_t* tmiss;   // the RIS tile flags (null: every tile is live)
    float* tab;
};
hipError_t launch_phat_table(const PhatTableDev& d, hipStream_t stream);
// Per pixel of the view (row-major): the stored p-hat of light `light` (< L); -1 where the table holds none -- a pixel of
// a background tile, or one whose candidate loop's result is known
hipError_t launch_debug_phat(const PhatTableDev& d, uint32_t light, float* out, hipStream_t stream);

}  // namespace romis
#endif
