// launch_shape.h -- the constants the kernels (kernels.hip, mis.hip) and the host's kernel choice (route.h) share: tile
// and block sizes, the lean spatial kernels' domain and LDS layout, the handle fields, the RIS light-table forms.
#pragma once

#include "restir_types.h"

namespace romis {

constexpr uint32_t kBlock = 256;
constexpr size_t kLdsBudget = 64 * 1024;   // LDS a kernel may stage a BVH / light table into
inline size_t bvh_lds_bytes(const SceneDev& s) { return ((size_t)2 * s.num_nodes + (size_t)3 * s.num_tris) * 16; }

// Work mapping.  Tiles of 32x8 pixels, one 256-lane block each (a wave = 32x2 pixels).
constexpr uint32_t kTileW = 32, kTileH = 8;
static_assert(kTileW * kTileH == kBlock, "one lane per tile pixel");

// The RIS light-table forms (kernels.hip ris_pixel's LT) and the float4s per light of each
constexpr int kLtGeneral = 0, kLtPoint = 1, kLtGrid = 2, kLtPgram = 3, kLtRegular = 4;
constexpr uint32_t lt_stride(int lt) {
    return lt == kLtGeneral ? 7u : lt == kLtPgram ? 4u : lt == kLtRegular ? 1u : 2u;
}

// The lean N = 1 / 2 spatial passes: K <= kLeanK neighbours, and for the biased ones, which stage the tile's
// neighbourhood window in LDS, R <= kLdsSpatialR.
constexpr uint32_t kLeanK = 5;
constexpr uint32_t kLdsSpatialR = 10;
constexpr uint32_t kApronMax = (kTileW + 2u * kLdsSpatialR) * (kTileH + 2u * kLdsSpatialR);   // 1456 px
// TH: tile height in 8-row units (blocks of 256 TH threads, a (32 + 2R) x (8 TH + 2R) window).
constexpr uint32_t apron_max(uint32_t TH) { return (kTileW + 2u * kLdsSpatialR) * (kTileH * TH + 2u * kLdsSpatialR); }
// LDS of a handle block: the n_t window, the two handle windows, then the light table (2 (L + 1) float4)
constexpr uint32_t h_lds_f4(uint32_t TH) { return apron_max(TH) + apron_max(TH) / 2u; }
// LDS of the fused kernel's ray phase, in float4 behind the staged BVH: s_from and s_to (512 rays), s_vis (512 words),
// the 256 bin counts, the four wave totals of their scan
constexpr uint32_t kFinRays = 512u;
constexpr uint32_t kFinLdsF4 = 2u * kFinRays + kFinRays / 4u + 256u / 4u + 1u;

// The M field of a sample handle: point lights M | light index << 24, a light grid M | light index << 19
constexpr uint32_t kHandleM = 0x00FFFFFFu;
constexpr uint32_t kHandleMG = 0x0007FFFFu;

}  // namespace romis
