// shadow_vis.hip -- k_shadow_vis: the visibility bits of a still view (shadow_vis.h has the layout, DESIGN.md §6
// "Visibility bits" the reasoning), and the debug kernel that unpacks one light's bits.  Compiled with
// -ffp-contract=off like every other kernel: visible_listed() here is the frame kernel's.
//
// One block of 512 threads per 32 x 16 tile of the fused pass, thread t at the pixel the frame kernel's thread t holds
// (shadow_vis.h).  The block loops over the tile's L lights: record rec[tile][i] and light i are the same for all its
// lanes, so a list's length does not diverge within a wave and a "walk the BVH" record walks for the whole wave; each
// lane asks visible_listed(bvh, num_tris, rec[i], false, xyz(p_mat[pix]), light_c2[i]) -- the frame kernel's call for a
// pixel that does not hold the miss material -- and shifts the answer into the word it stores after every 32nd light.
// No atomics, no barrier: a lane writes only its own words.  A lane whose pixel the frame kernel never asks about --
// outside the rect, in a background RIS tile, or with the miss material (the frame kernel tests every triangle there,
// the record's `outside` case) -- traces nothing and stores zeros.  Every index is in range: the pixel by the rect test,
// the records by the loop's bound, the words by sv_size.
#include "kernels_common.h"
#include "shadow_vis.h"

namespace romis {
namespace {

// (shadow_lists.hip's, kernels.hip tile_flag_at / make_px's clamp)
__device__ __forceinline__ bool sv_background_pixel(const MissTiles& mt, const Region& rg, uint32_t x, uint32_t y) {
    if (!mt.m) return false;
    const uint32_t ntxv = (rg.vw + kTileW - 1u) / kTileW;
    return mt.flags[((y - rg.vy0) / kTileH) * ntxv + (x - rg.vx0) / kTileW] == 0u;
}
__device__ __forceinline__ bool sv_miss_material(const SceneDev& s, float4 pm) {
    return min(__float_as_uint(pm.w), s.num_materials - 1u) == s.num_materials - 1u;
}
// does the plane hold bits for view pixel (x, y) of the rect?  pm: its p_mat record when it does
__device__ __forceinline__ bool sv_held(const ShadowListsDev& d, uint32_t x, uint32_t y, float4& pm) {
    const Region& rg = d.rg;
    if (x >= rg.rx0 + rg.rw || y >= rg.ry0 + rg.rh || sv_background_pixel(d.mt, rg, x, y)) return false;
    pm = d.p_mat[(size_t)(y - rg.vy0) * rg.vw + (x - rg.vx0)];
    return !sv_miss_material(d.s, pm);
}

__global__ __launch_bounds__(kSvTilePx) void k_shadow_vis(ShadowVisDev v) {
    const ShadowListsDev& d = v.lists;
    const SceneDev& s = d.s;
    const Region& rg = d.rg;
    const uint32_t t = threadIdx.x, L = s.num_lights, words = sv_words(L);
    const uint32_t ntx = (rg.rw + kSvTileW - 1u) / kSvTileW;
    const uint32_t tile = blockIdx.x, w = t >> 6, l = t & 63u;
    const uint32_t x = rg.rx0 + (tile % ntx) * kSvTileW + (w & 3u) * 8u + (l & 7u);
    const uint32_t y = rg.ry0 + (tile / ntx) * kSvTileH + (w >> 2) * 8u + (l >> 3);
    float4 pm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool held = sv_held(d, x, y, pm);
    const v3 P = mk(pm.x, pm.y, pm.z);
    const Bvh bvh = global_bvh(s);
    const uint4* const rec = d.rec + (size_t)tile * sl_stride(L);
    uint32_t* const out = v.bits + sv_index(sv_slot_of_thread(tile, t), words, 0u);
    uint32_t acc = 0u;
    for (uint32_t i = 0; i < L; i++) {
        if (held && visible_listed(bvh, s.num_tris, rec[i], false, P, xyz(s.light_c2[i]))) acc |= sv_bit(i);
        if ((i & 31u) == 31u || i + 1u == L) {
            out[sv_word_of(i)] = acc;
            acc = 0u;
        }
    }
}

__global__ __launch_bounds__(256) void k_debug_shadow_vis(ShadowVisDev v, uint32_t light, uint8_t* out) {
    const ShadowListsDev& d = v.lists;
    const Region& rg = d.rg;
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x & 31u), y = blockIdx.y * kTileH + (threadIdx.x >> 5);
    if (x >= rg.rw || y >= rg.rh) return;
    float4 pm;
    uint8_t r = 0xFFu;
    if (sv_held(d, rg.rx0 + x, rg.ry0 + y, pm)) {
        const uint32_t word = v.bits[sv_index(sv_slot(rg.rw, x, y), sv_words(d.s.num_lights), sv_word_of(light))];
        r = (word & sv_bit(light)) ? 1u : 0u;
    }
    out[(size_t)y * rg.rw + x] = r;
}

}  // namespace

hipError_t launch_shadow_vis(const ShadowVisDev& d, hipStream_t stream) {
    const uint32_t tiles = sv_tiles(d.lists.rg.rw, d.lists.rg.rh);
    const uint32_t words = sv_words(d.lists.s.num_lights);
    if (d.lists.s.num_tris > kSlMaxTris || !words || words > kSvMaxWords || !d.bits || !d.lists.rec) return hipErrorInvalidValue;
    if (!tiles) return hipSuccess;
    hipLaunchKernelGGL(k_shadow_vis, dim3(tiles), dim3(kSvTilePx), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_debug_shadow_vis(const ShadowVisDev& d, uint32_t light, uint8_t* out, hipStream_t stream) {
    const Region& rg = d.lists.rg;
    if (light >= d.lists.s.num_lights) return hipErrorInvalidValue;
    if (!rg.rw || !rg.rh) return hipSuccess;
    hipLaunchKernelGGL(k_debug_shadow_vis, dim3((rg.rw + kTileW - 1u) / kTileW, (rg.rh + kTileH - 1u) / kTileH), dim3(256), 0, stream,
                       d, light, out);
    return hipGetLastError();
}

}  // namespace romis
