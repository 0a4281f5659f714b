// shadow_lists.hip -- k_shadow_lists: the shadow-ray candidate lists of a still view (shadow_lists.h has the test and
// DESIGN.md §6 "Shadow lists" the reasoning), and the debug kernel that compares a ray traced over its list with the
// BVH walk.  Compiled with -ffp-contract=off like every other kernel, so the records are sl_record's on the host.
//
// One block of 128 threads per 32 x 16 tile of the fused pass: C2's 128 lights fill both waves (with 256 threads, one per
// record, the third wave ran the zero sample's record on a single lane and the fourth nothing).  Thread t first reduces
// four of the tile's 512 pixels into the box of the tile's hit points and prepares triangles t, t + 128 (their vertices
// and intervals on the test's axes, 128 bytes each) in LDS; then it builds records t, t + 128, .. of the tile's L lights
// by running sl_record over the triangles, which every lane reads from LDS at the same address.  Record L, the zero
// sample's, says "walk the BVH" for every tile that has hit points: a lane holds that sample and still needs a ray only
// when its shade is NaN, and the walk is right by definition.  Nothing is shared between the records, so the only
// barrier is the one that publishes the triangles and the box.  Every index is in range: pixels by the rect test,
// triangles and records by their loops' bounds (num_tris <= 256 for the LDS array and the one-byte indices, refused by
// launch_shadow_lists otherwise).
#include "kernels_common.h"
#include "shadow_lists.h"

namespace romis {
namespace {

// the flag of the 32 x 8 RIS tile holding view pixel (x, y) (kernels.hip tile_flag_at)
__device__ __forceinline__ bool background_pixel(const MissTiles& mt, const Region& rg, uint32_t x, uint32_t y) {
    if (!mt.m) return false;
    const uint32_t ntxv = (rg.vw + kTileW - 1u) / kTileW;
    return mt.flags[((y - rg.vy0) / kTileH) * ntxv + (x - rg.vx0) / kTileW] == 0u;
}
__device__ __forceinline__ bool miss_material(const SceneDev& s, float4 pm) {
    return min(__float_as_uint(pm.w), s.num_materials - 1u) == s.num_materials - 1u;   // make_px's clamp
}
__device__ __forceinline__ float wave_min(float v) {
    for (int d = 32; d; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}

constexpr uint32_t kSlThreads = 128u;
__global__ __launch_bounds__(kSlThreads) void k_shadow_lists(ShadowListsDev d) {
    __shared__ SlTri s_tri[kSlMaxTris];
    __shared__ float s_box[2][7];   // per wave: -lo, hi (as minima of the negated values), the bad flag
    const SceneDev& s = d.s;
    const Region& rg = d.rg;
    const uint32_t t = threadIdx.x, L = s.num_lights;
    const uint32_t ntx = (rg.rw + kSlTileW - 1u) / kSlTileW;
    const uint32_t tile = blockIdx.x, tx0 = rg.rx0 + (tile % ntx) * kSlTileW, ty0 = rg.ry0 + (tile / ntx) * kSlTileH;

    SlBox root;
    for (int a = 0; a < 3; a++) root.lo[a] = root.hi[a] = 0.0f;
    if (s.num_nodes) {
        const float4 lo = s.nodes[0], hi = s.nodes[1];
        root.lo[0] = lo.x; root.lo[1] = lo.y; root.lo[2] = lo.z;
        root.hi[0] = hi.x; root.hi[1] = hi.y; root.hi[2] = hi.z;
    }
    const float m = sl_margin(root);
    for (uint32_t k = t; k < s.num_tris; k += kSlThreads)
        s_tri[k] = sl_tri(reinterpret_cast<const float*>(s.tri_v0), reinterpret_cast<const float*>(s.tri_e1),
                          reinterpret_cast<const float*>(s.tri_e2), k, m);

    // the box of the tile's hit points: min over (-x, x) pairs, so one reduction serves both ends
    float v[6] = {ROMIS_FLT_MAX, ROMIS_FLT_MAX, ROMIS_FLT_MAX, ROMIS_FLT_MAX, ROMIS_FLT_MAX, ROMIS_FLT_MAX};
    float bad = 1.0f;   // 0 once a hit point is not finite
    for (uint32_t h = 0; h < 4u; h++) {
        const uint32_t x = tx0 + (t & 31u), y = ty0 + (t >> 5) + 4u * h;
        if (x < rg.rx0 + rg.rw && y < rg.ry0 + rg.rh && !background_pixel(d.mt, rg, x, y)) {
            const float4 pm = d.p_mat[(size_t)(y - rg.vy0) * rg.vw + (x - rg.vx0)];
            if (!miss_material(s, pm)) {
                if (!(sl_finite(pm.x) && sl_finite(pm.y) && sl_finite(pm.z))) bad = 0.0f;
                v[0] = fminf(v[0], -pm.x); v[1] = fminf(v[1], -pm.y); v[2] = fminf(v[2], -pm.z);
                v[3] = fminf(v[3], pm.x); v[4] = fminf(v[4], pm.y); v[5] = fminf(v[5], pm.z);
            }
        }
    }
    for (int a = 0; a < 6; a++) v[a] = wave_min(v[a]);
    bad = wave_min(bad);
    if ((t & 63u) == 0u) {
        for (int a = 0; a < 6; a++) s_box[t >> 6][a] = v[a];
        s_box[t >> 6][6] = bad;
    }
    __syncthreads();
    for (int a = 0; a < 6; a++) v[a] = fminf(s_box[0][a], s_box[1][a]);
    bad = fminf(s_box[0][6], s_box[1][6]);
    SlBox T;
    for (int a = 0; a < 3; a++) { T.lo[a] = v[3 + a]; T.hi[a] = -v[a]; }
    const bool is_bad = bad == 0.0f;
    const bool empty = !is_bad && (T.lo[0] > T.hi[0] || T.lo[1] > T.hi[1] || T.lo[2] > T.hi[2]);
    uint4* const rec = d.rec + (size_t)tile * sl_stride(L);
    const SlTile tl = sl_tile(T, m);
    for (uint32_t i = t; i < L; i += kSlThreads) {
        const float4 p = s.light_c2[i];
        const float y[3] = {p.x, p.y, p.z};
        const SlRecord r = sl_record(tl, empty, is_bad, y, s_tri, s.num_tris, d.cap);
        rec[i] = make_uint4((uint32_t)r.lo, (uint32_t)(r.lo >> 32), (uint32_t)r.hi, (uint32_t)(r.hi >> 32));
    }
    if (t == 0u) rec[L] = make_uint4(empty ? 0u : kSlWalk, 0u, 0u, 0u);   // the zero sample's
}

__global__ __launch_bounds__(256) void k_debug_shadow_lists(ShadowListsDev d, uint32_t light, uint8_t* out_bvh, uint8_t* out_list) {
    const SceneDev& s = d.s;
    const Region& rg = d.rg;
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x & 31u), y = blockIdx.y * kTileH + (threadIdx.x >> 5);
    if (x >= rg.rw || y >= rg.rh) return;
    const size_t o = (size_t)y * rg.rw + x;
    const uint32_t gx = rg.rx0 + x, gy = rg.ry0 + y, L = s.num_lights;
    if (background_pixel(d.mt, rg, gx, gy)) {
        out_bvh[o] = 0xFFu; out_list[o] = 0xFFu;
        return;
    }
    const float4 pm = d.p_mat[(size_t)(gy - rg.vy0) * rg.vw + (gx - rg.vx0)];
    const v3 P = mk(pm.x, pm.y, pm.z);
    const v3 yl = light < L ? xyz(s.light_c2[light]) : mk(0.0f, 0.0f, 0.0f);
    const uint32_t ntx = (rg.rw + kSlTileW - 1u) / kSlTileW, tile = (y / kSlTileH) * ntx + x / kSlTileW;
    const Bvh b = global_bvh(s);
    out_bvh[o] = visible(b, P, yl) ? 1u : 0u;
    out_list[o] = visible_listed(b, s.num_tris, d.rec[(size_t)tile * sl_stride(L) + light], miss_material(s, pm), P, yl) ? 1u : 0u;
}

}  // namespace

hipError_t launch_shadow_lists(const ShadowListsDev& d, hipStream_t stream) {
    const uint32_t tiles = shadow_list_tiles(d.rg);
    // the triangles' LDS array and one-byte indices
    if (d.s.num_tris > kSlMaxTris || d.cap < 1u || d.cap > kSlCap) return hipErrorInvalidValue;
    if (!tiles) return hipSuccess;
    hipLaunchKernelGGL(k_shadow_lists, dim3(tiles), dim3(kSlThreads), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_debug_shadow_lists(const ShadowListsDev& d, uint32_t light, uint8_t* out_bvh, uint8_t* out_list,
                                     hipStream_t stream) {
    if (!d.rg.rw || !d.rg.rh) return hipSuccess;
    hipLaunchKernelGGL(k_debug_shadow_lists, dim3((d.rg.rw + kTileW - 1u) / kTileW, (d.rg.rh + kTileH - 1u) / kTileH), dim3(256), 0,
                       stream, d, light, out_bvh, out_list);
    return hipGetLastError();
}

}  // namespace romis
