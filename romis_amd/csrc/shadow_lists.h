// shadow_lists.h -- candidate triangles of the fused last pass's shadow rays, per 32 x 16 tile and point light
// (DESIGN.md §6 "Shadow lists").  Which triangles can block a segment from any hit point of a tile to light i depends
// on the scene upload, the kept G-buffer and the light table alone, so the lists are built once per still view and
// light set (shadow_lists.hip k_shadow_lists) and every later frame's ray tests its list instead of walking the BVH.
// Nothing here stores an answer: a ray is still traced with tri_any, over fewer triangles, and any-hit does not depend
// on the order or on extra candidates -- a list that holds every triangle the ray can hit gives visible()'s result.
//
// One text for the host (tests/cpp/shadow_lists_check.cpp) and the kernel.
#pragma once

#include <math.h>
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

constexpr uint32_t kSlTileW = 32u, kSlTileH = 16u;   // the fused pass's tile (lean_tile<2>)
constexpr uint32_t kSlMaxTris = 256u;                // one-byte indices into the traversal arrays
constexpr uint32_t kSlCap = 15u;                     // indices a record holds
constexpr uint32_t kSlWalk = 255u;                   // the count byte of a record that says "walk the BVH"
// Records per tile: lights 0 .. L - 1 and the zero sample (L), whose record walks the BVH (shadow_lists.hip)
constexpr uint32_t sl_stride(uint32_t num_lights) { return num_lights + 1u; }

// A 16-byte record, little-endian: byte 0 the count (0 .. kSlCap, or kSlWalk), bytes 1 .. 15 the indices.
struct SlRecord { uint64_t lo, hi; };
ROMIS_HD uint32_t sl_count(const SlRecord& r) { return (uint32_t)(r.lo & 0xFFu); }
ROMIS_HD uint32_t sl_index(const SlRecord& r, uint32_t k) {   // k < count
    return (uint32_t)((k < 7u ? r.lo >> (8u * k + 8u) : r.hi >> (8u * (k - 7u))) & 0xFFu);
}

struct SlBox { float lo[3], hi[3]; };

ROMIS_HD bool sl_finite(float v) { return fabsf(v) <= 3.402823466e+38F; }   // false for NaN

// The margin every box is padded by.  The family tested below is exact geometry; what it must cover is the ray
// visible() really traces -- P2 = P + 1e-3 dir and P2 + t dir with a rounded unit dir, each a few ulp (2^-23 of the
// coordinates) off the segment P -> y over the scene's extent -- the triangles tri_any accepts although the exact ray
// passes them by a few ulp of their size, and the rounding of the sweep's own interval ends (a quotient c / a moves a
// point by 2^-24 |c|, c a difference of scene coordinates).  All of these are below 1e-6 of the larger of the scene's
// extent and its distance from the origin; the margin is 1e-5 of that figure, the one build_bvh pads its boxes by and
// tile_triangles takes, applied to both the tile box and the triangle's box: more than ten times the rounding, and
// at 1080p some hundred times below a pixel's footprint, so the lists stay short.
ROMIS_HD float sl_margin(const SlBox& root) {
    float s = 0.0f;
    for (int a = 0; a < 3; a++) s = fmaxf(s, fmaxf(root.hi[a] - root.lo[a], fmaxf(fabsf(root.lo[a]), fabsf(root.hi[a]))));
    return 1e-5f * s + 1e-30f;
}

// The axes the sweep is tested on: the coordinate axes, the six face diagonals (a box or triangle turned about one
// axis has a fat coordinate box and a thin diagonal one) and, per triangle, its normal.  Components -1, 0, 1.
constexpr int kSlAxes = 9;
ROMIS_HD float sl_axis(int u, int a) {
    // (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,-1,0) (1,0,1) (1,0,-1) (0,1,1) (0,1,-1)
    const int t[kSlAxes] = {0x001, 0x010, 0x100, 0x011, 0x031, 0x101, 0x301, 0x110, 0x310};   // nibble a: 1 -> +1, 3 -> -1
    const int c = (t[u] >> (4 * a)) & 3;
    return c == 1 ? 1.0f : c == 3 ? -1.0f : 0.0f;
}
// A point's coordinate on axis u, and a box's interval there
ROMIS_HD float sl_project(int u, const float* p) { return (sl_axis(u, 0) * p[0] + sl_axis(u, 1) * p[1]) + sl_axis(u, 2) * p[2]; }
ROMIS_HD void sl_project_box(const float* n, const SlBox& b, float& lo, float& hi) {
    lo = hi = 0.0f;
    for (int a = 0; a < 3; a++) {
        lo += fminf(n[a] * b.lo[a], n[a] * b.hi[a]);
        hi += fmaxf(n[a] * b.lo[a], n[a] * b.hi[a]);
    }
}

// A tile's hit points: their box padded by the margin m, and its intervals on the axes
struct SlTile { SlBox box; float lo[kSlAxes], hi[kSlAxes]; float m; };
ROMIS_HD SlTile sl_tile(const SlBox& T, float m) {
    SlTile t;
    t.m = m;
    for (int a = 0; a < 3; a++) { t.box.lo[a] = T.lo[a] - m; t.box.hi[a] = T.hi[a] + m; }
    for (int u = 0; u < kSlAxes; u++) {
        const float n[3] = {sl_axis(u, 0), sl_axis(u, 1), sl_axis(u, 2)};
        sl_project_box(n, t.box, t.lo[u], t.hi[u]);
    }
    return t;
}

// Triangle k (v0, v0 + e1, v0 + e2: the operands tri_any reads, records of four floats): its intervals on the axes,
// padded by m per unit of the axis' 1-norm (a point moved by m per coordinate moves that far on the axis), and its
// plane n . x = d with the same pad pn
struct SlTri { float lo[kSlAxes], hi[kSlAxes]; float n[3], d, pn; float v[3][3]; };
ROMIS_HD SlTri sl_tri(const float* v0, const float* e1, const float* e2, uint32_t k, float m) {
    SlTri t;
    const float p[3] = {v0[4u * k], v0[4u * k + 1u], v0[4u * k + 2u]};
    const float a[3] = {e1[4u * k], e1[4u * k + 1u], e1[4u * k + 2u]}, b[3] = {e2[4u * k], e2[4u * k + 1u], e2[4u * k + 2u]};
    const float q[3] = {p[0] + a[0], p[1] + a[1], p[2] + a[2]}, r[3] = {p[0] + b[0], p[1] + b[1], p[2] + b[2]};
    for (int i = 0; i < 3; i++) { t.v[0][i] = p[i]; t.v[1][i] = q[i]; t.v[2][i] = r[i]; }
    for (int u = 0; u < kSlAxes; u++) {
        const float x = sl_project(u, p), y = sl_project(u, q), z = sl_project(u, r);
        const float pad = m * ((fabsf(sl_axis(u, 0)) + fabsf(sl_axis(u, 1))) + fabsf(sl_axis(u, 2)));
        t.lo[u] = fminf(x, fminf(y, z)) - pad;
        t.hi[u] = fmaxf(x, fmaxf(y, z)) + pad;
    }
    t.n[0] = a[1] * b[2] - b[1] * a[2];
    t.n[1] = a[2] * b[0] - b[2] * a[0];
    t.n[2] = a[0] * b[1] - b[0] * a[1];
    // the three vertices' coordinates on the normal differ by rounding alone: their interval, padded like the others
    const float x = (t.n[0] * p[0] + t.n[1] * p[1]) + t.n[2] * p[2], y = (t.n[0] * q[0] + t.n[1] * q[1]) + t.n[2] * q[2];
    const float z = (t.n[0] * r[0] + t.n[1] * r[1]) + t.n[2] * r[2];
    t.pn = m * ((fabsf(t.n[0]) + fabsf(t.n[1])) + fabsf(t.n[2]));
    t.d = fminf(x, fminf(y, z));
    t.pn += fmaxf(x, fmaxf(y, z)) - t.d;
    return t;
}

// a s <= c narrows [s0, s1]; false: no s satisfies it.  The quotient is taken only where it can move an end -- c below
// a times that end -- since most inequalities leave the interval as it is; an end left alone by the rounded product's
// verdict only keeps more.
ROMIS_HD bool sl_clip(float a, float c, float& s0, float& s1) {
    if (a > 0.0f) { if (c < a * s1) s1 = fminf(s1, c / a); }
    else if (a < 0.0f) { if (c < a * s0) s0 = fmaxf(s0, c / a); }
    else if (c < 0.0f) return false;
    return true;
}
// On one axis: at parameter s the family's points lie in (1 - s) [tlo, thi] + s y, which meets [blo, bhi] iff
// tlo + s (y - tlo) <= bhi  and  thi + s (y - thi) >= blo -- two linear inequalities in s
ROMIS_HD bool sl_clip_axis(float tlo, float thi, float y, float blo, float bhi, float& s0, float& s1) {
    return sl_clip(y - tlo, bhi - tlo, s0, s1) && sl_clip(thi - y, thi - blo, s0, s1) && !(s0 > s1);
}

// Can triangle B be met by a segment from a point of tile T's box to y?  A point of the segment X(s) = (1 - s) P + s y
// that lies in the triangle lies, on every axis, inside the triangle's interval at that one s; so the triangle is
// dropped when the s-intervals of the axes and [0, 1] have no common point.  (A NaN in B keeps it: fminf / fmaxf and
// the comparisons let NaN pass.)
ROMIS_HD bool sl_keep(const SlTile& T, const float* y, const SlTri& B) {
    float s0 = 0.0f, s1 = 1.0f;
    for (int u = 0; u < kSlAxes; u++)
        if (!sl_clip_axis(T.lo[u], T.hi[u], sl_project(u, y), B.lo[u], B.hi[u], s0, s1)) return false;
    float tlo, thi;
    sl_project_box(B.n, T.box, tlo, thi);
    const float yn = (B.n[0] * y[0] + B.n[1] * y[1]) + B.n[2] * y[2];
    if (!sl_clip_axis(tlo, thi, yn, B.d - B.pn, B.d + B.pn, s0, s1)) return false;
    // The family is a thin pyramid about the line from the tile's centre to the light; seen along that line a triangle
    // it passes by lies beyond one of the triangle's edges.  The axes edge x (y - centre) tell: they separate the two
    // triangles of a quad, whose boxes are one.  Any vector is a valid axis -- the intervals are taken on the axis as
    // computed, each padded by m per unit of its 1-norm, far above the products' rounding (sl_margin).
    const float d[3] = {y[0] - 0.5f * (T.box.lo[0] + T.box.hi[0]), y[1] - 0.5f * (T.box.lo[1] + T.box.hi[1]),
                        y[2] - 0.5f * (T.box.lo[2] + T.box.hi[2])};
    for (int i = 0; i < 3; i++) {
        const float* a = B.v[i];
        const float* b = B.v[i == 2 ? 0 : i + 1];
        const float e[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const float u[3] = {e[1] * d[2] - d[1] * e[2], e[2] * d[0] - d[2] * e[0], e[0] * d[1] - d[0] * e[1]};
        sl_project_box(u, T.box, tlo, thi);
        const float yu = (u[0] * y[0] + u[1] * y[1]) + u[2] * y[2];
        const float x0 = (u[0] * B.v[0][0] + u[1] * B.v[0][1]) + u[2] * B.v[0][2];
        const float x1 = (u[0] * B.v[1][0] + u[1] * B.v[1][1]) + u[2] * B.v[1][2];
        const float x2 = (u[0] * B.v[2][0] + u[1] * B.v[2][1]) + u[2] * B.v[2][2];
        const float pad = T.m * ((fabsf(u[0]) + fabsf(u[1])) + fabsf(u[2]));
        if (!sl_clip_axis(tlo, thi, yu, fminf(x0, fminf(x1, x2)) - pad, fmaxf(x0, fmaxf(x1, x2)) + pad, s0, s1)) return false;
    }
    return true;
}

// The record of one (tile, light) pair.  T: sl_tile of the box of the tile's hit points; empty: the tile has none (no
// ray will ask); bad: one of them is not finite.  tris: the n triangles (sl_tri).  cap <= kSlCap.
// kSlWalk where the list cannot be trusted or does not fit: a non-finite tile box or light, more than cap candidates,
// or a light within 2e-3 (+ the margin) of the tile box -- a start point closer than visible()'s 1e-3 offset to the
// light puts P2 beyond the light, and the ray then runs up to 1e-3 past it, outside the family.
ROMIS_HD SlRecord sl_record(const SlTile& T, bool empty, bool bad, const float* y, const SlTri* tris, uint32_t n, uint32_t cap) {
    SlRecord r{0u, 0u};
    if (empty) return r;
    const SlRecord walk{kSlWalk, 0u};
    if (bad || n > kSlMaxTris || !sl_finite(y[0]) || !sl_finite(y[1]) || !sl_finite(y[2])) return walk;
    bool near = true;
    for (int a = 0; a < 3; a++) near = near && y[a] >= T.box.lo[a] - 2e-3f && y[a] <= T.box.hi[a] + 2e-3f;
    if (near) return walk;
    uint32_t cnt = 0u;
    for (uint32_t k = 0; k < n; k++) {
        if (!sl_keep(T, y, tris[k])) continue;
        if (cnt == cap) return walk;
        if (cnt < 7u) r.lo |= (uint64_t)k << (8u * cnt + 8u);
        else r.hi |= (uint64_t)k << (8u * (cnt - 7u));
        cnt++;
    }
    r.lo |= cnt;
    return r;
}

}  // namespace romis

#if defined(__HIPCC__)
#include "restir_types.h"

namespace romis {

// The records of one build (shadow_lists.hip): rg's rect cut into 32 x 16 tiles numbered row-major (lean_tile<2>'s
// numbering), sl_stride(L) records per tile -- light i at light_c2[i], record L the zero sample's (0, 0, 0) -- at
// rec[tile * sl_stride(L) + i].  mt: the MissTiles of the fused pass (m = 0: no flags); a pixel of a background RIS tile
// holds no G-buffer record and asks for no ray.  cap: indices per record (kSlCap; tests lower it).
struct ShadowListsDev {
    SceneDev s;
    Region rg;
    const float4* p_mat;
    MissTiles mt;
    uint32_t cap;
    uint4* rec;
};
inline uint32_t shadow_list_tiles(const Region& rg) {
    return ((rg.rw + kSlTileW - 1u) / kSlTileW) * ((rg.rh + kSlTileH - 1u) / kSlTileH);
}
hipError_t launch_shadow_lists(const ShadowListsDev& d, hipStream_t stream);
// Per pixel of rg's rect (row-major, one byte each): visible() from the pixel's p_mat to light `light` (<= L) by the BVH
// walk and by the record, 0 / 1; 0xFF in both for a pixel of a background RIS tile.
hipError_t launch_debug_shadow_lists(const ShadowListsDev& d, uint32_t light, uint8_t* out_bvh, uint8_t* out_list,
                                     hipStream_t stream);

}  // namespace romis
#endif
