// bvh_check -- host checks of csrc/bvh.cpp (build_bvh, quantize_nodes): the flattened tree's invariants, and the
// pruning of the device's ray walks against brute force.  tests/test_bvh_invariants.py writes the triangle files
// (uint32 count, then 9 floats per triangle: v0, v1, v2) and reads the lines printed here.  No device code.
//
//   bvh_check [--rays N] file...        (N = 0: the invariants alone)
//
// THE RAY PART RESTATES DEVICE FUNCTIONS of csrc/kernels_common.h -- keep them in step when one changes:
//   safe_inv, widen, box_hit                 -> safe_inv, widen, box_hit below
//   tri_any / tri_test (one set of float expressions) -> tri_exact
//   occluded    (the walk over the 32-byte nodes)     -> walk_float: the leaves it would test, without the early return
//   occluded_q  (the 16-byte nodes, fma slabs)        -> walk_quantized
//   closest     (widen(t_best), the tie rule)         -> closest_walk
//   visible / visible_q (P2 = P + 1e-3 dir, tfar)     -> make_ray
// and of csrc/restir.cpp restir_set_scene: the traversal arrays v0, e1 = v1 - v0, e2 = v2 - v0 in BVH order.
// What must hold: the triangles of the leaves a walk accepts contain every triangle the exact test hits (so any-hit and
// closest-hit over them equal brute force over all triangles), for the float boxes and for the quantized ones.
//
// That argument is about triangles with an area.  For three collinear vertices det = e1 . (d x e2) is the rounding error
// of a zero, so u, v and t are quotients of rounding errors: the exact test then reports "hits" at distances that have
// nothing to do with where the triangle lies, and no box around the triangle can promise to contain them (found here:
// 48 such triangles, ray 16911 of the set below -- brute force t = 0.41666669 on triangle 36, the walk's closest hit
// t = 0.51416016 on triangle 25).  Such inputs get the invariants alone (--rays 0).  Triangles whose det is an exact
// zero -- three equal vertices, collinear vertices along an axis -- are never hit and are part of the ray inputs.
#include "bvh.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

using namespace romis;

namespace {

std::atomic<int> g_fail{0};
std::string g_where;

#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (g_fail < 40) {                                            \
                std::printf("FAIL %s: ", g_where.c_str());                \
                std::printf(__VA_ARGS__);                                 \
                std::printf("  [%s]\n", #cond);                           \
            }                                                             \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct V3 { float x, y, z; };
V3 mk(float x, float y, float z) { return {x, y, z}; }
V3 vadd(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
V3 vsub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
V3 vscale(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
float vdot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
V3 vcross(V3 x, V3 y) { return mk(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y); }
V3 vnormalize(V3 a) { return vscale(a, 1.0f / std::sqrt(vdot(a, a))); }
float comp(V3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }

// ---- the device functions restated ---------------------------------------------------------------------------
V3 safe_inv(V3 d) {
    return mk(1.0f / (d.x == 0.0f ? std::copysign(1e-30f, d.x) : d.x), 1.0f / (d.y == 0.0f ? std::copysign(1e-30f, d.y) : d.y),
              1.0f / (d.z == 0.0f ? std::copysign(1e-30f, d.z) : d.z));
}
float widen(float t) { return t * 1.0001f + 1e-4f; }

bool slabs(float tx0, float tx1, float ty0, float ty1, float tz0, float tz1, float tmax_box) {
    const float tmin = std::fmax(std::fmax(std::fmin(tx0, tx1), std::fmin(ty0, ty1)), std::fmax(std::fmin(tz0, tz1), 0.0f));
    const float tmax = std::fmin(std::fmin(std::fmax(tx0, tx1), std::fmax(ty0, ty1)), std::fmin(std::fmax(tz0, tz1), tmax_box));
    return tmin <= tmax;
}
bool box_hit(const float* lo, const float* hi, V3 o, V3 invd, float tmax_box) {
    return slabs((lo[0] - o.x) * invd.x, (hi[0] - o.x) * invd.x, (lo[1] - o.y) * invd.y, (hi[1] - o.y) * invd.y,
                 (lo[2] - o.z) * invd.z, (hi[2] - o.z) * invd.z, tmax_box);
}

struct Tri { V3 v0, e1, e2; uint32_t orig; };

bool tri_exact(const Tri& tr, V3 o, V3 d, float tfar, float& t) {
    const V3 pvec = vcross(d, tr.e2);
    const float det = vdot(tr.e1, pvec);
    const float inv = 1.0f / det;
    const V3 tvec = vsub(o, tr.v0);
    const float u = vdot(tvec, pvec) * inv;
    const V3 qvec = vcross(tvec, tr.e1);
    const float v = vdot(d, qvec) * inv;
    t = vdot(tr.e2, qvec) * inv;
    return det != 0.0f && (u >= 0.0f && u <= 1.0f) && (v >= 0.0f && u + v <= 1.0f) && (t > 0.0f && t <= tfar);
}

struct Tree {
    FlatBvh bvh;
    QuantizedNodes q;
    std::vector<Tri> tris;   // BVH order
};

// occluded without the early return: marks every triangle of every leaf whose box the walk accepts
void walk_float(const Tree& tr, V3 o, V3 d, float tfar, std::vector<uint8_t>& mark) {
    const V3 invd = safe_inv(d);
    const float tb = widen(tfar);
    uint32_t i = 0;
    while (i < tr.bvh.num_nodes) {
        const float* n = &tr.bvh.nodes[8 * i];
        const uint32_t miss = f2u(n[3]), leaf = f2u(n[7]);
        if (box_hit(n, n + 4, o, invd, tb)) {
            if (leaf) {
                for (uint32_t k = 0; k < (leaf >> 24); k++) mark[(leaf & 0xFFFFFFu) + k] = 1;
                i = miss;
            } else {
                i = i + 1;
            }
        } else {
            i = miss;
        }
    }
}

void walk_quantized(const Tree& tr, V3 o, V3 d, float tfar, std::vector<uint8_t>& mark) {
    const V3 invd = safe_inv(d);
    const float tb = widen(tfar);
    const float* s = tr.q.s;
    const float* lo = tr.q.lo;
    const V3 A = mk(s[0] * invd.x, s[1] * invd.y, s[2] * invd.z);
    const V3 C = mk((lo[0] - o.x) * invd.x, (lo[1] - o.y) * invd.y, (lo[2] - o.z) * invd.z);
    uint32_t i = 0;
    while (i < tr.bvh.num_nodes) {
        const uint32_t* n = &tr.q.words[4 * i];
        const float tx0 = std::fmaf((float)(n[0] & 0xFFFFu), A.x, C.x), tx1 = std::fmaf((float)(n[1] >> 16), A.x, C.x);
        const float ty0 = std::fmaf((float)(n[0] >> 16), A.y, C.y), ty1 = std::fmaf((float)(n[2] & 0xFFFFu), A.y, C.y);
        const float tz0 = std::fmaf((float)(n[1] & 0xFFFFu), A.z, C.z), tz1 = std::fmaf((float)(n[2] >> 16), A.z, C.z);
        const uint32_t cnt = n[3] >> 28, miss = n[3] & 0xFFFFu;
        if (slabs(tx0, tx1, ty0, ty1, tz0, tz1, tb)) {
            if (cnt) {
                for (uint32_t k = 0; k < cnt; k++) mark[((n[3] >> 16) & 0xFFFu) + k] = 1;
                i = miss;
            } else {
                i = i + 1;
            }
        } else {
            i = miss;
        }
    }
}

bool closest_walk(const Tree& tr, V3 o, V3 d, float& t_best, uint32_t& tri_best) {
    const V3 invd = safe_inv(d);
    bool found = false;
    t_best = FLT_MAX;
    tri_best = 0xFFFFFFFFu;
    uint32_t i = 0;
    while (i < tr.bvh.num_nodes) {
        const float* n = &tr.bvh.nodes[8 * i];
        const uint32_t miss = f2u(n[3]), leaf = f2u(n[7]);
        if (box_hit(n, n + 4, o, invd, widen(t_best))) {
            if (leaf) {
                for (uint32_t k = 0; k < (leaf >> 24); k++) {
                    const Tri& t3 = tr.tris[(leaf & 0xFFFFFFu) + k];
                    float t;
                    const bool h = tri_exact(t3, o, d, FLT_MAX, t);
                    if (h && (!found || t < t_best || (t == t_best && t3.orig < tri_best))) {
                        found = true; t_best = t; tri_best = t3.orig;
                    }
                }
                i = miss;
            } else {
                i = i + 1;
            }
        } else {
            i = miss;
        }
    }
    return found;
}

// ---- invariants ------------------------------------------------------------------------------------------------
struct Span { float lo[3], hi[3]; };

// Checks the subtree at node i; returns the index after it.  cover[k]: how many leaves hold BVH-order triangle k.
uint32_t check_subtree(const Tree& tr, const std::vector<BvhTriangle>& in, uint32_t i, uint32_t clamped, float pad,
                       std::vector<uint32_t>& cover, Span& span, uint32_t depth) {
    const uint32_t n = tr.bvh.num_nodes;
    if (i >= n || depth > n) { CHECK(false, "node %u of %u at depth %u\n", i, n, depth); return n; }
    const float* o = &tr.bvh.nodes[8 * i];
    const uint32_t miss = f2u(o[3]), leaf = f2u(o[7]);
    for (int a = 0; a < 3; a++) { span.lo[a] = FLT_MAX; span.hi[a] = -FLT_MAX; }
    uint32_t end;
    if (leaf) {
        const uint32_t first = leaf & 0xFFFFFFu, cnt = leaf >> 24;
        CHECK(cnt >= 1 && cnt <= clamped, "node %u: leaf of %u triangles, max_leaf %u\n", i, cnt, clamped);
        CHECK((size_t)first + cnt <= in.size(), "node %u: leaf [%u, +%u) of %zu\n", i, first, cnt, in.size());
        for (uint32_t k = first; k < first + cnt && k < in.size(); k++) {
            cover[k]++;
            const BvhTriangle& t = in[tr.bvh.tri_order[k]];
            for (const float* v : {t.v0, t.v1, t.v2})
                for (int a = 0; a < 3; a++) { span.lo[a] = std::min(span.lo[a], v[a]); span.hi[a] = std::max(span.hi[a], v[a]); }
        }
        end = i + 1;
    } else {
        Span l, r;
        const uint32_t right = check_subtree(tr, in, i + 1, clamped, pad, cover, l, depth + 1);
        end = right < n ? check_subtree(tr, in, right, clamped, pad, cover, r, depth + 1) : n;
        CHECK(right < n, "node %u: an inner node without a right child\n", i);
        if (right < n) {
            CHECK(f2u(tr.bvh.nodes[8 * (i + 1) + 3]) == right, "node %u: the left child's miss link is not the right child %u\n", i, right);
            for (uint32_t c : {i + 1, right}) {   // a child's box lies inside its parent's
                const float* b = &tr.bvh.nodes[8 * c];
                for (int a = 0; a < 3; a++)
                    CHECK(b[a] >= o[a] && b[4 + a] <= o[4 + a], "node %u axis %d: child %u [%g, %g] outside [%g, %g]\n", i, a, c,
                          b[a], b[4 + a], o[a], o[4 + a]);
            }
            for (int a = 0; a < 3; a++) { span.lo[a] = std::min(l.lo[a], r.lo[a]); span.hi[a] = std::max(l.hi[a], r.hi[a]); }
        }
    }
    CHECK(miss > i, "node %u: miss link %u does not grow\n", i, miss);
    CHECK(miss == end, "node %u: miss link %u, the next subtree in preorder is %u\n", i, miss, end);
    for (int a = 0; a < 3; a++)
        CHECK(o[a] <= span.lo[a] - pad && o[4 + a] >= span.hi[a] + pad, "node %u axis %d: box [%g, %g], vertices [%g, %g], pad %g\n",
              i, a, o[a], o[4 + a], span.lo[a], span.hi[a], pad);
    return end;
}

bool build_and_check(const std::vector<BvhTriangle>& in, uint32_t max_leaf, Tree& tr) {
    const int before = g_fail.load();
    const uint32_t clamped = std::min(std::max(max_leaf, 1u), 255u);
    const size_t T = in.size();
    tr.bvh = build_bvh(in, max_leaf);
    tr.q = quantize_nodes(tr.bvh);
    const FlatBvh& b = tr.bvh;
    CHECK(b.tri_order.size() == T && b.nodes.size() == 8 * (size_t)b.num_nodes, "%zu order entries, %zu node floats\n",
          b.tri_order.size(), b.nodes.size());
    CHECK((T == 0) == (b.num_nodes == 0), "%zu triangles, %u nodes\n", T, b.num_nodes);
    if (g_fail != before) return false;
    std::vector<uint32_t> seen(T, 0);
    for (uint32_t k : b.tri_order) {
        CHECK(k < T, "tri_order entry %u of %zu\n", k, T);
        if (k < T) seen[k]++;
    }
    for (size_t k = 0; k < T; k++) CHECK(seen[k] == 1, "triangle %zu appears %u times in tri_order\n", k, seen[k]);
    if (g_fail != before) return false;

    tr.tris.resize(T);
    for (size_t k = 0; k < T; k++) {
        const BvhTriangle& t = in[b.tri_order[k]];
        Tri& d = tr.tris[k];
        d.v0 = mk(t.v0[0], t.v0[1], t.v0[2]);
        d.e1 = mk(t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2]);
        d.e2 = mk(t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2]);
        d.orig = b.tri_order[k];
    }
    bool structural_q = b.num_nodes > 0 && b.num_nodes < 65536u;
    if (T) {
        // the pad build_bvh applies: 1e-5 of the scene's size (the largest |coordinate| or extent of the bounds)
        Span all;
        for (int a = 0; a < 3; a++) { all.lo[a] = FLT_MAX; all.hi[a] = -FLT_MAX; }
        for (const BvhTriangle& t : in)
            for (const float* v : {t.v0, t.v1, t.v2})
                for (int a = 0; a < 3; a++) { all.lo[a] = std::min(all.lo[a], v[a]); all.hi[a] = std::max(all.hi[a], v[a]); }
        float scale = 0.0f;
        for (int a = 0; a < 3; a++) scale = std::max({scale, std::fabs(all.lo[a]), std::fabs(all.hi[a]), all.hi[a] - all.lo[a]});
        const float pad = 1e-5f * scale + 1e-30f;
        CHECK(pad > 0.0f, "pad %g\n", pad);
        std::vector<uint32_t> cover(T, 0);
        Span span;
        const uint32_t end = check_subtree(tr, in, 0, clamped, pad, cover, span, 0);
        CHECK(end == b.num_nodes, "the root's subtree ends at %u of %u nodes\n", end, b.num_nodes);
        for (size_t k = 0; k < T; k++) CHECK(cover[k] == 1, "triangle slot %zu lies in %u leaves\n", k, cover[k]);
        for (uint32_t i = 0; i < b.num_nodes; i++) {
            const uint32_t leaf = f2u(b.nodes[8 * i + 7]);
            structural_q = structural_q && (leaf == 0u || ((leaf >> 24) < 16u && (leaf & 0xFFFFFFu) + (leaf >> 24) <= 4096u));
        }
    }
    // the quantized nodes: there exactly when the fields fit (our inputs' coordinates are finite and in range)
    const QuantizedNodes& q = tr.q;
    CHECK(q.ok == structural_q, "quantized nodes ok = %d, the fields %s\n", (int)q.ok, structural_q ? "fit" : "do not fit");
    if (!q.ok) {
        CHECK(q.words.size() == 4 && !(q.words[0] | q.words[1] | q.words[2] | q.words[3]), "%zu words without quantized nodes\n",
              q.words.size());
    } else {
        CHECK(q.words.size() == 4 * (size_t)b.num_nodes, "%zu words for %u nodes\n", q.words.size(), b.num_nodes);
        for (uint32_t i = 0; i < b.num_nodes && q.words.size() == 4 * (size_t)b.num_nodes; i++) {
            const uint32_t* w = &q.words[4 * i];
            const float* o = &b.nodes[8 * i];
            const uint32_t ql[3] = {w[0] & 0xFFFFu, w[0] >> 16, w[1] & 0xFFFFu}, qh[3] = {w[1] >> 16, w[2] & 0xFFFFu, w[2] >> 16};
            for (int a = 0; a < 3; a++) {
                const double lo = (double)q.lo[a] + (double)ql[a] * (double)q.s[a], hi = (double)q.lo[a] + (double)qh[a] * (double)q.s[a];
                CHECK(lo <= (double)o[a] && hi >= (double)o[4 + a], "node %u axis %d: quantized [%.9g, %.9g] inside float [%.9g, %.9g]\n",
                      i, a, lo, hi, o[a], o[4 + a]);
            }
            const uint32_t miss = f2u(o[3]), leaf = f2u(o[7]);
            CHECK((w[3] & 0xFFFFu) == miss && ((w[3] >> 16) & 0xFFFu) == (leaf & 0xFFFFFFu) && (w[3] >> 28) == (leaf >> 24),
                  "node %u: word %08x for miss %u leaf %08x\n", i, w[3], miss, leaf);
        }
    }
    return g_fail == before;
}

// ---- rays ------------------------------------------------------------------------------------------------------
uint32_t mix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
struct Rng {
    uint32_t s;
    uint32_t next() { s += 0x9E3779B9u; return mix32(s); }
    float uni() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }   // [0, 1)
    float sym() { return 2.0f * uni() - 1.0f; }
};

struct Ray { V3 o, d; float tfar; };

// visible(): the shadow ray from P towards y
Ray make_ray(V3 P, V3 y) {
    Ray r;
    r.d = vnormalize(vsub(y, P));
    r.o = vadd(P, vscale(r.d, 1e-3f));
    const V3 e = vsub(y, r.o);
    r.tfar = std::sqrt(vdot(e, e));
    return r;
}

V3 on_triangle(const BvhTriangle& t, float a, float b) {
    if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
    V3 v0 = mk(t.v0[0], t.v0[1], t.v0[2]), v1 = mk(t.v1[0], t.v1[1], t.v1[2]), v2 = mk(t.v2[0], t.v2[1], t.v2[2]);
    return vadd(v0, vadd(vscale(vsub(v1, v0), a), vscale(vsub(v2, v0), b)));
}

enum Family { kGeneric, kOneZero, kPlumb, kCoincident, kSurface, kVertex, kEdge, kSubnormal, kNear, kFar, kNanPart, kFamilies };
const char* kFamilyName[kFamilies] = {"generic", "one_zero", "plumb", "coincident", "surface", "vertex", "edge", "subnormal",
                                      "near", "far", "nan_part"};

struct RayStats {
    uint64_t rays = 0, zero_comp = 0, nan_dir = 0, subnormal = 0, occluded = 0, clear = 0, closest_found = 0, ties = 0;
};

// rays first, first + step, ... below nrays (one thread's share: a ray depends on its index alone)
void check_rays(const std::vector<BvhTriangle>& in, const std::vector<Tree>& trees, uint32_t first, uint32_t step, uint32_t nrays,
                RayStats& st) {
    const size_t T = in.size();
    if (!T) return;
    const float* root = trees[0].bvh.nodes.data();
    V3 lo = mk(root[0], root[1], root[2]), ext = mk(root[4] - root[0], root[5] - root[1], root[6] - root[2]);
    const float size = std::max({ext.x, ext.y, ext.z, 1e-3f});
    std::vector<uint8_t> mark(T);
    std::vector<uint32_t> hits;
    std::vector<std::vector<uint32_t>> slot_of(trees.size(), std::vector<uint32_t>(T));   // per tree: original index -> BVH slot
    for (size_t ti = 0; ti < trees.size(); ti++)
        for (size_t k = 0; k < T; k++) slot_of[ti][trees[ti].tris[k].orig] = (uint32_t)k;
    std::vector<float> thit(T);
    std::vector<const Tri*> by_orig(T);
    for (const Tri& t3 : trees[0].tris) by_orig[t3.orig] = &t3;
    for (uint32_t r = first; r < nrays; r += step) {
        Rng g{mix32(r * 2654435761u + 12345u)};
        const int fam = (int)(r % kFamilies);
        // P: a point of a triangle (two rays in three), else a point in the bounds grown by a quarter
        V3 P;
        if (r % 3 != 2) P = on_triangle(in[g.next() % T], g.uni(), g.uni());
        else P = mk(lo.x + ext.x * (1.5f * g.uni() - 0.25f), lo.y + ext.y * (1.5f * g.uni() - 0.25f), lo.z + ext.z * (1.5f * g.uni() - 0.25f));
        const BvhTriangle& tt = in[g.next() % T];
        const V3 v0 = mk(tt.v0[0], tt.v0[1], tt.v0[2]);
        const V3 e12 = vadd(vsub(mk(tt.v1[0], tt.v1[1], tt.v1[2]), v0), vsub(mk(tt.v2[0], tt.v2[1], tt.v2[2]), v0));
        const float k = (g.next() & 1u ? 1.0f : -1.0f) * size * (0.05f + g.uni());
        const int axis = (int)(g.next() % 3u);
        V3 y;
        switch (fam) {
        case kOneZero:   y = vadd(P, mk(axis == 0 ? 0.0f : size * g.sym(), axis == 1 ? 0.0f : size * g.sym(), axis == 2 ? 0.0f : size * g.sym())); break;
        case kPlumb:     y = vadd(P, mk(axis == 0 ? k : 0.0f, axis == 1 ? k : 0.0f, axis == 2 ? k : 0.0f)); break;
        case kCoincident: y = P; break;
        case kSurface:   y = on_triangle(tt, g.uni(), g.uni()); break;
        case kVertex:    y = v0; break;
        case kEdge:      y = vadd(v0, vscale(e12, 0.25f)); break;
        case kSubnormal: P.x = (r & 16u) ? -0.0f : 0.0f; y = vadd(P, mk(1e-40f, k, 0.0f)); break;
        case kNear:      y = vadd(P, vscale(vnormalize(mk(g.sym(), g.sym(), g.sym())), 5e-4f)); break;
        case kFar:       y = vadd(P, vscale(vnormalize(mk(g.sym(), g.sym(), g.sym())), 1e19f)); break;
        case kNanPart:   y = mk(lo.x + ext.x * g.uni(), lo.y + ext.y * g.uni(), lo.z + ext.z * g.uni()); break;
        default:         y = mk(lo.x + ext.x * g.uni(), lo.y + ext.y * g.uni(), lo.z + ext.z * g.uni()); break;
        }
        Ray ray = make_ray(P, y);
        if (fam == kNanPart) {   // one NaN component, or a NaN tfar, on an otherwise ordinary ray
            const float nan = std::nanf("");
            if (axis == 0) ray.d.x = nan; else if (axis == 1) ray.tfar = nan; else ray.o.z = nan;
        }
        if (fam == kSubnormal) {   // the direction as given, not normalized away: a subnormal x beside a unit y
            ray.d = mk(1e-40f, k > 0.0f ? 1.0f : -1.0f, 0.0f);
            ray.o = vadd(P, vscale(ray.d, 1e-3f));
            ray.tfar = std::fabs(k);
        }
        st.rays++;
        bool zero = false, nan = false, sub = false;
        for (int c = 0; c < 3; c++) {
            const float v = comp(ray.d, c);
            zero = zero || v == 0.0f;
            nan = nan || v != v;
            sub = sub || (v != 0.0f && std::fabs(v) < FLT_MIN);
        }
        st.zero_comp += zero; st.nan_dir += nan; st.subnormal += sub;

        // brute force, over every triangle in original order (the oracle's any_hit / closest_hit): one evaluation serves
        // both, (t > 0 && t <= tfar) being (t > 0 && t <= FLT_MAX) && t <= tfar
        bool cfound = false;
        float ct = FLT_MAX;
        uint32_t ctri = 0xFFFFFFFFu, tie = 0;
        hits.clear();
        for (size_t i = 0; i < T; i++) {
            float tc;
            const bool hc = tri_exact(*by_orig[i], ray.o, ray.d, FLT_MAX, tc);
            thit[i] = hc ? tc : -1.0f;
            if (hc && tc <= ray.tfar) hits.push_back((uint32_t)i);
            if (hc && (!cfound || tc < ct)) { cfound = true; ct = tc; ctri = (uint32_t)i; }
        }
        for (size_t i = 0; cfound && i < T; i++) tie += thit[i] == ct;
        const bool any = !hits.empty();
        st.occluded += any; st.clear += !any; st.closest_found += cfound; st.ties += tie > 1;

        for (size_t ti = 0; ti < trees.size(); ti++) {
            const Tree& tr = trees[ti];
            for (int quantized = 0; quantized < 2 && any; quantized++) {
                if (quantized && !tr.q.ok) continue;
                std::fill(mark.begin(), mark.end(), 0);
                if (quantized) walk_quantized(tr, ray.o, ray.d, ray.tfar, mark); else walk_float(tr, ray.o, ray.d, ray.tfar, mark);
                for (uint32_t h : hits)
                    CHECK(mark[slot_of[ti][h]],
                          "ray %u (%s) o (%.9g, %.9g, %.9g) d (%.9g, %.9g, %.9g) tfar %.9g: the %s walk prunes triangle %u, which it hits\n",
                          r, kFamilyName[fam], ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, ray.tfar,
                          quantized ? "quantized" : "float", h);
            }
            float wt;
            uint32_t wtri;
            const bool wf = closest_walk(tr, ray.o, ray.d, wt, wtri);
            CHECK(wf == cfound && (!wf || (f2u(wt) == f2u(ct) && wtri == ctri)),
                  "ray %u (%s) o (%.9g, %.9g, %.9g) d (%.9g, %.9g, %.9g): closest walk %d t %.9g tri %u, brute force %d t %.9g tri %u\n",
                  r, kFamilyName[fam], ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, (int)wf, wt, wtri, (int)cfound, ct, ctri);
        }
    }
}

bool read_triangles(const char* path, std::vector<BvhTriangle>& out) {
    FILE* fh = std::fopen(path, "rb");
    if (!fh) return false;
    uint32_t n = 0;
    bool ok = std::fread(&n, 4, 1, fh) == 1 && n < (1u << 24);
    if (ok) {
        out.resize(n);
        static_assert(sizeof(BvhTriangle) == 36, "nine floats");
        ok = n == 0 || std::fread(out.data(), sizeof(BvhTriangle), n, fh) == n;
    }
    std::fclose(fh);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t leaves[] = {1, 2, 3, 5, 15, 16, 255, 0, 1000};
    const uint32_t ray_leaves[] = {2, 3, 15, 16};
    uint32_t nrays = 100000;
    int first = 1;
    if (argc > 2 && !std::strcmp(argv[1], "--rays")) { nrays = (uint32_t)std::strtoul(argv[2], nullptr, 10); first = 3; }
    if (first >= argc) { std::fprintf(stderr, "usage: bvh_check [--rays N] file...\n"); return 2; }
    for (int a = first; a < argc; a++) {
        std::vector<BvhTriangle> in;
        const char* base = std::strrchr(argv[a], '/');
        base = base ? base + 1 : argv[a];
        if (!read_triangles(argv[a], in)) { std::printf("FAIL %s: cannot read\n", base); g_fail++; continue; }
        std::vector<Tree> ray_trees;
        for (uint32_t ml : leaves) {
            g_where = std::string(base) + " max_leaf " + std::to_string(ml);
            Tree tr;
            const bool ok = build_and_check(in, ml, tr);
            uint32_t largest = 0;
            for (uint32_t i = 0; i < tr.bvh.num_nodes; i++) largest = std::max(largest, f2u(tr.bvh.nodes[8 * i + 7]) >> 24);
            std::printf("tree %s max_leaf %u triangles %zu nodes %u depth %u largest_leaf %u q_ok %d %s\n", base, ml, in.size(),
                        tr.bvh.num_nodes, tr.bvh.max_depth, largest, (int)tr.q.ok, ok ? "ok" : "BAD");
            if (ok && std::find(std::begin(ray_leaves), std::end(ray_leaves), ml) != std::end(ray_leaves)) ray_trees.push_back(std::move(tr));
        }
        if (nrays && ray_trees.size() == sizeof(ray_leaves) / sizeof(ray_leaves[0]) && !in.empty()) {
            g_where = std::string(base) + " rays";
            const int before = g_fail.load();
            const uint32_t nthreads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
            std::vector<RayStats> part(nthreads);
            std::vector<std::thread> pool;
            for (uint32_t t = 0; t < nthreads; t++)
                pool.emplace_back([&, t] { check_rays(in, ray_trees, t, nthreads, nrays, part[t]); });
            for (std::thread& t : pool) t.join();
            RayStats st;
            for (const RayStats& p : part) {
                st.rays += p.rays; st.zero_comp += p.zero_comp; st.nan_dir += p.nan_dir; st.subnormal += p.subnormal;
                st.occluded += p.occluded; st.clear += p.clear; st.closest_found += p.closest_found; st.ties += p.ties;
            }
            std::printf("rays %s n %llu zero_component %llu nan %llu subnormal %llu occluded %llu clear %llu closest %llu ties %llu %s\n", base,
                        (unsigned long long)st.rays, (unsigned long long)st.zero_comp, (unsigned long long)st.nan_dir,
                        (unsigned long long)st.subnormal, (unsigned long long)st.occluded, (unsigned long long)st.clear,
                        (unsigned long long)st.closest_found, (unsigned long long)st.ties, g_fail == before ? "ok" : "BAD");
        }
    }
    std::printf("%s: %d failures\n", g_fail ? "FAILED" : "PASSED", g_fail.load());
    return g_fail ? 1 : 0;
}
