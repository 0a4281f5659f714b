// shadow_lists_check -- host check of csrc/shadow_lists.h: no record may leave out a triangle that a ray of its family
// hits.  tests/test_shadow_lists_host.py writes the case files and reads the lines printed here.
//
//   shadow_lists_check [--points N] [--cap C] case.bin [case.bin ...]
//
// A case file (little-endian): uint32 triangles, lights, tiles; v0, e1, e2 as [triangles][4] floats (the traversal
// arrays' records); per light 3 floats and a uint32 (1: its records must all say "walk the BVH"); per tile 6 floats,
// the box of its hit points (lo, hi).  Per (tile, light) the record is built as k_shadow_lists builds it; N seeded random
// start points inside the tile box are then traced with visible()'s own ray (restated below in the device's operation
// order) against every triangle, and a hit triangle missing from a list is an error.
//
// One line per case:  <file> pairs P rays R hits H missing M bad_index B must_walk_violations V walk K hist c0 .. c15
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "shadow_lists.h"

using namespace romis;

namespace {

struct V3 { float x, y, z; };
V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 x, V3 y) { return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y}; }
V3 normalize(V3 a) { return scale(a, 1.0f / sqrtf(dot(a, a))); }

// kernels_common.h tri_any
bool tri_any(const float* v0, const float* e1_, const float* e2_, V3 o, V3 d, float tfar) {
    const V3 e1{e1_[0], e1_[1], e1_[2]}, e2{e2_[0], e2_[1], e2_[2]};
    const V3 pvec = cross(d, e2);
    const float det = dot(e1, pvec);
    const float inv = 1.0f / det;
    const V3 tvec = sub(o, V3{v0[0], v0[1], v0[2]});
    const float u = dot(tvec, pvec) * inv;
    const V3 qvec = cross(tvec, e1);
    const float v = dot(d, qvec) * inv;
    const float t = dot(e2, qvec) * inv;
    return det != 0.0f && (u >= 0.0f && u <= 1.0f) && (v >= 0.0f && u + v <= 1.0f) && (t > 0.0f && t <= tfar);
}

uint32_t g_rng = 0x9E3779B9u;
float rnd() {   // xorshift32 -> [0, 1]
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
    return (float)(g_rng >> 8) / 16777215.0f;
}

bool read_all(const char* path, std::vector<char>& buf) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    buf.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n >= 0 && std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    return ok;
}

int run_case(const char* path, uint32_t points, uint32_t cap) {
    std::vector<char> buf;
    if (!read_all(path, buf) || buf.size() < 12) { std::printf("%s unreadable\n", path); return 1; }
    uint32_t hdr[3];
    std::memcpy(hdr, buf.data(), 12);
    const uint32_t nt = hdr[0], nl = hdr[1], ntile = hdr[2];
    const size_t want = 12 + (size_t)nt * 48 + (size_t)nl * 16 + (size_t)ntile * 24;
    if (buf.size() != want) { std::printf("%s size %zu, expected %zu\n", path, buf.size(), want); return 1; }
    std::vector<float> v0(4 * (size_t)nt), e1(v0.size()), e2(v0.size()), lights(4 * (size_t)nl), tiles(6 * (size_t)ntile);
    const char* p = buf.data() + 12;
    std::memcpy(v0.data(), p, v0.size() * 4); p += v0.size() * 4;
    std::memcpy(e1.data(), p, e1.size() * 4); p += e1.size() * 4;
    std::memcpy(e2.data(), p, e2.size() * 4); p += e2.size() * 4;
    std::memcpy(lights.data(), p, lights.size() * 4); p += lights.size() * 4;
    std::memcpy(tiles.data(), p, tiles.size() * 4);

    // the scene's bounds (the root box k_shadow_lists reads carries build_bvh's padding on top: a larger margin)
    SlBox root;
    for (int a = 0; a < 3; a++) { root.lo[a] = 3.402823466e+38F; root.hi[a] = -3.402823466e+38F; }
    for (uint32_t k = 0; k < nt; k++)
        for (int a = 0; a < 3; a++) {
            const float c[3] = {v0[4 * k + a], v0[4 * k + a] + e1[4 * k + a], v0[4 * k + a] + e2[4 * k + a]};
            for (float x : c) { root.lo[a] = fminf(root.lo[a], x); root.hi[a] = fmaxf(root.hi[a], x); }
        }
    const float m = sl_margin(root);
    std::vector<SlTri> tris(nt);
    for (uint32_t k = 0; k < nt; k++) tris[k] = sl_tri(v0.data(), e1.data(), e2.data(), k, m);

    unsigned long long pairs = 0, rays = 0, hits = 0, missing = 0, bad_index = 0, must = 0, walk = 0, hist[16] = {0};
    unsigned long long walk_tiles = 0;
    for (uint32_t t = 0; t < ntile; t++) {
        SlBox T;
        bool bad = false;
        for (int a = 0; a < 3; a++) {
            T.lo[a] = tiles[6 * t + a]; T.hi[a] = tiles[6 * t + 3 + a];
            bad = bad || !sl_finite(T.lo[a]) || !sl_finite(T.hi[a]);
        }
        const bool empty = !bad && (T.lo[0] > T.hi[0] || T.lo[1] > T.hi[1] || T.lo[2] > T.hi[2]);
        const SlTile tile = sl_tile(T, m);
        bool tile_walks = false;
        for (uint32_t l = 0; l < nl; l++) {
            const float* y = &lights[4 * l];
            uint32_t must_walk;
            std::memcpy(&must_walk, y + 3, 4);
            const SlRecord r = sl_record(tile, empty, bad, y, tris.data(), nt, cap);
            const uint32_t cnt = sl_count(r);
            pairs++;
            if (cnt == kSlWalk) { walk++; tile_walks = tile_walks || !must_walk; }
            else if (cnt <= kSlCap) hist[cnt]++;
            else bad_index++;
            if (must_walk && !empty && cnt != kSlWalk) must++;
            if (cnt == kSlWalk || empty) continue;
            if (cnt > cap) { bad_index++; continue; }
            bool in_list[kSlMaxTris] = {false};
            for (uint32_t k = 0; k < cnt; k++) {
                const uint32_t i = sl_index(r, k);
                if (i >= nt) bad_index++;
                else in_list[i] = true;
            }
            for (uint32_t q = 0; q < points; q++) {
                // corners and faces as well as the interior: every third point snaps each coordinate to an end
                V3 P;
                float* c = &P.x;
                for (int a = 0; a < 3; a++) {
                    float w = rnd();
                    if (q % 3u == 0u) w = w < 0.5f ? 0.0f : 1.0f;
                    c[a] = T.lo[a] + (T.hi[a] - T.lo[a]) * w;
                    c[a] = fminf(fmaxf(c[a], T.lo[a]), T.hi[a]);
                }
                // visible(): kernels_common.h
                const V3 Y{y[0], y[1], y[2]};
                const V3 dir = normalize(sub(Y, P));
                const V3 P2 = add(P, scale(dir, 1e-3f));
                const V3 d2 = sub(Y, P2);
                const float tfar = sqrtf(dot(d2, d2));
                rays++;
                for (uint32_t k = 0; k < nt; k++)
                    if (tri_any(&v0[4 * k], &e1[4 * k], &e2[4 * k], P2, dir, tfar)) {
                        hits++;
                        if (!in_list[k]) missing++;
                    }
            }
        }
        if (tile_walks) walk_tiles++;
    }
    std::fprintf(stderr, "%s: %llu of %u tiles hold a record that walks the BVH (lights that must walk aside)\n", path, walk_tiles, ntile);
    std::printf("%s pairs %llu rays %llu hits %llu missing %llu bad_index %llu must_walk_violations %llu walk %llu hist", path,
                pairs, rays, hits, missing, bad_index, must, walk);
    for (int i = 0; i < 16; i++) std::printf(" %llu", hist[i]);
    std::printf("\n");
    return (missing || bad_index || must) ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    uint32_t points = 8, cap = kSlCap;
    int rc = 0, i = 1;
    for (; i < argc; i++) {
        if (!std::strcmp(argv[i], "--points") && i + 1 < argc) points = (uint32_t)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--cap") && i + 1 < argc) cap = (uint32_t)std::atoi(argv[++i]);
        else break;
    }
    if (i >= argc || cap < 1 || cap > kSlCap) {
        std::fprintf(stderr, "usage: shadow_lists_check [--points N] [--cap 1..15] case.bin ...\n");
        return 2;
    }
    for (; i < argc; i++) rc |= run_case(argv[i], points, cap);
    return rc;
}
