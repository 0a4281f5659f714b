// bvh.h -- host-side SAH BVH build, flattened into the stackless ("threaded") layout the kernels traverse.
// Replaces EmbreeInterface::initScene's rtcCommitScene(BUILD_QUALITY_HIGH) (embree_interface.cpp:30-51).
#pragma once

#include <cstdint>
#include <vector>

namespace romis {

struct BvhTriangle {
    float v0[3], v1[3], v2[3];
};

struct FlatBvh {
    // 8 floats per node: lo.xyz, bits(miss), hi.xyz, bits(leaf)   (see SceneDev in restir_types.h)
    std::vector<float> nodes;
    // triangle order: tri_order[k] = original index of the k-th triangle in BVH order
    std::vector<uint32_t> tri_order;
    uint32_t num_nodes = 0;
    uint32_t max_depth = 0;
};

// Builds a binned-SAH BVH (leaves of <= max_leaf triangles) and flattens it depth-first with miss links.
// Boxes are padded by `pad` in every direction so the device slab test is conservative.
FlatBvh build_bvh(const std::vector<BvhTriangle>& tris, uint32_t max_leaf = 4);

// Recomputes the boxes of `bvh` over moved triangles (the list build_bvh was given, same count and order, new vertex
// positions) and leaves its topology alone: miss links, leaf words, tri_order.  Each box is what build_bvh computes for
// the same subtree -- the unpadded min / max over its vertices, then lo - pad, hi + pad with pad = 1e-5f * scale + 1e-30f
// and scale taken from the new root -- so refitting with the triangles the tree was built from reproduces its nodes bit
// for bit.  The tree still only prunes; a refit tree of a scene that moved far from the one it was split for walks more
// nodes per ray and gives the same hits.  This is the specification of the device refit (refit.hip).
void refit_bvh(FlatBvh& bvh, const std::vector<BvhTriangle>& tris);

// The shadow rays' 16-byte nodes (SceneDev::nodes_q, kernels_common.h occluded_q): 4 words per node, six 16-bit bounds
// (lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16) on the grid lo + q * s over the root box, then
// miss link | first triangle << 16 | count << 28 (count 0: inner node).
struct QuantizedNodes {
    std::vector<uint32_t> words;   // 4 per node; 4 zero words when !ok
    float lo[3] = {0.0f, 0.0f, 0.0f}, s[3] = {1.0f, 1.0f, 1.0f};
    bool ok = false;               // < 65,536 nodes, every leaf < 16 triangles ending within the first 4,096, a finite grid
};

// Snaps each padded box of `bvh` outward to the 16-bit grid, so the quantized box contains the float one: a test against
// it accepts every box the float test accepts (and a few more), and any-hit decides by the exact triangle tests alone.
QuantizedNodes quantize_nodes(const FlatBvh& bvh);

}  // namespace romis
