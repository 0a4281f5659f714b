// refit.h -- host-side launchers of the kernels in refit.hip: the scene's traversal arrays recomputed on the device from
// moved vertices (restir_update_meshes).  All enqueue on `stream`, never synchronise.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace romis {

// What a refit reads and writes.  The tables are written once per scene upload (restir_set_scene) and describe the
// tree's topology, which a refit keeps; bvh.h refit_bvh and quantize_nodes specify the results.
struct RefitDev {
    uint32_t num_nodes, num_tris;
    uint32_t q_ok;                 // the scene has quantized nodes (SceneDev::nodes_q_ok)
    // per scene upload
    const float* vpos;             // [vertices][3] positions of all meshes, back to back (the part an update overwrites)
    const float* vnrm;             // [vertices][3] normals
    const uint4* tri_idx;          // [triangles], original order: the three vertex indices into vpos / vnrm, the mesh
    const uint32_t* tri_order;     // [triangles]: original index of the k-th triangle in BVH order
    const uint2* topo;             // [nodes]: (miss link, leaf word) -- FlatBvh's nodes[8i + 3], nodes[8i + 7]
    const uint2* range;            // [nodes]: the subtree's triangles, (first BVH-order slot, count)
    const uint32_t* level_nodes;   // [nodes]: node indices by depth, the deepest level first
    const uint32_t* level_start;   // [levels + 1]: level l (0 = the deepest) is level_nodes[level_start[l] .. level_start[l + 1])
    uint32_t levels;
    // the scene arrays (SceneDev)
    float4* nodes;
    uint4* nodes_q;
    float4 *tri_v0, *tri_e1, *tri_e2, *tri_n0, *tri_n1, *tri_n2;
    float4* raw;                   // [2 * nodes] unpadded boxes between the two launches of a tree too large for LDS
};

// (2 nodes + 3 triangles) * 16 bytes within the LDS budget of the frame kernels' staged BVH: one workgroup refits the
// boxes in one launch
bool refit_fits_lds(uint32_t num_nodes, uint32_t num_tris);

// tri_v0 / tri_e1 / tri_e2 in BVH order from vpos; normals: tri_n0 / n1 / n2 by original index from vnrm as well
hipError_t launch_refit_triangles(const RefitDev& r, bool normals, hipStream_t stream);
// nodes and (q_ok) nodes_q from vpos: one launch where refit_fits_lds, else two (boxes per node, then pad + quantize)
hipError_t launch_refit_boxes(const RefitDev& r, hipStream_t stream);

}  // namespace romis
