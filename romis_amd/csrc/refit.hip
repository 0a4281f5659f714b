// refit.hip -- the scene's traversal arrays recomputed from moved vertices (restir_update_meshes): triangle records,
// BVH boxes, quantized nodes.  The topology is the uploaded tree's; csrc/bvh.cpp refit_bvh and quantize_nodes specify
// every bit written here (DESIGN.md "Dynamic scenes").  Compiled with -ffp-contract=off like every other kernel: the pad
// is a product and a sum, as on the host.
//
// No launch here reads what another block of the same launch wrote: a small tree is one workgroup, a large one computes
// every node's box from that node's own triangle range, and the pad (which needs the root) runs in the next launch.
#include "refit.h"

#include <cfloat>

#include "launch_shape.h"

namespace romis {
namespace {

__device__ __forceinline__ float3 load3(const float* p, uint32_t v) {
    return make_float3(p[3u * v], p[3u * v + 1u], p[3u * v + 2u]);
}
__device__ __forceinline__ float3 min3(float3 a, float3 b) { return make_float3(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)); }
__device__ __forceinline__ float3 max3(float3 a, float3 b) { return make_float3(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)); }

// restir_set_scene's expressions: v0, e1 = v1 - v0, e2 = v2 - v0 (one rounding each), w = bits(original index)
__global__ __launch_bounds__(kBlock) void k_refit_triangles(RefitDev r) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= r.num_tris) return;
    const uint32_t orig = r.tri_order[k];
    const uint4 ix = r.tri_idx[orig];
    const float3 a = load3(r.vpos, ix.x), b = load3(r.vpos, ix.y), c = load3(r.vpos, ix.z);
    r.tri_v0[k] = make_float4(a.x, a.y, a.z, __uint_as_float(orig));
    r.tri_e1[k] = make_float4(b.x - a.x, b.y - a.y, b.z - a.z, 0.0f);
    r.tri_e2[k] = make_float4(c.x - a.x, c.y - a.y, c.z - a.z, 0.0f);
}

// vertex normals by original triangle index, n0.w = bits(mesh)
__global__ __launch_bounds__(kBlock) void k_refit_normals(RefitDev r) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= r.num_tris) return;
    const uint4 ix = r.tri_idx[t];
    const float3 a = load3(r.vnrm, ix.x), b = load3(r.vnrm, ix.y), c = load3(r.vnrm, ix.z);
    r.tri_n0[t] = make_float4(a.x, a.y, a.z, __uint_as_float(ix.w));
    r.tri_n1[t] = make_float4(b.x, b.y, b.z, 0.0f);
    r.tri_n2[t] = make_float4(c.x, c.y, c.z, 0.0f);
}

// the bounds of BVH-order triangle slot k's three vertices, merged into (lo, hi)
__device__ __forceinline__ void grow_slot(const RefitDev& r, uint32_t k, float3& lo, float3& hi) {
    const uint4 ix = r.tri_idx[r.tri_order[k]];
    const float3 a = load3(r.vpos, ix.x), b = load3(r.vpos, ix.y), c = load3(r.vpos, ix.z);
    lo = min3(lo, min3(a, min3(b, c)));
    hi = max3(hi, max3(a, max3(b, c)));
}

// build_bvh's pad from the unpadded root box
__device__ __forceinline__ float root_pad(float3 lo, float3 hi) {
    float scale = 0.0f;
    scale = fmaxf(fmaxf(scale, fabsf(lo.x)), fmaxf(fabsf(hi.x), hi.x - lo.x));
    scale = fmaxf(fmaxf(scale, fabsf(lo.y)), fmaxf(fabsf(hi.y), hi.y - lo.y));
    scale = fmaxf(fmaxf(scale, fabsf(lo.z)), fmaxf(fabsf(hi.z), hi.z - lo.z));
    return 1e-5f * scale + 1e-30f;
}

// quantize_nodes' grid step over the padded root box [lo, hi] (its q_lo is lo itself: a float is its own nearest float)
__device__ __forceinline__ float grid_step(float lo, float hi) {
    return (float)fmax(((double)hi - (double)lo) / 65532.0, 1e-30);
}

// Node i's padded box into nodes and, on the grid (q_lo, q_s) of the padded root, into nodes_q: quantize_nodes' floor /
// ceil of the same double quotients
__device__ __forceinline__ void write_node(const RefitDev& r, uint32_t i, float3 lo, float3 hi, float pad, float3 q_lo, float3 q_s) {
    const uint2 tp = r.topo[i];
    const float3 plo = make_float3(lo.x - pad, lo.y - pad, lo.z - pad), phi = make_float3(hi.x + pad, hi.y + pad, hi.z + pad);
    r.nodes[2u * i] = make_float4(plo.x, plo.y, plo.z, __uint_as_float(tp.x));
    r.nodes[2u * i + 1u] = make_float4(phi.x, phi.y, phi.z, __uint_as_float(tp.y));
    if (!r.q_ok) return;
    const float l[3] = {plo.x, plo.y, plo.z}, h[3] = {phi.x, phi.y, phi.z};
    const float ql0[3] = {q_lo.x, q_lo.y, q_lo.z}, qs[3] = {q_s.x, q_s.y, q_s.z};
    uint32_t q[6];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double ql = floor(((double)l[a] - (double)ql0[a]) / (double)qs[a]);
        const double qh = ceil(((double)h[a] - (double)ql0[a]) / (double)qs[a]);
        q[a] = (uint32_t)fmax(ql, 0.0);
        q[3 + a] = (uint32_t)fmin(fmax(qh, 0.0), 65535.0);
    }
    r.nodes_q[i] = make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16),
                              min(tp.x, 65535u) | ((tp.y & 0xFFFu) << 16) | ((tp.y >> 24) << 28));
}

// A tree that fits the LDS budget: one workgroup.  Levels from the deepest up -- a leaf's box from its triangles'
// vertices, an inner node's from its children's boxes in LDS (both one level down, written before the last barrier) --
// then the pad from the root and every node's padded and quantized box.  LDS: lo[nodes], hi[nodes] as float4.
constexpr uint32_t kRefitBlock = 1024;
__global__ __launch_bounds__(kRefitBlock) void k_refit_boxes_lds(RefitDev r) {
    extern __shared__ __attribute__((aligned(16))) float4 s_box[];
    const uint32_t n = r.num_nodes;
    float4* s_lo = s_box;
    float4* s_hi = s_box + n;
    for (uint32_t lvl = 0; lvl < r.levels; lvl++) {
        const uint32_t end = r.level_start[lvl + 1u];
        for (uint32_t j = r.level_start[lvl] + threadIdx.x; j < end; j += kRefitBlock) {
            const uint32_t i = r.level_nodes[j];
            const uint2 tp = r.topo[i];
            float3 lo = make_float3(FLT_MAX, FLT_MAX, FLT_MAX), hi = make_float3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
            if (tp.y) {
                const uint32_t first = tp.y & 0xFFFFFFu, cnt = tp.y >> 24;
                for (uint32_t k = first; k < first + cnt; k++) grow_slot(r, k, lo, hi);
            } else {
                const uint32_t left = i + 1u, right = r.topo[left].x;
                const float4 al = s_lo[left], ah = s_hi[left], bl = s_lo[right], bh = s_hi[right];
                lo = min3(make_float3(al.x, al.y, al.z), make_float3(bl.x, bl.y, bl.z));
                hi = max3(make_float3(ah.x, ah.y, ah.z), make_float3(bh.x, bh.y, bh.z));
            }
            s_lo[i] = make_float4(lo.x, lo.y, lo.z, 0.0f);
            s_hi[i] = make_float4(hi.x, hi.y, hi.z, 0.0f);
        }
        __syncthreads();
    }
    const float3 rlo = make_float3(s_lo[0].x, s_lo[0].y, s_lo[0].z), rhi = make_float3(s_hi[0].x, s_hi[0].y, s_hi[0].z);
    const float pad = root_pad(rlo, rhi);
    const float3 q_lo = make_float3(rlo.x - pad, rlo.y - pad, rlo.z - pad);
    const float3 q_s = make_float3(grid_step(q_lo.x, rhi.x + pad), grid_step(q_lo.y, rhi.y + pad), grid_step(q_lo.z, rhi.z + pad));
    for (uint32_t i = threadIdx.x; i < n; i += kRefitBlock)
        write_node(r, i, make_float3(s_lo[i].x, s_lo[i].y, s_lo[i].z), make_float3(s_hi[i].x, s_hi[i].y, s_hi[i].z), pad, q_lo, q_s);
}

// A larger tree, first launch: one wave per node reduces the node's own triangle range (its subtree's triangles are
// contiguous in BVH order) -- O(triangles x depth) reads of arrays no block of this launch writes.
__global__ __launch_bounds__(kBlock) void k_refit_boxes_wave(RefitDev r) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
    if (i >= r.num_nodes) return;   // whole waves leave together
    const uint2 rg = r.range[i];
    float3 lo = make_float3(FLT_MAX, FLT_MAX, FLT_MAX), hi = make_float3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
    for (uint32_t k = lane; k < rg.y; k += 64u) grow_slot(r, rg.x + k, lo, hi);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min3(lo, make_float3(__shfl_xor(lo.x, d, 64), __shfl_xor(lo.y, d, 64), __shfl_xor(lo.z, d, 64)));
        hi = max3(hi, make_float3(__shfl_xor(hi.x, d, 64), __shfl_xor(hi.y, d, 64), __shfl_xor(hi.z, d, 64)));
    }
    if (lane == 0u) {
        r.raw[2u * i] = make_float4(lo.x, lo.y, lo.z, 0.0f);
        r.raw[2u * i + 1u] = make_float4(hi.x, hi.y, hi.z, 0.0f);
    }
}

// ... second launch: the pad from the root's box, then each node's padded and quantized box
__global__ __launch_bounds__(kBlock) void k_refit_finish(RefitDev r) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.num_nodes) return;
    const float4 r0 = r.raw[0], r1 = r.raw[1];
    const float3 rlo = make_float3(r0.x, r0.y, r0.z), rhi = make_float3(r1.x, r1.y, r1.z);
    const float pad = root_pad(rlo, rhi);
    const float3 q_lo = make_float3(rlo.x - pad, rlo.y - pad, rlo.z - pad);
    const float3 q_s = make_float3(grid_step(q_lo.x, rhi.x + pad), grid_step(q_lo.y, rhi.y + pad), grid_step(q_lo.z, rhi.z + pad));
    const float4 lo = r.raw[2u * i], hi = r.raw[2u * i + 1u];
    write_node(r, i, make_float3(lo.x, lo.y, lo.z), make_float3(hi.x, hi.y, hi.z), pad, q_lo, q_s);
}

inline dim3 blocks_of(uint32_t n, uint32_t per) { return dim3((n + per - 1u) / per); }

}  // namespace

bool refit_fits_lds(uint32_t num_nodes, uint32_t num_tris) {
    return ((size_t)2 * num_nodes + (size_t)3 * num_tris) * 16 <= kLdsBudget;
}

hipError_t launch_refit_triangles(const RefitDev& r, bool normals, hipStream_t stream) {
    if (!r.num_tris) return hipSuccess;
    hipLaunchKernelGGL(k_refit_triangles, blocks_of(r.num_tris, kBlock), dim3(kBlock), 0, stream, r);
    if (normals) hipLaunchKernelGGL(k_refit_normals, blocks_of(r.num_tris, kBlock), dim3(kBlock), 0, stream, r);
    return hipGetLastError();
}

hipError_t launch_refit_boxes(const RefitDev& r, hipStream_t stream) {
    if (!r.num_nodes) return hipSuccess;
    if (refit_fits_lds(r.num_nodes, r.num_tris)) {
        hipLaunchKernelGGL(k_refit_boxes_lds, dim3(1), dim3(kRefitBlock), (size_t)r.num_nodes * 32, stream, r);
    } else {
        if (!r.raw) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_refit_boxes_wave, blocks_of(r.num_nodes, kBlock / 64u), dim3(kBlock), 0, stream, r);
        hipLaunchKernelGGL(k_refit_finish, blocks_of(r.num_nodes, kBlock), dim3(kBlock), 0, stream, r);
    }
    return hipGetLastError();
}

}  // namespace romis
