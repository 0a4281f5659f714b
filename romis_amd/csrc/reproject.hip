// reproject.hip -- the gather of restir_frame_reproject: a predecessor grid moved to where the current camera sees its
// surface points (reproject.h has the steps and DESIGN.md §6 "Reprojection" the semantics).  Compiled with
// -ffp-contract=off like every other kernel: the source pixel is the host's restir_reproject_pixel bit for bit.
//
// One lane per pixel, 32 x 8 blocks over the image.  A lane reads its own two G-buffer records, the two records of
// its source pixel, and copies that pixel's N sub-reservoirs (and frame handles); nothing is shared between lanes, so
// there is no LDS and no barrier.  Every index is below W * H: the lane's own by the bounds test, the source's by
// reproject_source's range test.
#include "reproject.h"

#include "launch_shape.h"

namespace romis {
namespace {

__device__ __forceinline__ bool is_miss(const ReprojDev& r, float4 pm) {
    return min(__float_as_uint(pm.w), r.miss_mat) == r.miss_mat;   // make_px's clamp
}

__global__ __launch_bounds__(kBlock) void k_reproject(ReprojDev r) {
    const uint32_t x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
    const uint32_t W = r.prev_cam.W, H = r.prev_cam.H;
    if (x >= W || y >= H) return;
    const size_t npx = (size_t)W * H, p = (size_t)y * W + x;
    uint32_t why = kReprojMiss, sx = 0u, sy = 0u;
    size_t q = 0;
    const float4 cpm = r.cur_pm[p];
    if (!is_miss(r, cpm)) {
        float d;
        why = reproject_source(r.prev_cam, cpm.x, cpm.y, cpm.z, sx, sy, d);
        if (why == kReprojOk) {
            q = (size_t)sy * W + sx;
            const float4 cnt = r.cur_nt[p], ppm = r.prev_pm[q], pnt = r.prev_nt[q];
            why = is_miss(r, ppm) ? kReprojPrevMiss : reproject_similar(pnt.x, pnt.y, pnt.z, pnt.w, cnt.x, cnt.y, cnt.z, d);
        }
    }
    const bool ok = why == kReprojOk;
    for (uint32_t j = 0; j < r.N; j++) {
        const size_t o = (size_t)j * npx;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (ok) {   // (a load under the lane mask: a select between the two addresses would put the zeros in scratch)
            a = r.ia[o + q];
            b = r.ib[o + q];
        }
        r.oa[o + p] = a;
        r.ob[o + p] = b;
    }
    if (r.hin) {
        const float zh = __uint_as_float(r.zero_handle);
        if (r.N == 1u) {
            const uint32_t* hm = reinterpret_cast<const uint32_t*>(r.hin + npx);
            uint32_t* om = reinterpret_cast<uint32_t*>(r.hout + npx);
            r.hout[p] = ok ? r.hin[q] : 0.0f;
            om[p] = ok ? hm[q] : r.zero_handle;
        } else {
            reinterpret_cast<float4*>(r.hout)[p] =
                ok ? reinterpret_cast<const float4*>(r.hin)[q] : make_float4(0.0f, zh, 0.0f, zh);
        }
    }
    if (r.map) r.map[p] = ok ? (uint32_t)q : 0xFFFFFFFFu - why;
}

}  // namespace

hipError_t launch_reproject(const ReprojDev& r, hipStream_t stream) {
    const uint32_t W = r.prev_cam.W, H = r.prev_cam.H;
    if (!W || !H) return hipSuccess;
    hipLaunchKernelGGL(k_reproject, dim3((W + kTileW - 1u) / kTileW, (H + kTileH - 1u) / kTileH), dim3(kTileW, kTileH), 0,
                       stream, r);
    return hipGetLastError();
}

}  // namespace romis
