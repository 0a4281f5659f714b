// present.hip -- the conversion of restir_image_begin: the context's last image (float3 per pixel, row 0 = top) into
// 8-bit pixels in a staging buffer (present.h has the steps and DESIGN.md §6 "Presenting a frame" the semantics).
// Compiled with -ffp-contract=off like every other kernel; the multiply by 255 is the host's single float32 multiply.
//
// A lane converts four consecutive pixels of one run: three 16-byte loads (48 B) and one 16-byte store where the
// group lies wholly inside the run and both its source and its destination are 16-byte aligned -- every group of
// RGBA8's single run but the last partial one, and every group of BGRA8_BOTTOM_UP's per-row runs when W % 4 == 0.
// The other groups convert pixel by pixel (three 4-byte loads, one 4-byte store each).  Nothing is shared between
// lanes: no LDS, no barrier.  Every index is below rows * row_px: the group's first pixel by the bounds test, the
// others by the in-run test.
#include "present.h"

namespace romis {
namespace {

constexpr uint32_t kPresentBlock = 256;

template <bool kBgr>
__global__ __launch_bounds__(kPresentBlock) void k_present(PresentDev p) {
    const uint64_t x = ((uint64_t)blockIdx.x * kPresentBlock + threadIdx.x) * 4u;   // the group's first pixel in its run
    if (x >= p.row_px) return;
    for (uint32_t y = blockIdx.y; y < p.rows; y += gridDim.y) {
        const uint64_t src = (uint64_t)y * p.row_px + x;                                  // pixel index in rgb
        const uint64_t dst = (uint64_t)(p.bgr_flip ? p.rows - 1u - y : y) * p.row_px + x;   // ... and in out
        const float* s = p.rgb + src * 3u;
        uint32_t* o = p.out + dst;
        if (x + 4u <= p.row_px && ((src | dst) & 3u) == 0u) {
            const float4 a = reinterpret_cast<const float4*>(s)[0];
            const float4 b = reinterpret_cast<const float4*>(s)[1];
            const float4 c = reinterpret_cast<const float4*>(s)[2];
            uint4 w;
            w.x = present_word<kBgr>(a.x, a.y, a.z);
            w.y = present_word<kBgr>(a.w, b.x, b.y);
            w.z = present_word<kBgr>(b.z, b.w, c.x);
            w.w = present_word<kBgr>(c.y, c.z, c.w);
            *reinterpret_cast<uint4*>(o) = w;
            // keeps the store whole: without it hipcc sinks its last word into the per-pixel path's fourth store and
            // leaves 12 + 4 bytes here
            asm volatile("" ::: "memory");
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                if (x + k < p.row_px) o[k] = present_word<kBgr>(s[3u * k], s[3u * k + 1u], s[3u * k + 2u]);
        }
    }
}

}  // namespace

hipError_t launch_present(const PresentDev& p, hipStream_t stream) {
    if (!p.row_px || !p.rows) return hipSuccess;
    const uint64_t groups = (p.row_px + 3u) / 4u;
    const uint64_t bx = (groups + kPresentBlock - 1u) / kPresentBlock;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)bx, p.rows < 65535u ? p.rows : 65535u);
    if (p.bgr_flip)
        hipLaunchKernelGGL(k_present<true>, grid, dim3(kPresentBlock), 0, stream, p);
    else
        hipLaunchKernelGGL(k_present<false>, grid, dim3(kPresentBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace romis
