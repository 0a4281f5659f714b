// present.h -- a frame as 8-bit pixels (restir_image_begin): the context's last image, float3 per owned pixel with row
// 0 = top, converted on the device into a staging buffer that a pinned host buffer then receives.  The steps are those
// of the host's restir_rgb_to_rgba8 (screen.cpp): a comparison, a select or one float32 multiply each, so the kernel
// (present.hip k_present) and the host agree byte for byte (DESIGN.md §6 "Presenting a frame").
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROMIS_PRESENT_HD __host__ __device__ __forceinline__
#else
#define ROMIS_PRESENT_HD inline
#endif

namespace romis {

// Screen::writeBitmapToFile's byte of one colour value (screen.cpp:45-51): glm::clamp(x, 0, 1) with glm's comparisons
// (x < 0 ? 0 : x, then 1 < m ? 1 : m: a NaN passes through both), one float32 multiply by 255, NaN -> 0 (x86-64's
// cvttss2si gives 0x80000000, low byte 0), truncation toward zero.  The product lies in [0, 255] or is NaN.
ROMIS_PRESENT_HD uint32_t present_byte(float x) {
    const float m = (x < 0.0f) ? 0.0f : x;
    const float c = (1.0f < m) ? 1.0f : m;
    const float v = c * 255.0f;
    return (v != v) ? 0u : (uint32_t)(int)v;
}

// One pixel's 32-bit word as it lies in memory (little endian): R, G, B, A bytes, or stbi_write_bmp's B, G, R, A
template <bool kBgr>
ROMIS_PRESENT_HD uint32_t present_word(float r, float g, float b) {
    const uint32_t br = present_byte(r), bg = present_byte(g), bb = present_byte(b);
    return kBgr ? (bb | (bg << 8) | (br << 16) | 0xFF000000u) : (br | (bg << 8) | (bb << 16) | 0xFF000000u);
}

#if defined(__HIPCC__)
// One launch of k_present over `rows` runs of `row_px` pixels: run y of `rgb` (3 floats per pixel, runs back to back)
// becomes run (flip ? rows - 1 - y : y) of `out` (4 bytes per pixel).  RGBA8 is ONE run of all the image's pixels;
// BGRA8_BOTTOM_UP is a run per image row, flipped.  Both buffers are 16-byte aligned (hipMalloc) and hold
// rows * row_px pixels.
struct PresentDev {
    const float* rgb;
    uint32_t* out;
    uint64_t row_px;
    uint32_t rows;
    bool bgr_flip;
};

// Enqueues on `stream`, never synchronises.
hipError_t launch_present(const PresentDev& p, hipStream_t stream);
#endif

}  // namespace romis
