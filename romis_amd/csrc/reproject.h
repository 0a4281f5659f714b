// reproject.h -- motion-compensated temporal reuse (restir_frame_reproject): where a surface point of the current frame
// was seen by the predecessor's camera, and whether the predecessor's pixel there shows the same surface.  One text for
// the host (restir_reproject_pixel) and the kernel (reproject.hip k_reproject); every step is a single float32 operation
// in a fixed order, compiled with -ffp-contract=off and correctly rounded division / sqrt on both sides, so the two
// agree bit for bit (DESIGN.md §6 "Reprojection").
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROMIS_HD __host__ __device__ __forceinline__
#else
#define ROMIS_HD inline
#endif

namespace romis {

// Why a pixel of the reprojected grid is empty (restir_frame_reproject's out_map holds 0xFFFFFFFF - reason)
constexpr uint32_t kReprojMiss = 0u;        // the current camera's primary ray hits nothing
constexpr uint32_t kReprojBehind = 1u;      // the point lies behind the predecessor's camera (!(c.z > 0))
constexpr uint32_t kReprojOffScreen = 2u;   // it projects outside the predecessor's image (or to NaN)
constexpr uint32_t kReprojPrevMiss = 3u;    // the predecessor's pixel there sees nothing
constexpr uint32_t kReprojDepth = 4u;       // ... or a surface at another depth
constexpr uint32_t kReprojNormal = 5u;      // ... or one turned away
constexpr uint32_t kReprojOk = 0xFFFFFFFFu;

// The predecessor's camera (restir_camera_frame's fields) and image size
struct ReprojCam {
    float qx, qy, qz, qw;   // scalars, not arrays: the kernel's argument stays in registers
    float ox, oy, oz;
    float half_w, half_h;
    uint32_t W, H;
};

// The source pixel of world point P: primary_pixel's ray of pixel (x, y) leaves o along R (-nx half_w, ny half_h, 1)
// with nx = x / W * 2 - 1, ny = y / H * 2 - 1 (kernels.hip; Trackball::generateRay), so with c = R^-1 (P - o) --
// quat * vec3 (type_quat.inl:347-354) of the conjugate, device_math.h qrotate's expressions -- the pixel is the nearest
// sample position to (-c.x / c.z / half_w, c.y / c.z / half_h).  d = glm::length(P - o), the depth the predecessor's
// pixel must show.  Returns kReprojOk with (sx, sy), else kReprojBehind / kReprojOffScreen.
// at (nullable): the continuous position (at[0], at[1]) the nearest pixel is rounded from -- pixel x sits at coordinate x, as
// primary_pixel places its sample -- for the image history's bilinear gather (history.h); written only with kReprojOk or
// kReprojOffScreen.  The same expressions either way: without `at` the function is what it was before the parameter existed.
ROMIS_HD uint32_t reproject_source(const ReprojCam& cam, float Px, float Py, float Pz, uint32_t& sx, uint32_t& sy, float& d,
                                   float* at = nullptr) {
    const float vx = Px - cam.ox, vy = Py - cam.oy, vz = Pz - cam.oz;
    d = sqrtf((vx * vx + vy * vy) + vz * vz);
    const float qx = -cam.qx, qy = -cam.qy, qz = -cam.qz, qw = cam.qw;
    const float ux = qy * vz - vy * qz, uy = qz * vx - vz * qx, uz = qx * vy - vx * qy;          // cross(q.xyz, v)
    const float wx = qy * uz - uy * qz, wy = qz * ux - uz * qx, wz = qx * uy - ux * qy;          // cross(q.xyz, uv)
    const float cx = vx + ((ux * qw) + wx) * 2.0f, cy = vy + ((uy * qw) + wy) * 2.0f, cz = vz + ((uz * qw) + wz) * 2.0f;
    sx = sy = 0u;
    if (!(cz > 0.0f)) return kReprojBehind;
    const float r = cx / cz;
    const float nx = (-r) / cam.half_w;
    const float s = cy / cz;
    const float ny = s / cam.half_h;
    const float cfx = ((nx + 1.0f) * 0.5f) * (float)cam.W;
    const float cfy = ((ny + 1.0f) * 0.5f) * (float)cam.H;
    const float fx = floorf(cfx + 0.5f);
    const float fy = floorf(cfy + 0.5f);
    if (at) {
        at[0] = cfx;
        at[1] = cfy;
    }
    if (!(fx >= 0.0f && fx < (float)cam.W && fy >= 0.0f && fy < (float)cam.H)) return kReprojOffScreen;   // NaN too
    sx = (uint32_t)fx;
    sy = (uint32_t)fy;
    return kReprojOk;
}

// The biased spatial test (render_utils.cpp:114-118) between the predecessor's pixel (its normal and t as stored in
// n_t) and the current pixel (its normal as load_px gives it), the current depth replaced by d: applied whatever
// unbiased_combination says.  kReprojOk, kReprojDepth or kReprojNormal (the depth test first, as the || reads).
ROMIS_HD uint32_t reproject_similar(float pnx, float pny, float pnz, float pt, float cnx, float cny, float cnz, float d) {
    const float depthFracDiff = fabsf(1.0f - pt / d);
    const float normalsDotProd = (pnx * cnx + pny * cny) + pnz * cnz;
    if (depthFracDiff > 0.1f) return kReprojDepth;
    if (normalsDotProd < 0.90630778703f) return kReprojNormal;
    return kReprojOk;
}

#if defined(__HIPCC__)
// One launch of k_reproject: W x H pixels, SoA planes [N][W * H] (restir_types.h Region, ps = 1).
struct ReprojDev {
    ReprojCam prev_cam;
    uint32_t N;
    uint32_t miss_mat;             // the miss material's index (SceneDev::num_materials - 1)
    const float4* cur_nt;          // the current camera's G-buffer
    const float4* cur_pm;
    const float4* prev_nt;         // the predecessor camera's, traced over the geometry as it stands now
    const float4* prev_pm;
    const float4* ia;              // the predecessor's res_a / res_b planes
    const float4* ib;
    float4* oa;                    // the reprojected grid's
    float4* ob;
    // frame handles (nullptr: the predecessor carries none): N = 1 the W plane then the M | index << 24 plane, N = 2
    // 16-byte records (W_0, M_0 | i_0 << 24, W_1, M_1 | i_1 << 24)
    const float* hin;
    float* hout;
    uint32_t zero_handle;          // the zero sample's M word: M = 0 | the light count << 24
    uint32_t* map;                 // nullable: the source pixel's flat index, or 0xFFFFFFFF - reason
};

// Enqueues on `stream`, never synchronises.
hipError_t launch_reproject(const ReprojDev& r, hipStream_t stream);
#endif

}  // namespace romis
