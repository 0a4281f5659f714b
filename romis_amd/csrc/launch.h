// launch.h -- host-side launchers of the kernels in kernels.hip (all enqueue on `stream`, never synchronise).
#pragma once

#include "restir_types.h"
#include "route.h"

namespace romis {

// The buffers of one frame-stage launch.  A launcher passes a kernel the ones its route names and null for the rest; a
// route that names a buffer the caller left null is a programming error (asserted).
struct LaunchBufs {
    uint32_t key = 0;                  // the stage's RNG key
    const CameraDev* cam = nullptr;    // primary rays
    const float* origin = nullptr;     // the camera origin (every other stage)
    float4* n_t = nullptr;             // G-buffer
    float4* p_mat = nullptr;
    float4* n_t2 = nullptr;            // a second record buffer that also receives the G-buffer n_t (the ping-pong partner)
    const float4* ia = nullptr;        // input reservoirs (temporal: the current grid; spatial; final shading)
    const float4* ib = nullptr;
    float4* oa = nullptr;              // output reservoirs
    float4* ob = nullptr;
    float2* dbg = nullptr;             // debug plane of the output
    // The target-pdf cache (N = 1, SoA planes): rp[p] = the target pdf of pixel p's held sample at p.  RIS / temporal /
    // the lean spatial passes write it for their output; temporal and the passes read it for the input's own sample
    // instead of re-evaluating it (same pixel, same G-buffer, same sample: the same bits).
    const float* rp_in = nullptr;
    float* rp_out = nullptr;
    uint8_t* vis = nullptr;            // own-pixel ray plane: a spatial pass writes it, final shading reads it
    uint8_t* flags = nullptr;          // MissTiles flags: primary + RIS writes them, the passes and final shading read
    Handles hin{nullptr, nullptr};     // the input's sample handles
    Handles hout{nullptr, nullptr};    // the output's
    float* rgb = nullptr;              // final shading's image (the owned rect)
    const uint4* shadow_lists = nullptr;   // the view's shadow-list records (shadow_lists.h), for a route with `lists`
    const uint32_t* shadow_vis = nullptr;  // the view's visibility bits (shadow_vis.h), for a route with `bits`
    const float* phat = nullptr;       // the view's p-hat table (phat_table.h), for a route with `phat`
    TemporalIn tin{};                  // primary + RIS + temporal: the predecessor grid
};

// One launcher per frame stage; its route (route.h) is computed from the same s, rg and f.
hipError_t launch_primary(const Route& r, const SceneDev& s, const Region& rg, const LaunchBufs& b, hipStream_t stream);
hipError_t launch_ris(const Route& r, const SceneDev& s, const Region& rg, const FeaturesDev& f, const LaunchBufs& b,
                      hipStream_t stream);
// genPrimaryRayHits + genCanonicalSamples in one kernel over the same region (route_primary_ris), with temporal reuse
// too (route_primary_ris_temporal).  A route of the k_gbuf_ris family (Kernel::kGbufRis / kGbufRisTemporal, Ask::gbuf_cached)
// reads b.n_t, b.p_mat and b.flags as an earlier frame of the same view left them and writes none of them.
hipError_t launch_primary_ris(const Route& r, const SceneDev& s, const Region& rg, const FeaturesDev& f, const LaunchBufs& b,
                              hipStream_t stream);
// launch_primary_ris's launch for a kGbufRis route with `phat` (phat_table.hip)
hipError_t launch_gbuf_ris_phat(const Route& r, const SceneDev& s, const Region& rg, const FeaturesDev& f, const LaunchBufs& b,
                                hipStream_t stream);
// ... for two RNG keys in one pass over the table (DESIGN.md §6 "RIS batch"): what each key's result is written to
struct RisBatchOut {
    uint32_t key = 0;
    Handles h{nullptr, nullptr};
    float* rp = nullptr;
};
hipError_t launch_gbuf_ris_phat_batch(const Route& r, const SceneDev& s, const Region& rg, const FeaturesDev& f, const LaunchBufs& b,
                                      const RisBatchOut (&out)[2], hipStream_t stream);
hipError_t launch_temporal(const SceneDev& s, const Region& rg, const FeaturesDev& f, uint32_t key, const float* origin,
                           const float4* n_t, const float4* p_mat, const float4* ca, const float4* cb,
                           const float4* pa, const float4* pb, float4* oa, float4* ob, float2* odbg,
                           const float* rp_in, float* rp_out, hipStream_t stream);
// r.final_done: final shading ran in the pass's kernel (b.rgb), the caller skips launch_final
hipError_t launch_spatial(const Route& r, const SceneDev& s, const Region& rg, const FeaturesDev& f, const LaunchBufs& b,
                          hipStream_t stream);
hipError_t launch_final(const Route& r, const SceneDev& s, const Region& rg, const FeaturesDev& f, const LaunchBufs& b,
                        hipStream_t stream);
hipError_t launch_halo_pack(const Region& rg, const HaloSegs& hs, uint32_t N, const float4* ra, const float4* rb, float4* out,
                            hipStream_t stream);
hipError_t launch_halo_unpack(const Region& rg, const HaloSegs& hs, uint32_t N, const float4* in, float4* ra, float4* rb,
                              hipStream_t stream);
// The next frame-kernel launch records `start` / `stop` (nullptr: none) within its dispatch; launch_events_used()
// tells whether a launch consumed them since the last set_launch_events.
void set_launch_events(hipEvent_t start, hipEvent_t stop);
bool launch_events_used();
hipError_t launch_read_stream(const float4* buf, size_t n4, float* sink, hipStream_t stream);
// R-MIS / R-OMIS over a whole W x H image (stage / frame buffers in the RESTIR_BUF_MIS_* layouts)
hipError_t launch_mis_neighbours(const SceneDev& s, uint32_t W, uint32_t H, const FeaturesDev& f, uint32_t key_s, uint32_t key_d,
                                 const float4* n_t, const float4* p_mat, uint32_t* nbr, hipStream_t stream);
hipError_t launch_mis_accumulate(const SceneDev& s, uint32_t W, uint32_t H, const FeaturesDev& f, const float* origin,
                                 const float4* n_t, const float4* p_mat, const uint32_t* nbr, const float4* ra,
                                 const float4* rb, const float2* rdbg, uint32_t iteration, float* acc, float* smp,
                                 uint32_t smp_samples, const Tuning& tu, hipStream_t stream);
hipError_t launch_mis_finish(uint32_t W, uint32_t H, const FeaturesDev& f, const float* acc, float* rgb, hipStream_t stream);
// The same over a screen tile (MisTile: n_t, p_mat, ra, rb, rdbg by view pixel; nbr, acc, smp by owned pixel; rgb = the
// owned rectangle, row 0 = its top)
hipError_t launch_mis_neighbours(const SceneDev& s, const MisTile& t, const FeaturesDev& f, uint32_t key_s, uint32_t key_d,
                                 const float4* n_t, const float4* p_mat, uint32_t* nbr, hipStream_t stream);
hipError_t launch_mis_accumulate(const SceneDev& s, const MisTile& t, const FeaturesDev& f, const float* origin,
                                 const float4* n_t, const float4* p_mat, const uint32_t* nbr, const float4* ra,
                                 const float4* rb, const float2* rdbg, uint32_t iteration, float* acc, float* smp,
                                 uint32_t smp_samples, const Tuning& tu, hipStream_t stream);
hipError_t launch_mis_finish(const MisTile& t, const FeaturesDev& f, const float* acc, float* rgb, hipStream_t stream);
// R-OMIS alpha visualisation words: [3T images][W*H] (k_romis_vis_t{T})
hipError_t launch_romis_vis(uint32_t W, uint32_t H, uint32_t T, const float* acc, uint32_t* out, hipStream_t stream);
hipError_t launch_debug_cod(uint32_t n, const float* A, const float* b, float* x, uint32_t count, hipStream_t stream);
hipError_t launch_debug_math(const float* x, const float* y, float* pw, float* ex, uint32_t n, hipStream_t stream);

}  // namespace romis
