// restir.cpp -- implementation of the C ABI in include/restir_c.h (host side of libromis_amd.so).
//
// Drop-in for renderReSTIR / renderRayTraced (src/rendering/render.cpp:28-62, :268-290): a context owns one
// HIP device + stream, the uploaded scene (materials, lights, flattened BVH) and the per-frame device
// buffers; every pass is one hand-written gfx950 kernel (kernels.hip) enqueued on the context's stream.
#include "abi_error.h"
#include "accum.h"
#include "denoise.h"
#include "exact.h"
#include "history.h"
#include "layout.h"

#include <rccl/rccl.h>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <dlfcn.h>
#include <filesystem>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <vector>

#include "bvh.h"
#include "device_math.h"
#include "launch.h"
#include "refit.h"
#include "present.h"
#include "reproject.h"
#include "restir_types.h"
#include "shadow_lists.h"
#include "phat_table.h"
#include "shadow_vis.h"
#include "ris_ahead.h"

namespace romis {
bool write_bmp_words(const char* path, uint32_t width, uint32_t height, const uint32_t* words);   // screen.cpp
restir_status denoise_params_check(const restir_denoise_params* p, const char* who);               // denoise_host.cpp
restir_status denoise_lum_params_check(const restir_denoise_lum_params* p, const char* who);
restir_status history_params_check(const restir_history_params* p, const char* who);                 // history_host.cpp
}
using namespace romis;

// ---------------------------------------------------------------------------------------------------------
// errors
namespace {
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(RESTIR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    restir_status ensure(size_t n) {
        if (n <= bytes && p) return RESTIR_OK;
        release();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; bytes = 0; return fail(RESTIR_ERR_HIP, "hipMalloc(%zu): %s", n, hipGetErrorString(e)); }
        bytes = n;
        return RESTIR_OK;
    }
    restir_status upload(const void* h, size_t n, hipStream_t s) {
        ST_TRY(ensure(n));
        HIP_TRY(hipMemcpyAsync(p, h, n, hipMemcpyHostToDevice, s));
        return RESTIR_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
// the exponent classes material_pow branches on (ROMIS_PWC_*): glibc's checkint(y) and zeroinfnan(y) cases
uint32_t pw_class(float y) {
    uint32_t iy; std::memcpy(&iy, &y, 4);
    if (std::isnan(y)) return ROMIS_PWC_NAN;
    if (y == 0.0f) return ROMIS_PWC_ZERO;
    if (std::isinf(y)) return y > 0.0f ? ROMIS_PWC_PINF : ROMIS_PWC_NINF;
    uint32_t c = y < 0.0f ? ROMIS_PWC_NEG : 0u;
    const int e = (int)(iy >> 23 & 0xff);
    if (e < 0x7f) return c;
    if (e > 0x7f + 23) return c | ROMIS_PWC_INT;
    if (iy & ((1u << (0x7f + 23 - e)) - 1)) return c;
    return c | ((iy & (1u << (0x7f + 23 - e))) ? ROMIS_PWC_INT | ROMIS_PWC_ODD : ROMIS_PWC_INT);
}

struct Pending {
    int kernel;
    hipEvent_t start, stop;
};

}  // namespace

// Record buffers that temporal frames hand back (restir_frame_release): each comes with the events of the work
// that last touched it (the producing frame's kernels, every render that read it as a predecessor), so a context
// re-uses it by making its stream wait on those events -- no hipMalloc / hipFree / device-wide sync per frame.
struct FramePool {
    struct Entry {
        DevBuf buf;
        std::vector<hipEvent_t> busy;
    };
    std::mutex mu;
    std::vector<Entry> free;
    bool closed = false;   // the owning context is gone: returned buffers are freed
    int device = 0;
    // the owning context's stream (null once closed): its own later frames read a predecessor's records on it without
    // recording read events (used_prev), so a drain waits for that stream before the records are freed
    hipStream_t owner = nullptr;
    static void drain(Entry& e) {
        for (hipEvent_t ev : e.busy) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
        e.busy.clear();
        e.buf.release();
    }
    // a buffer of at least `bytes` whose past users `stream` now waits for; false: none pooled
    bool take(size_t bytes, hipStream_t stream, DevBuf& out) {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < free.size(); i++) {
            if (free[i].buf.bytes < bytes) continue;
            for (hipEvent_t ev : free[i].busy) {
                (void)hipStreamWaitEvent(stream, ev, 0);
                (void)hipEventDestroy(ev);   // released when the recorded work completes
            }
            out = free[i].buf;
            free.erase(free.begin() + (long)i);
            return true;
        }
        return false;
    }
    // own: an event recorded on the owning context's own stream (the frame's `ready`): the next taker, on that stream,
    // is ordered after it already -- no wait packet (a 5-10 us gap between kernels); only a drain needs it
    void give(DevBuf buf, std::vector<hipEvent_t> busy, hipEvent_t own = nullptr) {
        Entry e{buf, std::move(busy)};
        std::lock_guard<std::mutex> lk(mu);
        if (closed || free.size() >= 4) {
            if (own) e.busy.push_back(own);
            // a later frame of the owner may still be reading the buffer on its stream (no read event): wait for it
            // rather than rely on hipFree's implicit synchronisation
            if (!closed && owner) (void)hipStreamSynchronize(owner);
            drain(e);
            return;
        }
        if (own) (void)hipEventDestroy(own);   // released when the recorded work completes
        free.push_back(std::move(e));
    }
    void close() {
        std::lock_guard<std::mutex> lk(mu);
        closed = true;
        owner = nullptr;   // the context synchronised its stream before closing the pool
        for (Entry& e : free) drain(e);
        free.clear();
    }
};

struct restir_frame {
    std::atomic<int> refs{1};
    int device = 0;
    DevBuf rec;   // the frame's reservoirs over its view: per-pixel records [n_t, a_0, b_0, ...] or [a planes | b planes]
    bool records = true;
    uint32_t W = 0, H = 0, vx0 = 0, vy0 = 0, vw = 0, vh = 0, N = 0;
    // frame handles: the scene upload (restir_ctx::scene_gen) whose light table the sample handles at rec's tail
    // (W, M | light index << 24, after the reservoir planes) index; 0 = none written
    uint64_t hgen = 0;
    uint32_t hzero = 0;   // that table's light count: the index a handle names the zero sample by (restir_frame_reproject)
    std::shared_ptr<FramePool> pool;   // where rec goes back on release (the producing context's)
    std::mutex mu;
    hipEvent_t ready = nullptr;        // recorded on the producer's stream after its last kernel touching rec
    std::vector<hipEvent_t> reads;     // recorded after each render that read this frame as its predecessor
};

namespace {
hipEvent_t record_event(hipStream_t s) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventRecord(ev, s) != hipSuccess) { (void)hipEventDestroy(ev); return nullptr; }
    return ev;
}
// a frame's records leave the producing context: remember where they go back to and when they are written
restir_frame* make_frame(const std::shared_ptr<FramePool>& pool, int device, hipStream_t s) {
    restir_frame* fr = new restir_frame();
    fr->device = device;
    fr->pool = pool;
    fr->ready = record_event(s);
    return fr;
}
// the consumer of a predecessor frame: its stream waits for the producer's kernels (another context / stream; a frame
// of this context -- own, its pool, which the frame keeps alive -- was produced on this stream: ordered already)
restir_status use_prev(const restir_frame* prev, int device, hipStream_t s, const FramePool* own) {
    if (prev->device != device)
        return fail(RESTIR_ERR_INVALID, "temporal predecessor lives on device %d, this context on %d", prev->device, device);
    if (prev->ready && prev->pool.get() != own) HIP_TRY(hipStreamWaitEvent(s, prev->ready, 0));
    return RESTIR_OK;
}
// ... and records that it read it, so the records are not recycled under the read (the pool's taker is its own
// context, on this stream when the reader is that context: ordered already)
void used_prev(const restir_frame* prev, hipStream_t s, const FramePool* own) {
    if (prev->pool.get() == own) return;
    restir_frame* fr = const_cast<restir_frame*>(prev);
    hipEvent_t ev = record_event(s);
    if (!ev) { (void)hipStreamSynchronize(s); return; }
    std::lock_guard<std::mutex> lk(fr->mu);
    fr->reads.push_back(ev);
}
}  // namespace

// One snapshot slot of a context (restir_image_begin): the staging buffer the conversion writes and the copy reads, the
// pinned host buffer the copy lands in, and the two events -- `converted` on the context's stream, `landed` on its copy
// stream.  Buffers and events are created on first need and live until restir_destroy.
struct restir_image {
    restir_ctx* ctx = nullptr;
    bool in_use = false;
    uint32_t width = 0, height = 0, format = 0;
    size_t bytes = 0;                  // of this snapshot (<= stage.bytes, host_bytes)
    DevBuf stage;
    void* host = nullptr;              // hipHostMalloc
    size_t host_bytes = 0;
    hipEvent_t converted = nullptr, landed = nullptr;
};

struct restir_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;

    // presenting (restir_image_begin): the slots, and the stream their device-to-host copies run on -- created by the
    // first snapshot, so a program that takes none opens no second queue
    restir_image images[RESTIR_MAX_IMAGES_IN_FLIGHT];
    hipStream_t copy_stream = nullptr;

    // scene
    DevBuf nodes, tri_v0, tri_e1, tri_e2, tri_n0, tri_n1, tri_n2, materials, lights, light_c2, light_c4, light_col, tex_texels,
        tex_dims, tri_uv, nodes_q;
    SceneDev sdev{};
    bool has_scene = false;
    // Two generations, both unique per change: frame handles name the light table they index (restir_set_scene,
    // restir_set_lights), the kept G-buffer the geometry it was traced over (restir_set_scene, restir_update_meshes)
    uint64_t scene_gen = 0;
    uint64_t geom_gen = 0;
    // What restir_update_meshes needs of the upload (refit.h RefitDev): the vertices and the triangles' indices into
    // them, the tree's topology as static tables; per mesh, where its vertices lie and which of them a triangle uses
    DevBuf vpos, vnrm, tri_idx, tri_order, topo, node_range, level_nodes, level_start, refit_raw;
    struct MeshKeep {
        uint32_t first_vertex = 0, num_vertices = 0;
        std::vector<uint8_t> referenced;   // [num_vertices]: a triangle names the vertex
        bool normals_bounded = true;       // SceneDev::normals_bounded over the mesh's referenced vertices
    };
    std::vector<MeshKeep> mesh_keep;
    uint32_t bvh_levels = 0;
    bool topo_q_ok = false;            // the upload had quantized nodes (a refit keeps them unless its grid is not finite)
    // ... and restir_set_lights: the materials' and texels' part of shade_finite / miss_shade_zero
    double shade_kmax = 0.0;
    bool shade_k_finite = true, miss_mat_zero = true;

    // work buffers for one view
    uint32_t vw = 0, vh = 0, N = 0;
    DevBuf n_t, p_mat, ra[2], rb[2], dbg[2], rgb;   // stage API: SoA planes
    DevBuf uv;                                      // the G-buffer texCoord plane (textured scenes)
    DevBuf rec[2];                                  // restir_render / halo frames: per-pixel records
    std::shared_ptr<FramePool> pool = std::make_shared<FramePool>();
    DevBuf rp[2];                                   // their target-pdf cache planes (N = 1, planes layout)
    DevBuf vis;                                     // unbiased + visibility pass -> final shading: own-pixel ray
    DevBuf tmiss;                                   // RIS -> spatial passes / final shading: background tiles (MissTiles)
    uint32_t tmiss_w = 0, tmiss_h = 0;              // the last frame's computed region when it kept the flags (else 0)
    uint64_t last_px = 0;                           // the last frame's computed pixels
    DevBuf hnd[2];                                  // sample handles of rec[i] (N = 1 point lights, k_spatial1h)
    // restir_frame_reproject's own scratch: the G-buffer planes of the current (0) and the predecessor's (1) camera and
    // the map it downloads -- never the frame path's planes, so the kept G-buffer below stays as it is
    DevBuf rpj_nt[2], rpj_pm[2], rpj_map;
    // The view whose G-buffer n_t, p_mat, uv (textured scenes) and tile flags tmiss hold (tuning "gbuf.reuse"): written
    // after a restir_render frame's fused primary + RIS launch over the SoA planes.  They are a function of these
    // fields and nothing else -- the frame index and the RNG key do not enter -- so a later frame whose fields are
    // equal launches the k_gbuf_ris family over them (gbuf_reusable) instead of tracing the primary rays again.
    // Everything else that writes those buffers, or changes what a frame would write there, clears `valid`.
    struct GbufView {
        bool valid = false;
        uint64_t scene_gen = 0;
        uint32_t cam[9] = {};                      // CameraDev: quat, origin, half_w, half_h, as bits
        uint32_t width = 0, height = 0;
        restir_tile tile{};
        uint32_t tex_on = 0;
        uint32_t light_facts = 0;                  // what the tile flags take from the light list: any lights, all finite
        bool flags = false;                        // tmiss holds the view's flags
        uint32_t skip = 0;                         // the skip_res word the tracing frame ran with
        uint32_t map2d = 0, xcd_rows = 0, xcd_cols = 0, items = 0;   // the tile order the flags are indexed by
        const void *n_t = nullptr, *p_mat = nullptr, *uv = nullptr, *tmiss = nullptr;   // the buffers themselves
    } gbuf;
    uint64_t gbuf_reuses = 0;                       // frames that took the k_gbuf_ris family (restir_gbuf_reuses)
    uint64_t gbuf_epoch = 0;                        // counts the tracing frames that wrote `gbuf`: names one kept G-buffer
    // The shadow lists of the kept G-buffer (shadow_lists.h, tuning "final.lists"): the records in `slists`, valid for
    // what `key` names -- that G-buffer, the light table (scene_gen) and the geometry (geom_gen) -- and for the launch
    // `dev` describes (the last pass's rect, the tile flags, the cap).  Built by the second consecutive frame that
    // reuses the G-buffer with the lights unchanged (gbuf_streak counts them), so a client that moves its lights every
    // frame never pays for them; whatever drops the G-buffer, the lights or the geometry leaves the key stale.
    DevBuf slists;
    struct ShadowListsKey {
        bool valid = false;
        uint64_t gbuf_epoch = 0, scene_gen = 0, geom_gen = 0;
    } slists_key;
    ShadowListsDev slists_dev{};
    uint32_t gbuf_streak = 0;
    uint64_t gbuf_streak_lights = 0;                // scene_gen of the frames the streak counts
    uint64_t shadow_list_frames = 0;                // frames whose last pass took the lists route, its rays traced over the lists
                                                    // or answered from the bits below (restir_shadow_list_frames)
    uint64_t slists_builds = 0;                     // k_shadow_lists launches: names one build of the lists
    // The visibility bits of the lists' rays (shadow_vis.h, tuning "final.vis"): valid for the one build of the lists
    // they asked (`svis_lists_build`), hence for exactly what leaves those lists valid -- the same key, rect and flags.
    DevBuf svis;
    bool svis_valid = false;
    uint64_t svis_lists_build = 0;
    ShadowVisDev svis_dev{};
    uint64_t shadow_vis_frames = 0;                 // frames whose last pass read the bits (restir_shadow_vis_frames)
    uint64_t shadow_vis_builds = 0;                 // k_shadow_vis launches (restir_shadow_vis_builds)
    // The p-hat table of the kept G-buffer (phat_table.h, tuning "ris.phat"): RIS's target pdf of every (pixel, point
    // light), valid for what `phat_key` names -- that G-buffer, the light table and the materials (scene_gen) -- and for
    // the launch `phat_dev` describes (the view, the tile flags, L, Features::shading; tex_on is the view record's).
    DevBuf phat;
    struct PhatKey {
        bool valid = false;
        uint64_t gbuf_epoch = 0, scene_gen = 0;
    } phat_key;
    // a table the device had no memory for: not asked for again while it would be the same table
    struct PhatRefused {
        bool valid = false;
        uint64_t gbuf_epoch = 0, scene_gen = 0;
        size_t bytes = 0;
    } phat_refused;
    PhatTableDev phat_dev{};
    uint64_t phat_frames = 0;                       // frames whose RIS read the table (restir_phat_frames)
    uint64_t phat_builds = 0;                       // k_phat_table launches (restir_phat_builds)
    // RIS look-ahead (ris_ahead.h, tuning "frames.ahead"; DESIGN.md §6 "RIS look-ahead"): on a still view served by the
    // p-hat table without temporal reuse, frame f + 1's RIS runs on `stream` beside frame f's last pass and writes the
    // plane set frame f does not read -- set 0 is (hnd[0], rp[0]), set s >= 1 (hnd[s - 1], rp[s - 1]) here: 12 B a pixel of
    // the view each.  `ring` holds the results that are in (or on their way into) a set, each under its key; the next
    // restir_render takes the one whose key equals its own and launches no RIS, else marks them all invalid (discards)
    // and runs as if there had been none.  From the batch_after-th still frame on a launch serves two frames (frames.batch,
    // DESIGN.md §6 "RIS batch"): the ring then holds up to kRisRingSlots results in kRisSets sets.
    struct {
        uint32_t on = 1, after = 4, prio = 0;       // knobs frames.ahead (2: RIS enqueued before the last pass), _after, _prio
        uint32_t batch = 2, batch_after = 8;        // knobs frames.batch (keys per launch from that streak on), _after
        uint32_t batch_form = 1;                    // frames.batch_form: 0 a batch when nothing is pending, 1 when one result is (A/B)
        uint32_t serial = 0;                        // frames.ahead_serial: 1 the launch waits for the frame's last pass (kernel times alone)
        hipStream_t stream = nullptr;               // created by the first eligible frame, non-blocking
        uint32_t stream_prio = 0;                   // frames.ahead_prio the stream was created with
        DevBuf hnd[kRisSets - 1], rp[kRisSets - 1];   // sets 2 ..: allocated when a batch is first launched
        // done[s]: after the look-ahead launch whose last set is s; consumed[s]: after the last pass that read set s;
        // ready: on the frame's stream once the G-buffer and the table the launches read are final.  slot_done[i]: the
        // done event ring slot i's taker has yet to wait for, consumed_ev[s]: the one the next writer of set s has
        // (null: none, or everything before it was synchronised)
        hipEvent_t done[kRisSets] = {}, consumed[kRisSets] = {}, ready = nullptr;
        hipEvent_t slot_done[kRisRingSlots] = {}, consumed_ev[kRisSets] = {};
        bool ready_ok = false;
        uint64_t ready_epoch = 0, ready_build = 0;  // the G-buffer and table build `ready` was recorded behind
        RisRing ring;
        uint64_t tuning_gen = 0;
        uint64_t frames = 0, discards = 0;          // restir_ahead_frames, restir_ahead_discards
        // the event the next timed_begin's launch records as its stop event when it carries no timing pair
        hipEvent_t stop_hint = nullptr;
        hipStream_t stop_hint_stream = nullptr;
    } ahead;
    int cur = 0;
    uint32_t rgb_w = 0, rgb_h = 0;
    // Where the last image came from (restir_accum_add folds an image a producer wrote, and each once): rgb_serial counts
    // the images the producers wrote -- restir_render, the MIS tile renders, restir_halo_end, the stage path's final /
    // finish kernels and uploads of RESTIR_BUF_RGB --, rgb_from says what `rgb` holds now: nothing, the rgb_serial-th
    // image, a buffer that has its size but not yet its pixels (restir_halo_begin, restir_stage_configure, a frame
    // that failed half way), or a restir_accum_resolve's output
    enum RgbFrom : uint32_t { RGB_NONE = 0, RGB_PRODUCED = 1, RGB_PENDING = 2, RGB_RESOLVED = 3 };
    uint64_t rgb_serial = 0;
    uint32_t rgb_from = RGB_NONE;
    void image_pending(uint32_t w, uint32_t h) { rgb_w = w; rgb_h = h; rgb_from = RGB_PENDING; }
    void image_produced() { rgb_serial++; rgb_from = RGB_PRODUCED; }

    // accumulating frames (restir_accum_*, accum.h): the state planes, 3 floats per pixel of the first added image, and
    // the stats kernel's per-block partials.  `open` with frames == 0 holds no buffer yet.  None of the still view's
    // caches above is named here: no accumulation call touches them.
    struct {
        bool open = false;
        uint32_t flags = 0, frames = 0, width = 0, height = 0;
        uint64_t added_serial = 0;   // rgb_serial of the last image folded in
        DevBuf mean, m2, partials;
    } acc;

    // launch-shape knobs (restir_set_tuning)
    Tuning tuning{};

    // RNG
    uint32_t seed = RESTIR_DEFAULT_SEED;
    uint32_t frame_index = 0;

    // halo-mode frame in flight (restir_halo_begin .. restir_halo_end)
    struct {
        bool active = false;
        uint32_t W = 0, H = 0, frame = 0, pass = 0, passes = 0;
        Region view{}, owned{};
        FeaturesDev f{};
        CameraDev camd{};
        HaloSegs send{}, recv{};
        uint64_t send_bytes = 0, recv_bytes = 0;
        uint32_t send_rank[RESTIR_MAX_HALO_SEGS] = {}, recv_rank[RESTIR_MAX_HALO_SEGS] = {};
        restir_halo_op ops[2 * RESTIR_MAX_HALO_SEGS] = {};   // what restir_halo_pass posts (restir_halo_ops)
        uint32_t nops = 0;
        uint32_t rank = 0, nranks = 0;   // this frame's tile (rank) of tiles_x * tiles_y
        int cur = 0;
        bool fb_records = true;
        bool rp_ok = false;          // the current grid's target-pdf cache is valid (restir_render's rp_ok)
        bool interior_done = false;  // the current pass's interior launch is issued (restir_halo_spatial_interior)
        bool part_rp = false;        // every launch of the current pass wrote the pdf cache
        uint8_t* tmiss = nullptr;    // the view's background-tile flags (fused RIS over the view, no temporal reuse)
    } halo;
    DevBuf halo_scratch;
    // record-only restir_halo_pass (restir_halo_record): the steps it issues, no RCCL call
    bool halo_record = false;
    std::vector<restir_halo_event> halo_log;
    // native RCCL halo transport (restir_halo_attach_rccl / _comm, restir_halo_pass)
    struct {
        void* comm = nullptr;            // ncclComm_t
        bool owned = false;              // created by restir_halo_attach_rccl (destroyed with the context)
        hipStream_t stream = nullptr;    // communication stream
        hipEvent_t packed = nullptr, moved = nullptr;
        int nranks = 0, rank = -1;       // the communicator's size and this context's rank in it
        DevBuf send, recv;
    } rccl;

    // stage API region
    Region stage_rg{};
    bool stage_ok = false;

    // R-MIS / R-OMIS: neighbourhoods [1 + cap][pixels] and accumulators [rows][pixels] (RESTIR_BUF_MIS_*)
    DevBuf mis_nbr, mis_acc, mis_smp;
    uint32_t mis_cap = 0, mis_rows = 0, mis_smp_samples = 0;
    // file side outputs (restir_set_renders_dir): R-OMIS alpha visualisation words [3T][pixels]
    std::string renders_dir;
    DevBuf mis_vis;
    std::vector<uint32_t> mis_vis_host;

    // timing
    bool timing = false;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_events;
    double ms[RESTIR_K_COUNT] = {0};
    uint64_t launches[RESTIR_K_COUNT] = {0};
    uint64_t timing_seq[RESTIR_K_COUNT] = {0};   // launches seen per kernel (timing.every sampling)

    // The exact image and the error figures (restir_render_exact, restir_reference_*, restir_error_get; exact.h), behind
    // everything a frame reads.  restir_render_exact's own scratch: the G-buffer planes of its view -- never the frame
    // path's planes, so the kept G-buffer and what is built over it stay as they are.  ref: the kept reference, 3 floats
    // per pixel of the image it was copied from (ref_w x ref_h; no buffer: none), and k_error_stats' partials.
    DevBuf exact_nt, exact_pm, exact_uv;
    DevBuf ref, err_partials;
    uint32_t ref_w = 0, ref_h = 0;

    // restir_denoise (denoise.h), behind everything a frame reads like the exact image: the planes of its own view --
    // dn_nt (.., t), dn_pf (P, flat), dn_ga (g, material), dn_uv what the primary kernel writes for a textured scene --
    // valid for the view dn_key names, and the two images its levels alternate between.
    DevBuf dn_nt, dn_pf, dn_ga, dn_uv, dn_tmp[2];
    struct DenoiseKey {
        bool valid = false;
        uint64_t geom_gen = 0;
        uint32_t cam[9] = {};                      // CameraDev: quat, origin, half_w, half_h, as bits
        uint32_t width = 0, height = 0;
        restir_tile tile{};
    } dn_key;
    uint64_t dn_guide_builds = 0;                   // guide traces (restir_denoise_guide_builds)
    // restir_denoise_lum's variance planes, one float per pixel, which its levels alternate between; they live and die
    // with the guide planes.  dn_var_px != 0: dn_var[dn_var_last] holds the last call's final plane of that many pixels
    DevBuf dn_var[2];
    uint32_t dn_var_last = 0;
    size_t dn_var_px = 0;

    // the reprojected image history (restir_history_*, history.h), behind everything a frame reads like the denoiser,
    // whose guide planes give it the current view's records.  planes: two sets of three 16-byte planes of width x height
    // pixels (set k's (N, t), (mean, n), (S, material) at planes 3 k ..), sized by the first advance.  have: set `set`
    // holds what the last advance kept, for camera `cam` (false: the next advance is all reason 7).  added_serial is the
    // history's own "folded already" mark (rgb_serial of the last image folded; 0: none), apart from acc's.
    struct {
        bool open = false, have = false;
        uint32_t var_fused = 1;   // tuning history.var_fused: the variance plane in one launch (0: three)
        uint32_t gather = RESTIR_HISTORY_GATHER_NEAREST;   // restir_history_gather_set: outlives begin / end and resets
        restir_history_params params{};
        uint32_t width = 0, height = 0;
        int set = 0;
        uint64_t added_serial = 0;
        uint64_t advances = 0, resets = 0;
        restir_camera cam{};
        DevBuf planes, map;
    } hist;
    // the geometry changed (restir_set_scene, restir_update_meshes): the kept records describe surfaces that have moved
    void history_reset() {
        if (hist.open && hist.have) {
            hist.have = false;
            hist.resets++;
        }
    }
};

// ---------------------------------------------------------------------------------------------------------
// pure host helpers
extern "C" {

int restir_abi_version(void) { return RESTIR_ABI_VERSION; }

void restir_features_default(restir_features* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->ray_trace_mode = RESTIR_MODE_RESTIR;
    out->initial_light_samples = 32;
    out->num_samples_in_reservoir = 2;
    out->num_neighbours_to_sample = 5;
    out->spatial_resample_radius = 10;
    out->spatial_resampling_passes = 2;
    out->temporal_clamp_m = 20;
    out->initial_samples_visibility_check = 0;
    out->unbiased_combination = 0;
    out->spatial_reuse = 1;
    out->spatial_reuse_visibility_check = 0;
    out->temporal_reuse = 1;
    out->enable_shading = 1;
    out->enable_texture_mapping = 1;
    out->enable_tone_mapping = 1;
    out->gamma = 1.0f;
    out->exposure = 1.5f;
    out->neighbour_same_geometry = 1;
    out->use_progressive_romis = 0;
    out->save_alphas_visualisation = 1;
    out->neighbour_max_depth_difference_fraction = 0.10f;
    out->neighbour_max_normal_angle_difference_radians = 0.436332f;
    out->max_iterations_mis = 5;
    out->neighbour_selection_strategy = RESTIR_NEIGHBOURS_SIMILAR;
    out->mis_weight_rmis = RESTIR_MIS_EQUAL;
    out->progressive_update_mod = 1;
}

uint32_t restir_rng_key(uint32_t seed, uint32_t frame, uint32_t stage, uint32_t pass) {
    return mix32(mix32(mix32(seed ^ 0x9E3779B9u) + frame) ^ (stage * 0x01000193u + pass * 0x27D4EB2Fu));
}

uint32_t restir_rng_draw(uint32_t key, uint32_t global_pixel, uint32_t slot) {
    return draw(pix_state(key, global_pixel), slot);
}

// Trackball (trackball.cpp:20-29, 75-78, 105-114) with glm::quat(euler) (type_quat.inl:208-217) and
// quat * vec3 (type_quat.inl:347-354); plain float arithmetic, no contraction.
void restir_camera_derive(const restir_camera* cam, restir_camera_frame* out) {
    if (!cam || !out) return;
    float hh = std::tan(cam->fovy / 2.0f);
    float hw = cam->aspect * hh;
    float hx = cam->rotation[0] * 0.5f, hy = cam->rotation[1] * 0.5f, hz = cam->rotation[2] * 0.5f;
    float cx = std::cos(hx), cy = std::cos(hy), cz = std::cos(hz);
    float sx = std::sin(hx), sy = std::sin(hy), sz = std::sin(hz);
    float q[4];
    q[3] = cx * cy * cz + sx * sy * sz;
    q[0] = sx * cy * cz - cx * sy * sz;
    q[1] = cx * sy * cz + sx * cy * sz;
    q[2] = cx * cy * sz - sx * sy * cz;
    // v = (0, 0, -distance): uv = cross(q.xyz, v), uuv = cross(q.xyz, uv), v + ((uv * w) + uuv) * 2
    const float v[3] = {0.0f, 0.0f, -cam->distance};
    float uv[3] = {q[1] * v[2] - v[1] * q[2], q[2] * v[0] - v[2] * q[0], q[0] * v[1] - v[0] * q[1]};
    float uuv[3] = {q[1] * uv[2] - uv[1] * q[2], q[2] * uv[0] - uv[2] * q[0], q[0] * uv[1] - uv[0] * q[1]};
    for (int a = 0; a < 3; a++) {
        float r = v[a] + ((uv[a] * q[3]) + uuv[a]) * 2.0f;
        out->origin[a] = cam->look_at[a] + r;
    }
    std::memcpy(out->quat, q, sizeof(q));
    out->half_w = hw;
    out->half_h = hh;
}

}  // extern "C"

extern "C" {

restir_status restir_device_count(int* out) {
    if (!out) return fail(RESTIR_ERR_INVALID, "restir_device_count: null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out = 0; return fail(RESTIR_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *out = n;
    return RESTIR_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// context helpers
namespace {

restir_status check_features(const restir_features* f) {
    if (!f) return fail(RESTIR_ERR_INVALID, "features is NULL");
    if (f->ray_trace_mode > RESTIR_MODE_ROMIS)
        return fail(RESTIR_ERR_INVALID, "Unsupported ray-tracing render mode %u requested from entry point", f->ray_trace_mode);
    if (f->ray_trace_mode != RESTIR_MODE_RESTIR) {
        if (f->neighbour_selection_strategy > RESTIR_NEIGHBOURS_EQUAL_SIMILAR_DISSIMILAR)
            return fail(RESTIR_ERR_INVALID, "neighbourSelectionStrategy %u", f->neighbour_selection_strategy);
        if (f->ray_trace_mode == RESTIR_MODE_RMIS && f->mis_weight_rmis > RESTIR_MIS_BALANCE)   // render.cpp:94
            return fail(RESTIR_ERR_INVALID, "Unhandled MIS weight type: %u", f->mis_weight_rmis);
        if (f->ray_trace_mode == RESTIR_MODE_ROMIS && f->num_neighbours_to_sample + 1u > RESTIR_ROMIS_MAX_TECHNIQUES)
            return fail(RESTIR_ERR_UNSUPPORTED, "R-OMIS with %u neighbours: at most %u techniques per pixel",
                        f->num_neighbours_to_sample, RESTIR_ROMIS_MAX_TECHNIQUES);
        if (f->ray_trace_mode == RESTIR_MODE_ROMIS && f->use_progressive_romis && f->progressive_update_mod == 0)
            return fail(RESTIR_ERR_INVALID, "progressiveUpdateMod 0 (iteration %% 0)");
    }
    if (f->num_samples_in_reservoir < 1 || f->num_samples_in_reservoir > RESTIR_MAX_N)
        return fail(RESTIR_ERR_INVALID, "numSamplesInReservoir %u outside 1..%u", f->num_samples_in_reservoir, RESTIR_MAX_N);
    if (f->spatial_resample_radius > 4096) return fail(RESTIR_ERR_INVALID, "spatialResampleRadius too large");
    if (f->num_neighbours_to_sample > 4096) return fail(RESTIR_ERR_INVALID, "numNeighboursToSample too large");
    if (f->gamma == 0.0f && f->enable_tone_mapping) { /* 1/gamma = inf, as in the reference */ }
    return RESTIR_OK;
}

FeaturesDev to_dev(const restir_features* f) {
    FeaturesDev d{};
    d.M = f->initial_light_samples;
    d.N = f->num_samples_in_reservoir;
    d.K = f->num_neighbours_to_sample;
    d.R = f->spatial_resample_radius;
    d.clamp_m = f->temporal_clamp_m;
    d.initial_vis = f->initial_samples_visibility_check;
    d.unbiased = f->unbiased_combination;
    d.spatial_vis = f->spatial_reuse_visibility_check;
    d.shading = f->enable_shading;
    d.tone_map = f->enable_tone_mapping;
    d.texture = f->enable_texture_mapping;
    d.gamma = f->gamma;
    d.exposure = f->exposure;
    d.mode = f->ray_trace_mode;
    d.strategy = f->neighbour_selection_strategy;
    d.same_geom = f->neighbour_same_geometry;
    d.depth_frac = f->neighbour_max_depth_difference_fraction;
    d.normal_rad = f->neighbour_max_normal_angle_difference_radians;
    d.mis_weight = f->mis_weight_rmis;
    d.progressive = f->use_progressive_romis;
    d.prog_mod = f->progressive_update_mod;
    d.iterations = f->max_iterations_mis;
    return d;
}

}  // namespace

// The scene as one launch over a view of npx pixels sees it: the G-buffer texCoord plane (allocated for textured
// scenes; k_primary writes it, every target pdf reads it) and whether diffuseAlbedo reads the textures.
static restir_status scene_for(restir_ctx* c, const FeaturesDev& f, size_t npx, SceneDev& out, DevBuf* uv = nullptr);

namespace {

// neighbourhood capacity of generateResampleIndicesGrid's output (neighbour_selection.cpp:45-105): k + 1, or the
// whole window for the strategies whose size arithmetic can take every member of a class
uint32_t mis_capacity(const restir_features* f, uint32_t W, uint32_t H) {
    const uint32_t k1 = f->num_neighbours_to_sample + 1u;
    if (f->neighbour_selection_strategy == RESTIR_NEIGHBOURS_RANDOM || f->neighbour_selection_strategy == RESTIR_NEIGHBOURS_SIMILAR)
        return k1;
    const uint64_t side = 2ull * f->spatial_resample_radius + 1ull;
    const uint64_t win = std::min<uint64_t>(side, W) * std::min<uint64_t>(side, H);
    return win > k1 ? (uint32_t)win : k1;
}
uint32_t mis_acc_rows(const restir_features* f) {
    const uint32_t T = f->num_neighbours_to_sample + 1u;
    return f->ray_trace_mode == RESTIR_MODE_ROMIS ? T * T + 6u * T + 3u : 3u;
}
constexpr uint64_t kMisSampleBudget = 4ull << 30;   // bytes of R-OMIS per-sample scratch
// The neighbourhoods, accumulators and per-sample scratch of ow x oh pixels of a W x H image: the whole image, or a
// screen tile's owned rectangle (the capacity is the image's: a window is clipped to the image, not to the tile)
restir_status ensure_mis(restir_ctx* c, const restir_features* f, uint32_t W, uint32_t H, uint32_t ow, uint32_t oh) {
    if (f->ray_trace_mode == RESTIR_MODE_RESTIR) return fail(RESTIR_ERR_INVALID, "the MIS stages need rayTraceMode RMIS or ROMIS");
    const size_t npx = (size_t)ow * oh;
    c->mis_cap = mis_capacity(f, W, H);
    c->mis_rows = mis_acc_rows(f);
    ST_TRY(c->mis_nbr.ensure((size_t)(1u + c->mis_cap) * npx * 4));
    ST_TRY(c->mis_acc.ensure((size_t)c->mis_rows * npx * 4));
    c->mis_smp_samples = 0;
    if (f->ray_trace_mode == RESTIR_MODE_ROMIS) {
        // R-OMIS per-sample scratch (k_romis_samples -> k_romis_accum): T + 3 rows per sample, as many of the T x N
        // samples as fit kMisSampleBudget (or the mis.chunk knob) and keep one launch's items below 2^31
        const uint64_t T = f->num_neighbours_to_sample + 1ull, S = T * f->num_samples_in_reservoir;
        const uint64_t per = (T + 3ull) * npx * 4ull;
        uint64_t n = std::max<uint64_t>(1, std::min<uint64_t>(S, kMisSampleBudget / per));
        if (c->tuning.mis_chunk) n = std::min<uint64_t>(n, c->tuning.mis_chunk);
        n = std::min<uint64_t>(n, std::max<uint64_t>(1, ((1ull << 31) - 1ull) / std::max<uint64_t>(npx, 1)));
        c->mis_smp_samples = (uint32_t)n;
        ST_TRY(c->mis_smp.ensure((size_t)(n * per)));
    }
    return RESTIR_OK;
}
restir_status ensure_mis(restir_ctx* c, const restir_features* f, uint32_t W, uint32_t H) { return ensure_mis(c, f, W, H, W, H); }
// renderROMIS reads neighborhood[0..k] (render.cpp:155-181): every pixel's window must hold k candidates
restir_status check_romis_window(const restir_features* f, uint32_t W, uint32_t H) {
    if (f->ray_trace_mode != RESTIR_MODE_ROMIS || f->neighbour_selection_strategy == RESTIR_NEIGHBOURS_RANDOM) return RESTIR_OK;
    const uint64_t corner = std::min<uint64_t>((uint64_t)f->spatial_resample_radius + 1u, W) *
                            std::min<uint64_t>((uint64_t)f->spatial_resample_radius + 1u, H);
    if (corner - 1u < f->num_neighbours_to_sample)
        return fail(RESTIR_ERR_INVALID, "R-OMIS: a %ux%u image with radius %u leaves fewer than k = %u candidates in a corner window "
                                        "(the reference indexes past the neighbourhood)", W, H, f->spatial_resample_radius,
                    f->num_neighbours_to_sample);
    return RESTIR_OK;
}

restir_status ensure_work(restir_ctx* c, uint32_t vw, uint32_t vh, uint32_t N, bool debug) {
    const size_t npx = (size_t)vw * vh;
    ST_TRY(c->n_t.ensure(npx * 16));
    ST_TRY(c->p_mat.ensure(npx * 16));
    for (int i = 0; i < 2; i++) {
        ST_TRY(c->ra[i].ensure(npx * N * 16));
        ST_TRY(c->rb[i].ensure(npx * N * 16));
        if (debug) ST_TRY(c->dbg[i].ensure(npx * N * 8));
    }
    c->vw = vw; c->vh = vh; c->N = N;
    return RESTIR_OK;
}

// A timing event: read only by hipEventElapsedTime after hipStreamSynchronize (collect_timings), so it needs no
// system-scope release of its own -- with one, the timed kernel's completion waits for a cache writeback that
// showed as 6.7 us before and 4.6 us after the C2 spatial pass (profiles/r4/gap).
hipError_t timing_event_create(const restir_ctx* c, hipEvent_t* e) {
    return c->tuning.timing_fence ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableSystemFence);
}

restir_status timed_begin(restir_ctx* c, int kernel, Pending& p) {
    p.kernel = kernel;
    p.start = p.stop = nullptr;
    // (a launch without a timing pair records the look-ahead's event, if one is asked for, as its stop event)
    set_launch_events(nullptr, c->ahead.stop_hint);
    if (!c->timing || !((c->tuning.timing_mask >> kernel) & 1u)) return RESTIR_OK;
    if (c->tuning.timing_every > 1u && (c->timing_seq[kernel]++ % c->tuning.timing_every) != 0u) return RESTIR_OK;
    for (hipEvent_t* e : {&p.start, &p.stop}) {
        if (!c->free_events.empty()) { *e = c->free_events.back(); c->free_events.pop_back(); }
        else HIP_TRY(timing_event_create(c, e));
    }
    set_launch_events(p.start, p.stop);   // recorded by the launch itself (hipExtLaunchKernelGGL)
    return RESTIR_OK;
}

restir_status timed_end(restir_ctx* c, Pending& p, hipError_t launch_err) {
    const bool used = launch_events_used();
    set_launch_events(nullptr, nullptr);
    const hipEvent_t hint = c->ahead.stop_hint;
    c->ahead.stop_hint = nullptr;
    if (launch_err != hipSuccess) return fail(RESTIR_ERR_HIP, "kernel launch: %s", hipGetErrorString(launch_err));
    // the look-ahead's event where the dispatch did not carry it: a timed launch (its pair went instead), or none at all
    if (hint && (p.start || !used)) HIP_TRY(hipEventRecord(hint, c->ahead.stop_hint_stream));
    if (!p.start) return RESTIR_OK;
    if (!used) {   // nothing launched (empty region): the events were never recorded
        c->free_events.push_back(p.start);
        c->free_events.push_back(p.stop);
        return RESTIR_OK;
    }
    c->pending.push_back(p);
    return RESTIR_OK;
}

// Wait for everything the context has enqueued: its stream and the look-ahead's.  Every site where something the frame
// kernels read is about to change or be freed, or where the caller is told that the work is done, comes through here.
hipError_t sync_streams(restir_ctx* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (c->ahead.stream) {
        const hipError_t e2 = hipStreamSynchronize(c->ahead.stream);
        if (e == hipSuccess) e = e2;
    }
    // nothing is left to wait for
    for (hipEvent_t& ev : c->ahead.slot_done) ev = nullptr;
    for (hipEvent_t& ev : c->ahead.consumed_ev) ev = nullptr;
    return e;
}

// Drop the look-ahead results: mark them invalid (counted per launch) and wait for their launches -- nothing is cancelled.  For whatever
// changes what the launch read or will write outside restir_render: a seed, a knob, the stage and halo paths, a scene.
void ahead_drop(restir_ctx* c) {
    c->ahead.discards += ris_ring_drop(c->ahead.ring);
    if (c->ahead.stream) (void)hipStreamSynchronize(c->ahead.stream);
    for (hipEvent_t& ev : c->ahead.slot_done) ev = nullptr;
}

restir_status collect_timings(restir_ctx* c) {
    if (c->pending.empty()) return RESTIR_OK;
    HIP_TRY(sync_streams(c));
    for (Pending& p : c->pending) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, p.start, p.stop));
        c->ms[p.kernel] += ms;
        c->launches[p.kernel] += 1;
        c->free_events.push_back(p.start);
        c->free_events.push_back(p.stop);
    }
    c->pending.clear();
    return RESTIR_OK;
}

#define TIMED(ctx, kid, call)                                   \
    do {                                                        \
        Pending p_;                                             \
        ST_TRY(timed_begin((ctx), (kid), p_));                  \
        ST_TRY(timed_end((ctx), p_, (call)));                   \
    } while (0)

CameraDev camera_dev(const restir_camera* cam) {
    restir_camera_frame cf;
    restir_camera_derive(cam, &cf);
    CameraDev d{};
    d.quat = make_float4(cf.quat[0], cf.quat[1], cf.quat[2], cf.quat[3]);
    for (int a = 0; a < 3; a++) d.origin[a] = cf.origin[a];
    d.half_w = cf.half_w;
    d.half_h = cf.half_h;
    return d;
}

Region make_region(uint32_t W, uint32_t H, uint32_t vx0, uint32_t vy0, uint32_t vw, uint32_t vh, uint32_t rx0,
                   uint32_t ry0, uint32_t rw, uint32_t rh) {
    Region r{};
    r.W = W; r.H = H;
    r.vx0 = vx0; r.vy0 = vy0; r.vw = vw; r.vh = vh;
    r.rx0 = rx0; r.ry0 = ry0; r.rw = rw; r.rh = rh;
    r.ps = 1; r.js = vw * vh;   // SoA planes (the stage API's buffers)
    return r;
}

// The frame path keeps one record per pixel, [n_t, res_a_0, res_b_0, res_a_1, ...]: a neighbour's depth /
// normal test and its reservoir come from the same cache lines (the spatial pass's gathers touch one record
// instead of three planes).
Region with_records(Region r, uint32_t N) {
    r.ps = 1u + 2u * N;
    r.js = 2u;
    return r;
}

// Frame-path buffers in either layout (tuning "layout.records"): records = rec[i] holds [n_t, a_j, b_j] per
// pixel; planes = rec[i] holds N res_a planes then N res_b planes, n_t is the separate plane n_t.
struct FrameBufs {
    restir_ctx* c;
    bool records;
    size_t npx;
    uint32_t N;
    // the plane set grid 0's handles and pdf cache lie in (>= 1: restir_ctx::ahead's, a look-ahead result the frame took)
    int set0 = 0;
    const DevBuf& hnd(int i) const { return i == 0 && set0 ? c->ahead.hnd[set0 - 1] : c->hnd[i]; }
    float4* pm() const { return c->p_mat.as<float4>(); }
    DevBuf& rgb() const { return c->rgb; }
    DevBuf& uv() const { return c->uv; }
    DevBuf& vis() const { return c->vis; }
    // the sample-handle planes of rec[i]: W then M | index << 24, one 4-byte plane each (ensure_handles)
    Handles h(int i) const {
        float* w = hnd(i).as<float>();
        return w ? Handles{w, reinterpret_cast<uint32_t*>(w + npx)} : Handles{nullptr, nullptr};
    }
    // frame handles: the same planes at the tail of rec[i] (planes layout, ensure_records), handed on with the records to
    // the frame restir_render returns -- the next frame's fused temporal reuse reads them: N = 1 the W and M | index
    // planes (8 B / px, not 32), N = 2 the 16-byte handle records (not 64 B)
    Handles fh(int i) const {
        if (records || (N != 1 && N != 2)) return Handles{nullptr, nullptr};
        float* w = reinterpret_cast<float*>(c->rec[i].as<float4>() + 2 * N * npx);
        return Handles{w, N == 1 ? reinterpret_cast<uint32_t*>(w + npx) : nullptr};
    }
    const float* fhw(const restir_frame* f) const { return reinterpret_cast<const float*>(f->rec.as<float4>() + 2 * N * npx); }
    const uint32_t* fhm(const restir_frame* f) const {
        return N == 1 ? reinterpret_cast<const uint32_t*>(fhw(f) + npx) : nullptr;
    }
    float4* nt(int i) const { return records ? c->rec[i].as<float4>() : c->n_t.as<float4>(); }
    float4* ra(int i) const { return c->rec[i].as<float4>() + (records ? 1 : 0); }
    float4* rb(int i) const { return c->rec[i].as<float4>() + (records ? 2 : npx * N); }
    float4* nt2() const { return records ? c->rec[1].as<float4>() : nullptr; }
    // the target-pdf cache planes (N = 1 planes layout only)
    float* rp(int i) const { return (!records && N == 1) ? (i == 0 && set0 ? c->ahead.rp[set0 - 1] : c->rp[i]).as<float>() : nullptr; }
    const float4* pa(const restir_frame* f) const { return f->rec.as<float4>() + (records ? 1 : 0); }
    const float4* pb(const restir_frame* f) const { return f->rec.as<float4>() + (records ? 2 : npx * N); }
    Region region(Region r) const { return records ? with_records(r, N) : r; }
    // a launch that reads grid `in` (its G-buffer, reservoirs, pdf cache and handles) and writes grid `out`
    LaunchBufs bufs(const CameraDev& cam, uint32_t key, int in, int out) const {
        LaunchBufs b;
        b.key = key; b.cam = &cam; b.origin = cam.origin;
        b.n_t = nt(in); b.p_mat = pm(); b.n_t2 = nt2();
        b.ia = ra(in); b.ib = rb(in); b.oa = ra(out); b.ob = rb(out);
        b.rp_in = rp(in); b.rp_out = rp(out);
        b.hin = h(in); b.hout = h(out);
        b.rgb = c->rgb.as<float>();
        return b;
    }
};

restir_status ensure_records(restir_ctx* c, uint32_t vw, uint32_t vh, uint32_t N, FrameBufs& fb) {
    const size_t npx = (size_t)vw * vh;
    fb = FrameBufs{c, c->tuning.records != 0, npx, N};
    const hipStream_t st = c->stream;
    // the kept G-buffer (restir_ctx::gbuf) does not survive another view size or a reallocation
    const void* const old_nt = c->n_t.p;
    const void* const old_pm = c->p_mat.p;
    if (vw != c->vw || vh != c->vh) c->gbuf.valid = false;
    ST_TRY(c->p_mat.ensure(npx * 16));
    if (!fb.records) ST_TRY(c->n_t.ensure(npx * 16));
    if (c->n_t.p != old_nt || c->p_mat.p != old_pm) c->gbuf.valid = false;
    // (planes, N = 1: + the frame handles' two 4-byte planes and 16 B of slack; N = 2: + the 16-byte handle records and
    // 16 B; FrameBufs::fh)
    const size_t rec_bytes = npx * (fb.records ? 1u + 2u * N : 2u * N) * 16 +
                             (fb.records ? 0 : N == 1 ? npx * 8 + 16 : N == 2 ? npx * 16 + 16 : 0);
    DevBuf* rec = c->rec;
    for (int i = 0; i < 2; i++) {
        // a buffer handed to a frame comes back through the pool (stream-ordered against its past users)
        if (!rec[i].p && c->pool->take(rec_bytes, st, rec[i])) continue;
        ST_TRY(rec[i].ensure(rec_bytes));
    }
    if (!fb.records && N == 1)
        for (int i = 0; i < 2; i++) ST_TRY(c->rp[i].ensure(npx * 4));
    c->vw = vw; c->vh = vh; c->N = N;
    return RESTIR_OK;
}

// rect grown by g, clipped to the view
Region grow_rect(const Region& base, uint32_t g) {
    Region r = base;
    uint32_t x0 = base.rx0 > base.vx0 + g ? base.rx0 - g : base.vx0;
    uint32_t y0 = base.ry0 > base.vy0 + g ? base.ry0 - g : base.vy0;
    uint64_t x1 = std::min<uint64_t>((uint64_t)base.rx0 + base.rw + g, (uint64_t)base.vx0 + base.vw);
    uint64_t y1 = std::min<uint64_t>((uint64_t)base.ry0 + base.rh + g, (uint64_t)base.vy0 + base.vh);
    r.rx0 = x0; r.ry0 = y0; r.rw = (uint32_t)(x1 - x0); r.rh = (uint32_t)(y1 - y0);
    return r;
}

// A temporal predecessor fits the frame about to render tile t of a width x height image: its grid is the tile's computed
// region (`what`: the caller's word for it), and it was rendered with this context's buffer layout.  ghost_rule
// (restir_render with spatial passes): nor may the tile have a ghost zone -- the predecessor's is not recomputed.
restir_status check_prev(const restir_ctx* c, const restir_frame* prev, uint32_t N, const restir_tile& t, uint32_t width,
                         uint32_t height, const char* what, bool ghost_rule) {
    if (prev->N != N || prev->vw != t.gwidth || prev->vh != t.gheight || prev->vx0 != t.gx0 || prev->vy0 != t.gy0 ||
        prev->W != width || prev->H != height)
        return fail(RESTIR_ERR_INVALID, "temporal predecessor grid does not match this %s / N", what);
    const bool has_ghost = t.gwidth != t.width || t.gheight != t.height;
    if (has_ghost && ghost_rule)
        return fail(RESTIR_ERR_UNSUPPORTED, "temporal reuse on a ghost-zoned tile needs the predecessor's ghost zone: "
                                            "render such tiles with the halo-exchange stages (restir_halo_begin)");
    if (prev->records != (c->tuning.records != 0))
        return fail(RESTIR_ERR_INVALID, "temporal predecessor grid was rendered with the other buffer layout");
    return RESTIR_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
static restir_status scene_for(restir_ctx* c, const FeaturesDev& f, size_t npx, SceneDev& out, DevBuf* uv) {
    out = c->sdev;
    if (c->sdev.num_textures) {
        DevBuf& u = uv ? *uv : c->uv;
        ST_TRY(u.ensure(std::max<size_t>(npx, 1) * 8));
        out.gbuf_uv = u.as<float2>();
        out.tex_on = f.texture ? 1u : 0u;
    }
    return RESTIR_OK;
}

extern "C" {

restir_status restir_create(int device, restir_ctx** out) {
    if (!out) return fail(RESTIR_ERR_INVALID, "restir_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(RESTIR_ERR_NO_DEVICE, "no HIP device (%s)", hipGetErrorString(e));
    if (device < 0) device = 0;
    if (device >= n) return fail(RESTIR_ERR_NO_DEVICE, "device %d >= device count %d", device, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RESTIR_ERR_NO_DEVICE, "device %d is %s; libromis_amd is built for gfx950 only", device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    restir_ctx* c = new restir_ctx();
    c->device = device;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(RESTIR_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    c->pool->owner = c->stream;
    *out = c;
    return RESTIR_OK;
}

static void release_rccl(restir_ctx* c);   // (halo section)
static void release_images(restir_ctx* c);   // (presenting section)

// Free the shadow-list records (restir_ctx::slists): where nothing can read them again -- another scene, final.lists
// off, the context's end.  (hipFree waits for the kernels that read them.)  The visibility bits hold those records'
// answers and go with them.
static void drop_shadow_vis(restir_ctx* c) {
    c->svis_valid = false;
    c->svis.release();
}
// Free the p-hat table (restir_ctx::phat) where nothing can read it again: the kept G-buffer it was built over is
// replaced (a tracing frame), the lights or materials changed, another scene, a cap below its size, ris.phat off, the
// context's end.  (hipFree waits for the kernels that read it.)
static void drop_phat_table(restir_ctx* c) {
    if (c->phat.p) ahead_drop(c);   // a look-ahead launch may be reading it on the other stream
    c->phat_key.valid = false;
    c->phat.release();
}
static void drop_shadow_lists(restir_ctx* c) {
    c->slists_key.valid = false;
    c->slists.release();
    drop_shadow_vis(c);
}

void restir_destroy(restir_ctx* c) {
    if (!c) return;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        (void)hipSetDevice(c->device);
        (void)sync_streams(c);   // a look-ahead launch may still be in flight
        for (int i = 0; i < kRisSets - 1; i++) { c->ahead.hnd[i].release(); c->ahead.rp[i].release(); }
        for (DevBuf* b : {&c->vis, &c->tmiss, &c->hnd[0], &c->hnd[1], &c->rpj_nt[0], &c->rpj_nt[1], &c->rpj_pm[0], &c->rpj_pm[1],
                          &c->rpj_map, &c->acc.mean, &c->acc.m2, &c->acc.partials, &c->exact_nt, &c->exact_pm, &c->exact_uv,
                          &c->ref, &c->err_partials, &c->dn_nt, &c->dn_pf, &c->dn_ga, &c->dn_uv, &c->dn_tmp[0], &c->dn_tmp[1],
                          &c->dn_var[0], &c->dn_var[1], &c->hist.planes, &c->hist.map})
            b->release();
        drop_shadow_lists(c);
        drop_phat_table(c);
        for (DevBuf* b : {&c->nodes, &c->nodes_q, &c->tri_v0, &c->tri_e1, &c->tri_e2, &c->tri_n0, &c->tri_n1, &c->tri_n2,
                          &c->materials, &c->lights, &c->light_c2, &c->light_c4, &c->light_col, &c->tex_texels, &c->tex_dims, &c->tri_uv, &c->uv, &c->n_t, &c->p_mat, &c->ra[0], &c->ra[1], &c->rb[0], &c->rb[1],
                          &c->dbg[0], &c->dbg[1], &c->rgb, &c->halo_scratch, &c->rec[0], &c->rec[1], &c->rp[0], &c->rp[1]})
            b->release();
        for (Pending& p : c->pending) { (void)hipEventDestroy(p.start); (void)hipEventDestroy(p.stop); }
        for (hipEvent_t ev : c->free_events) (void)hipEventDestroy(ev);
        c->pool->close();   // frames still alive free their records themselves on release
        release_rccl(c);
        release_images(c);
        for (hipEvent_t ev : c->ahead.done) if (ev) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : c->ahead.consumed) if (ev) (void)hipEventDestroy(ev);
        if (c->ahead.ready) (void)hipEventDestroy(c->ahead.ready);
        if (c->ahead.stream) (void)hipStreamDestroy(c->ahead.stream);
        (void)hipStreamDestroy(c->stream);
    }
    delete c;
}

restir_status restir_set_seed(restir_ctx* c, uint32_t seed, uint32_t frame_index) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (ris_ring_pending(c->ahead.ring)) {   // keyed by the seed and frame index that were: dropped, whatever the new ones are
        HIP_TRY(hipSetDevice(c->device));
        ahead_drop(c);
    }
    c->seed = seed;
    c->frame_index = frame_index;
    return RESTIR_OK;
}

restir_status restir_set_renders_dir(restir_ctx* c, const char* dir) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    c->renders_dir = dir ? dir : "";
    return RESTIR_OK;
}

restir_status restir_set_scene(restir_ctx* c, const restir_mesh* meshes, uint32_t num_meshes, const restir_light* lights,
                               uint32_t num_lights) {
    return restir_set_scene_textured(c, meshes, num_meshes, lights, num_lights, nullptr, 0);
}

// regularLightGrid's layout (scene.cpp:5-28) recovered from a light grid's corners: light i = x * ny + y has its corner
// at (start + s01 * float(x)) + s02 * float(y), computed in float as the reference does.  start = light 0's corner;
// s01 / s02 per component from the corners of lights ny and 1 (their difference, then the nearest floats around it)
// and accepted only when they reproduce every light's corner bit for bit; ny = the first power-of-two divisor of
// the light count that works.  The RIS kernels' kLtRegular form then evaluates the same expression instead of
// reading the corner from the table.
struct RegularGrid {
    bool ok = false;
    uint32_t ny_log2 = 0;
    float start[3] = {0, 0, 0}, s01[3] = {0, 0, 0}, s02[3] = {0, 0, 0};
};
static float grid_corner(float start, float s01, float s02, uint32_t x, uint32_t y) {
    volatile float a = s01 * (float)x;   // float products and sums, no contraction (the reference's order)
    volatile float b = start + a;
    volatile float c = s02 * (float)y;
    return b + c;
}
static RegularGrid find_regular_grid(const std::vector<float>& lt, uint32_t L) {
    RegularGrid g;
    if (L < 2) return g;
    auto near_floats = [](float t, float* out) {   // t and its 64 float neighbours on either side
        int n = 0;
        out[n++] = t;
        float up = t, dn = t;
        for (int k = 0; k < 64; k++) {
            up = std::nextafter(up, INFINITY);
            dn = std::nextafter(dn, -INFINITY);
            out[n++] = up;
            out[n++] = dn;
        }
        return n;
    };
    for (uint32_t lg = 0; (1u << lg) <= L; lg++) {
        const uint32_t ny = 1u << lg, nx = L / ny;
        if (nx * ny != L) break;
        if (ny < 2) continue;
        bool all = true;
        float st[3], a01[3], a02[3];
        for (int cpt = 0; cpt < 3 && all; cpt++) {
            const float start = lt[cpt];
            float c01[129], c02[129];
            const int n01 = nx > 1 ? near_floats(lt[28 * ny + cpt] - start, c01) : (c01[0] = 0.0f, 1);
            const int n02 = near_floats(lt[28 * 1 + cpt] - start, c02);
            bool found = false;
            for (int i01 = 0; i01 < n01 && !found; i01++)
                for (int i02 = 0; i02 < n02 && !found; i02++) {
                    bool match = true;
                    for (uint32_t i = 0; i < L && match; i++) {
                        const float v = grid_corner(start, c01[i01], c02[i02], i >> lg, i & (ny - 1u));
                        match = std::memcmp(&v, &lt[28 * i + cpt], 4) == 0;
                    }
                    if (match) { found = true; st[cpt] = start; a01[cpt] = c01[i01]; a02[cpt] = c02[i02]; }
                }
            all = found;
        }
        if (all) {
            g.ok = true;
            g.ny_log2 = lg;
            for (int cpt = 0; cpt < 3; cpt++) {
                g.start[cpt] = st[cpt]; g.s01[cpt] = a01[cpt]; g.s02[cpt] = a02[cpt];
            }
            return g;
        }
    }
    return g;
}

static std::atomic<uint64_t> g_scene_gens{0};   // restir_ctx::scene_gen / geom_gen: never 0, never twice

static restir_status check_lights(const restir_light* lights, uint32_t num_lights) {
    for (uint32_t i = 0; i < num_lights; i++)
        if (lights[i].type > RESTIR_LIGHT_PARALLELOGRAM)
            return fail(RESTIR_ERR_INVALID, "light %u: bad type %u", i, lights[i].type);
    return RESTIR_OK;
}

// SceneDev::normals_bounded over one mesh: the normals [num_vertices][3] of the vertices its triangles name
static bool normals_bounded_of(const float* normals, const restir_ctx::MeshKeep& mk) {
    for (uint32_t v = 0; v < mk.num_vertices; v++)
        for (int a = 0; a < 3 && mk.referenced[v]; a++)
            if (!(std::fabs(normals[3 * (size_t)v + a]) <= 0x1p125f)) return false;
    return true;
}

// The light half of a scene upload (restir_set_scene*, restir_set_lights; lights checked by check_lights): the 7-row
// table, its compact forms and everything SceneDev derives from the lights.  The materials' part of the shading flags is
// the context's (shade_kmax, shade_k_finite, miss_mat_zero).  Synchronises the stream before it returns: the tables are
// host vectors.
static restir_status upload_lights(restir_ctx* c, const restir_light* lights, uint32_t num_lights) {
    // lights: 7 float4 records
    std::vector<float> lt(28 * std::max<uint32_t>(num_lights, 1), 0.0f);
    uint32_t types = 0;
    for (uint32_t i = 0; i < num_lights; i++) {
        const restir_light& l = lights[i];
        types |= 1u << l.type;
        float* o = &lt[28 * i];
        const float* src[7] = {l.p0, l.p1, l.p2, l.c0, l.c1, l.c2, l.c3};
        for (int r = 0; r < 7; r++) { std::memcpy(&o[4 * r], src[r], 12); o[4 * r + 3] = 0.0f; }
        o[3] = u2f(l.type);
    }
    ST_TRY(c->lights.upload(lt.data(), lt.size() * 4, c->stream));
    // the compact light table of the RIS kernels' point and grid forms (kernels.hip kLtPoint / kLtGrid): rows 0 and 3
    // of every record.  A light grid (the reference's regularLightGrid, scene.cpp:5-28): every light a parallelogram
    // with light 0's edges and one colour at all four of its corners, bit for bit.
    // Parallelograms with one colour at all four corners (kLtPgram: rows 0..3 of every record) are the
    // reference's default nightclub set (scene.cpp:30-66); a grid also shares light 0's edges.
    bool pgram = num_lights > 0 && types == (1u << RESTIR_LIGHT_PARALLELOGRAM);
    for (uint32_t i = 0; pgram && i < num_lights; i++) {
        const float* o = &lt[28 * i];
        pgram = std::memcmp(o + 16, o + 12, 3 * sizeof(float)) == 0 && std::memcmp(o + 20, o + 12, 3 * sizeof(float)) == 0 &&
                std::memcmp(o + 24, o + 12, 3 * sizeof(float)) == 0;
    }
    bool grid = pgram;
    for (uint32_t i = 0; grid && i < num_lights; i++) grid = std::memcmp(&lt[28 * i + 4], &lt[4], 8 * sizeof(float)) == 0;
    const RegularGrid reg = grid ? find_regular_grid(lt, num_lights) : RegularGrid{};
    std::vector<float> lc4(16 * std::max<uint32_t>(pgram ? num_lights : 1u, 1u), 0.0f);
    for (uint32_t i = 0; pgram && i < num_lights; i++) std::memcpy(&lc4[16 * i], &lt[28 * i], 64);
    ST_TRY(c->light_c4.upload(lc4.data(), lc4.size() * 4, c->stream));
    // two planes (SceneDev::light_c2): rows 0 of every light, then rows 3 -- a random light's 16-byte read from an LDS
    // copy then lands on one of 16 bank groups instead of 8 (32-byte records)
    std::vector<float> lc2(8 * std::max<uint32_t>(num_lights, 1), 0.0f);
    for (uint32_t i = 0; i < num_lights; i++) {
        std::memcpy(&lc2[4 * i], &lt[28 * i], 16);
        std::memcpy(&lc2[4 * (num_lights + i)], &lt[28 * i + 12], 16);
    }
    ST_TRY(c->light_c2.upload(lc2.data(), lc2.size() * 4, c->stream));
    std::vector<float> lcol(4 * std::max<uint32_t>(num_lights, 1), 0.0f);   // c0 of every light (kLtRegular)
    for (uint32_t i = 0; i < num_lights; i++) std::memcpy(&lcol[4 * i], &lt[28 * i + 12], 12);
    ST_TRY(c->light_col.upload(lcol.data(), lcol.size() * 4, c->stream));
    HIP_TRY(sync_streams(c));   // host vectors go out of scope

    SceneDev& s = c->sdev;
    s.lights = c->lights.as<float4>();
    s.num_lights = num_lights;
    s.light_types = types;
    s.light_c2 = c->light_c2.as<float4>();
    s.lights_grid = grid ? 1u : 0u;
    s.light_c4 = c->light_c4.as<float4>();
    s.lights_pgram = pgram ? 1u : 0u;
    s.lights_regular = reg.ok ? 1u : 0u;
    s.grid_ny_log2 = reg.ny_log2;
    s.grid_start = make_float4(reg.start[0], reg.start[1], reg.start[2], 0.0f);
    s.grid_s01 = make_float4(reg.s01[0], reg.s01[1], reg.s01[2], 0.0f);
    s.grid_s02 = make_float4(reg.s02[0], reg.s02[1], reg.s02[2], 0.0f);
    s.light_col = c->light_col.as<float4>();
    // w = p / (1/L) (light.cpp:80) equals p * L exactly when 1/L is a power of two
    s.light_scale = (num_lights && (num_lights & (num_lights - 1)) == 0) ? (float)num_lights : 0.0f;
    s.lights_finite = 1u;
    for (uint32_t i = 0; i < 28 * num_lights; i++)
        if (!std::isfinite(lt[i]) && (i % 4) != 3) s.lights_finite = 0u;
    // every product colour x kd / colour x ks stays finite (with a margin for the mix() rounding of segment /
    // parallelogram colours): shade() may then skip its per-component NaN tests for finite dotNL and pow
    {
        double cmax = 0.0;
        bool finite = c->shade_k_finite;
        for (uint32_t i = 0; i < num_lights; i++)
            for (int r = 3; r < 7; r++)
                for (int a = 0; a < 3; a++) {
                    const float v = lt[28 * i + 4 * r + a];
                    finite = finite && std::isfinite(v);
                    cmax = std::max(cmax, (double)std::fabs(v));
                }
        s.shade_finite = (finite && cmax * c->shade_kmax <= 0x1p120) ? 1u : 0u;
        s.miss_shade_zero = (s.lights_finite && cmax <= 0x1p126 && c->miss_mat_zero) ? 1u : 0u;
    }
    c->scene_gen = ++g_scene_gens;   // frame handles written so far name the table this one replaced
    return RESTIR_OK;
}

restir_status restir_set_scene_textured(restir_ctx* c, const restir_mesh* meshes, uint32_t num_meshes,
                                        const restir_light* lights, uint32_t num_lights, const restir_texture* textures,
                                        uint32_t num_textures) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (num_meshes && !meshes) return fail(RESTIR_ERR_INVALID, "meshes is NULL");
    if (num_lights && !lights) return fail(RESTIR_ERR_INVALID, "lights is NULL");
    if (num_textures && !textures) return fail(RESTIR_ERR_INVALID, "textures is NULL");
    for (uint32_t i = 0; i < num_textures; i++)
        if (!textures[i].width || !textures[i].height || !textures[i].rgb)
            return fail(RESTIR_ERR_INVALID, "texture %u: empty image", i);
    for (uint32_t m = 0; m < num_meshes; m++)
        if (meshes[m].material.kd_texture > num_textures)
            return fail(RESTIR_ERR_INVALID, "mesh %u: kd_texture %u of %u textures", m, meshes[m].material.kd_texture,
                        num_textures);
    std::lock_guard<std::mutex> lk(c->mu);
    c->gbuf.valid = false; ahead_drop(c);   // another scene: the kept G-buffer is not its view
    HIP_TRY(hipSetDevice(c->device));
    drop_shadow_lists(c);    // ... nor are the lists its triangles' (a scene they serve builds its own)
    drop_phat_table(c);      // ... nor the p-hat table its lights' and materials'

    // flatten triangles (mesh order = original index order, like the oracle)
    std::vector<BvhTriangle> tris;
    std::vector<float> n0, n1, n2;   // float4 records
    std::vector<float> tuv;          // 2 float4 per triangle: (t0.xy, t1.xy), (t2.xy, 0, 0)
    // restir_update_meshes' view of the same: all vertices back to back, per triangle its three indices into them + the mesh
    std::vector<float> vpos, vnrm;
    std::vector<uint32_t> tri_idx;
    std::vector<restir_ctx::MeshKeep> mesh_keep(num_meshes);
    for (uint32_t m = 0; m < num_meshes; m++) {
        const restir_mesh& mesh = meshes[m];
        if (mesh.num_triangles && (!mesh.positions || !mesh.normals || !mesh.triangles))
            return fail(RESTIR_ERR_INVALID, "mesh %u: null arrays", m);
        restir_ctx::MeshKeep& mk = mesh_keep[m];
        mk.first_vertex = (uint32_t)(vpos.size() / 3);
        mk.num_vertices = mesh.num_vertices;
        mk.referenced.assign(mesh.num_vertices, 0);
        if ((uint64_t)mk.first_vertex + mesh.num_vertices >= (1ull << 31))
            return fail(RESTIR_ERR_INVALID, "too many vertices");
        vpos.resize(vpos.size() + 3 * (size_t)mesh.num_vertices, 0.0f);
        vnrm.resize(vnrm.size() + 3 * (size_t)mesh.num_vertices, 0.0f);
        if (mesh.num_vertices && mesh.num_triangles) {   // (a mesh without triangles: its arrays are never read, as before)
            std::memcpy(&vpos[3 * (size_t)mk.first_vertex], mesh.positions, 12 * (size_t)mesh.num_vertices);
            std::memcpy(&vnrm[3 * (size_t)mk.first_vertex], mesh.normals, 12 * (size_t)mesh.num_vertices);
        }
        for (uint32_t i = 0; i < mesh.num_triangles; i++) {
            const uint32_t* t = &mesh.triangles[3 * i];
            if (t[0] >= mesh.num_vertices || t[1] >= mesh.num_vertices || t[2] >= mesh.num_vertices)
                return fail(RESTIR_ERR_INVALID, "mesh %u triangle %u: vertex index out of range", m, i);
            for (int k = 0; k < 3; k++) {
                mk.referenced[t[k]] = 1;
                tri_idx.push_back(mk.first_vertex + t[k]);
            }
            tri_idx.push_back(m);
            BvhTriangle bt;
            std::memcpy(bt.v0, &mesh.positions[3 * t[0]], 12);
            std::memcpy(bt.v1, &mesh.positions[3 * t[1]], 12);
            std::memcpy(bt.v2, &mesh.positions[3 * t[2]], 12);
            tris.push_back(bt);
            for (int k = 0; k < 3; k++) {
                std::vector<float>& dst = k == 0 ? n0 : (k == 1 ? n1 : n2);
                dst.insert(dst.end(), &mesh.normals[3 * t[k]], &mesh.normals[3 * t[k]] + 3);
                dst.push_back(k == 0 ? u2f(m) : 0.0f);
            }
            for (int k = 0; k < 3; k++) {
                tuv.push_back(mesh.texcoords ? mesh.texcoords[2 * t[k]] : 0.0f);
                tuv.push_back(mesh.texcoords ? mesh.texcoords[2 * t[k] + 1] : 0.0f);
            }
            tuv.push_back(0.0f);
            tuv.push_back(0.0f);
        }
    }
    if (tris.size() >= (1u << 24)) return fail(RESTIR_ERR_INVALID, "too many triangles (%zu)", tris.size());
    FlatBvh bvh = build_bvh(tris, c->tuning.bvh_max_leaf);
    const size_t T = tris.size();
    std::vector<float> v0(4 * std::max<size_t>(T, 1)), e1(v0.size()), e2(v0.size());
    for (size_t k = 0; k < T; k++) {
        const BvhTriangle& t = tris[bvh.tri_order[k]];
        for (int a = 0; a < 3; a++) {
            v0[4 * k + a] = t.v0[a];
            e1[4 * k + a] = t.v1[a] - t.v0[a];
            e2[4 * k + a] = t.v2[a] - t.v0[a];
        }
        v0[4 * k + 3] = u2f(bvh.tri_order[k]);
    }
    // materials: one per mesh + the miss material (value-initialised HitInfo: kd 0, ks 0, shininess 1)
    // 3 float4 per material: (kd, shininess), (ks, pow mode), (underflow threshold, exponent, transparency, 0)
    std::vector<float> mats(12 * (num_meshes + 1), 0.0f);
    auto put_material = [&](uint32_t m, const restir_material& mt) {
        float* o = &mats[12 * m];
        o[0] = mt.kd[0]; o[1] = mt.kd[1]; o[2] = mt.kd[2]; o[3] = mt.shininess;
        o[4] = mt.ks[0]; o[5] = mt.ks[1]; o[6] = mt.ks[2];
        uint32_t mode = ROMIS_POW_GLIBC;
        float thr = 0.0f;
        const double y = (double)mt.shininess;
        if (mt.ks[0] == 0.0f && mt.ks[1] == 0.0f && mt.ks[2] == 0.0f) {
            mode = ROMIS_POW_SKIP;
        } else if (std::isfinite(y) && y > 0.0) {
            // |x| < thr  =>  y * log2|x| < -150 (1 + 2^-20): glibc's powf takes its underflow exit
            // (ylogx <= -150, returns +-0, the sign for a negative base and an odd integer y); the margin
            // dwarfs the 2^-32 relative error of its log2 and the rounding of y * log2|x|
            thr = (float)std::exp2(-150.0 * (1.0 + 0x1p-20) / y);
            if ((double)thr > std::exp2(-150.0 * (1.0 + 0x1p-20) / y)) thr = std::nextafter(thr, 0.0f);
        }
        const uint32_t cls = pw_class(mt.shininess);
        if (mode == ROMIS_POW_GLIBC && !(cls & (ROMIS_PWC_SPECIAL | ROMIS_PWC_NEG)) && thr >= FLT_MIN) mode = ROMIS_POW_SIMPLE;
        o[7] = u2f(mode);
        o[8] = thr; o[9] = u2f(cls); o[10] = mt.transparency; o[11] = u2f(mt.kd_texture);
    };
    for (uint32_t m = 0; m < num_meshes; m++) put_material(m, meshes[m].material);
    {
        restir_material miss{};   // value-initialised HitInfo material: kd 0, ks 0, shininess 1, transparency 1
        miss.shininess = 1.0f;
        miss.transparency = 1.0f;
        put_material(num_meshes, miss);
    }
    ST_TRY(check_lights(lights, num_lights));
    if (n0.empty()) { n0.assign(4, 0.0f); n1.assign(4, 0.0f); n2.assign(4, 0.0f); }
    std::vector<float> nodes = bvh.nodes;
    if (nodes.empty()) nodes.assign(8, 0.0f);
    // the shadow rays' 16-byte nodes (bvh.h quantize_nodes)
    const QuantizedNodes qn = quantize_nodes(bvh);
    const std::vector<uint32_t>& nq = qn.words;
    const float* q_lo = qn.lo;
    const float* q_s = qn.s;
    const bool q_ok = qn.ok;

    HIP_TRY(sync_streams(c));   // previous frames (either slot) may still read the old scene
    ST_TRY(c->nodes.upload(nodes.data(), nodes.size() * 4, c->stream));
    ST_TRY(c->nodes_q.upload(nq.data(), nq.size() * 4, c->stream));
    ST_TRY(c->tri_v0.upload(v0.data(), v0.size() * 4, c->stream));
    ST_TRY(c->tri_e1.upload(e1.data(), e1.size() * 4, c->stream));
    ST_TRY(c->tri_e2.upload(e2.data(), e2.size() * 4, c->stream));
    ST_TRY(c->tri_n0.upload(n0.data(), n0.size() * 4, c->stream));
    ST_TRY(c->tri_n1.upload(n1.data(), n1.size() * 4, c->stream));
    ST_TRY(c->tri_n2.upload(n2.data(), n2.size() * 4, c->stream));
    ST_TRY(c->materials.upload(mats.data(), mats.size() * 4, c->stream));
    // textures: texels as float4, images back to back; (width, height, first texel, 0) per image
    std::vector<float> texels;
    std::vector<uint32_t> dims;
    double tmax = 0.0;
    bool tfinite = true;
    for (uint32_t i = 0; i < num_textures; i++) {
        const restir_texture& tx = textures[i];
        dims.insert(dims.end(), {tx.width, tx.height, (uint32_t)(texels.size() / 4), 0u});
        for (size_t k = 0; k < (size_t)tx.width * tx.height; k++) {
            for (int a = 0; a < 3; a++) {
                const float v = tx.rgb[3 * k + a];
                texels.push_back(v);
                tfinite = tfinite && std::isfinite(v);
                tmax = std::max(tmax, (double)std::fabs(v));
            }
            texels.push_back(0.0f);
        }
    }
    if (texels.size() / 4 >= 0xFFFFFFFFull) return fail(RESTIR_ERR_INVALID, "textures too large");
    if (texels.empty()) texels.assign(4, 0.0f);
    if (dims.empty()) dims.assign(4, 0u);
    if (tuv.empty()) tuv.assign(8, 0.0f);
    ST_TRY(c->tex_texels.upload(texels.data(), texels.size() * 4, c->stream));
    ST_TRY(c->tex_dims.upload(dims.data(), dims.size() * 4, c->stream));
    ST_TRY(c->tri_uv.upload(tuv.data(), tuv.size() * 4, c->stream));
    // restir_update_meshes' tables (refit.h RefitDev): the topology a refit keeps.  Preorder: node i's subtree is
    // [i, miss(i)), its triangles one contiguous range of BVH-order slots, its children i + 1 and miss(i + 1).
    const uint32_t NN = bvh.num_nodes;
    std::vector<uint32_t> topo(2 * std::max<size_t>(NN, 1), 0u), range(topo.size(), 0u), depth(std::max<size_t>(NN, 1), 0u);
    for (uint32_t i = NN; i-- > 0;) {
        const uint32_t miss = f2u(bvh.nodes[8 * (size_t)i + 3]), leaf = f2u(bvh.nodes[8 * (size_t)i + 7]);
        topo[2 * i] = miss; topo[2 * i + 1] = leaf;
        if (leaf) {
            range[2 * i] = leaf & 0xFFFFFFu; range[2 * i + 1] = leaf >> 24;
        } else {
            const uint32_t right = f2u(bvh.nodes[8 * (size_t)(i + 1) + 3]);
            range[2 * i] = range[2 * (i + 1)];
            range[2 * i + 1] = range[2 * (i + 1) + 1] + range[2 * right + 1];
        }
    }
    uint32_t levels = NN ? 1u : 0u;
    for (uint32_t i = 0; i < NN; i++)
        if (!topo[2 * i + 1]) {
            depth[i + 1] = depth[topo[2 * (i + 1)]] = depth[i] + 1u;
            levels = std::max(levels, depth[i] + 2u);
        }
    std::vector<uint32_t> level_start(levels + 1, 0u), level_nodes(std::max<size_t>(NN, 1), 0u);
    for (uint32_t i = 0; i < NN; i++) level_start[levels - 1u - depth[i] + 1u]++;   // level 0 = the deepest
    for (uint32_t l = 0; l < levels; l++) level_start[l + 1] += level_start[l];
    {
        std::vector<uint32_t> at(level_start.begin(), level_start.end() - 1);
        for (uint32_t i = 0; i < NN; i++) level_nodes[at[levels - 1u - depth[i]]++] = i;
    }
    std::vector<uint32_t> order = bvh.tri_order;
    if (order.empty()) order.assign(1, 0u);
    if (tri_idx.empty()) tri_idx.assign(4, 0u);
    if (vpos.empty()) { vpos.assign(3, 0.0f); vnrm.assign(3, 0.0f); }
    ST_TRY(c->vpos.upload(vpos.data(), vpos.size() * 4, c->stream));
    ST_TRY(c->vnrm.upload(vnrm.data(), vnrm.size() * 4, c->stream));
    ST_TRY(c->tri_idx.upload(tri_idx.data(), tri_idx.size() * 4, c->stream));
    ST_TRY(c->tri_order.upload(order.data(), order.size() * 4, c->stream));
    ST_TRY(c->topo.upload(topo.data(), topo.size() * 4, c->stream));
    ST_TRY(c->node_range.upload(range.data(), range.size() * 4, c->stream));
    ST_TRY(c->level_nodes.upload(level_nodes.data(), level_nodes.size() * 4, c->stream));
    ST_TRY(c->level_start.upload(level_start.data(), level_start.size() * 4, c->stream));
    if (!refit_fits_lds(NN, (uint32_t)T)) ST_TRY(c->refit_raw.ensure((size_t)NN * 32));
    HIP_TRY(sync_streams(c));   // host vectors go out of scope
    c->bvh_levels = levels;
    c->topo_q_ok = q_ok;
    for (uint32_t m = 0; m < num_meshes; m++) {
        restir_ctx::MeshKeep& mk = mesh_keep[m];
        mk.normals_bounded = normals_bounded_of(&vnrm[3 * (size_t)mk.first_vertex], mk);
    }
    c->mesh_keep = std::move(mesh_keep);

    SceneDev& s = c->sdev;
    s.nodes = c->nodes.as<float4>();
    s.num_nodes = bvh.num_nodes;
    s.nodes_q = c->nodes_q.as<uint4>();
    s.nodes_q_ok = q_ok ? 1u : 0u;
    s.q_lo = make_float4(q_lo[0], q_lo[1], q_lo[2], 0.0f);
    s.q_s = make_float4(q_s[0], q_s[1], q_s[2], 0.0f);
    s.tri_v0 = c->tri_v0.as<float4>();
    s.tri_e1 = c->tri_e1.as<float4>();
    s.tri_e2 = c->tri_e2.as<float4>();
    s.tri_n0 = c->tri_n0.as<float4>();
    s.tri_n1 = c->tri_n1.as<float4>();
    s.tri_n2 = c->tri_n2.as<float4>();
    s.num_tris = (uint32_t)T;
    s.materials = c->materials.as<float4>();
    s.num_materials = num_meshes + 1;
    s.tex_texels = c->tex_texels.as<float4>();
    s.tex_dims = c->tex_dims.as<uint4>();
    s.tri_uv = c->tri_uv.as<float4>();
    s.num_textures = num_textures;
    s.gbuf_uv = nullptr;   // per launch (scene_for)
    s.tex_on = 0u;
    // the materials' and texels' part of shade_finite and miss_shade_zero (upload_lights has the lights' part)
    {
        double kmax = 0.0;
        bool finite = true;
        for (uint32_t m = 0; m <= num_meshes; m++)
            for (int a : {0, 1, 2, 4, 5, 6}) {
                const float v = mats[12 * m + a];
                finite = finite && std::isfinite(v);
                kmax = std::max(kmax, (double)std::fabs(v));
            }
        c->shade_k_finite = finite && tfinite;   // texels are diffuse colours too
        c->shade_kmax = std::max(kmax, tmax);
        c->miss_mat_zero = true;
        for (int a : {0, 1, 2, 4, 5, 6}) c->miss_mat_zero = c->miss_mat_zero && mats[12 * num_meshes + a] == 0.0f;
    }
    ST_TRY(upload_lights(c, lights, num_lights));
    s.normals_bounded = 1u;
    for (const std::vector<float>* nv : {&n0, &n1, &n2})
        for (size_t i = 0; i < nv->size(); i++)
            if ((i % 4) != 3 && !(std::fabs((*nv)[i]) <= 0x1p125f)) s.normals_bounded = 0u;
    c->geom_gen = ++g_scene_gens;
    c->history_reset();
    c->has_scene = true;
    return RESTIR_OK;
}

static RefitDev refit_dev(const restir_ctx* c) {
    const SceneDev& s = c->sdev;
    RefitDev r{};
    r.num_nodes = s.num_nodes; r.num_tris = s.num_tris; r.q_ok = c->topo_q_ok ? 1u : 0u;
    r.vpos = c->vpos.as<float>(); r.vnrm = c->vnrm.as<float>();
    r.tri_idx = c->tri_idx.as<uint4>(); r.tri_order = c->tri_order.as<uint32_t>();
    r.topo = c->topo.as<uint2>(); r.range = c->node_range.as<uint2>();
    r.level_nodes = c->level_nodes.as<uint32_t>(); r.level_start = c->level_start.as<uint32_t>();
    r.levels = c->bvh_levels;
    r.nodes = c->nodes.as<float4>(); r.nodes_q = c->nodes_q.as<uint4>();
    r.tri_v0 = c->tri_v0.as<float4>(); r.tri_e1 = c->tri_e1.as<float4>(); r.tri_e2 = c->tri_e2.as<float4>();
    r.tri_n0 = c->tri_n0.as<float4>(); r.tri_n1 = c->tri_n1.as<float4>(); r.tri_n2 = c->tri_n2.as<float4>();
    r.raw = c->refit_raw.as<float4>();
    return r;
}

// New vertex positions (and normals) for meshes of the uploaded scene: the vertices go to the device and refit.hip's
// kernels recompute the triangle records, the boxes and the quantized nodes there, in stream order behind every frame
// enqueued so far.  The host reads back the root's padded box (32 bytes, the one synchronisation) for SceneDev's
// by-value quantization grid.
restir_status restir_update_meshes(restir_ctx* c, const restir_mesh_update* updates, uint32_t count) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (count && !updates) return fail(RESTIR_ERR_INVALID, "updates is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_update_meshes before restir_set_scene");
    if (count == 0) return RESTIR_OK;
    // the whole input is checked before anything changes
    std::vector<uint8_t> named(c->mesh_keep.size(), 0);
    bool any_normals = false;
    for (uint32_t u = 0; u < count; u++) {
        const restir_mesh_update& up = updates[u];
        if (up.mesh >= c->mesh_keep.size())
            return fail(RESTIR_ERR_INVALID, "update %u: mesh %u of %zu", u, up.mesh, c->mesh_keep.size());
        const restir_ctx::MeshKeep& mk = c->mesh_keep[up.mesh];
        if (up.num_vertices != mk.num_vertices)
            return fail(RESTIR_ERR_INVALID, "update %u: mesh %u was uploaded with %u vertices, not %u", u, up.mesh, mk.num_vertices,
                        up.num_vertices);
        if (named[up.mesh]) return fail(RESTIR_ERR_INVALID, "update %u: mesh %u named twice", u, up.mesh);
        named[up.mesh] = 1;
        if (up.num_vertices && !up.positions) return fail(RESTIR_ERR_INVALID, "update %u: positions is NULL", u);
        // finite positions: min / max are then independent of the order the device evaluates them in
        for (size_t i = 0; i < 3 * (size_t)up.num_vertices; i++)
            if (!std::isfinite(up.positions[i]))
                return fail(RESTIR_ERR_INVALID, "update %u: mesh %u vertex %zu has a non-finite position", u, up.mesh, i / 3);
        any_normals = any_normals || (up.normals && up.num_vertices);
    }
    HIP_TRY(hipSetDevice(c->device));
    c->gbuf.valid = false; ahead_drop(c);   // the kept G-buffer is the old geometry's: the next frame traces
    c->geom_gen = ++g_scene_gens;
    c->history_reset();
    for (uint32_t u = 0; u < count; u++) {
        const restir_mesh_update& up = updates[u];
        restir_ctx::MeshKeep& mk = c->mesh_keep[up.mesh];
        if (!up.num_vertices) continue;
        const size_t off = 12 * (size_t)mk.first_vertex, bytes = 12 * (size_t)up.num_vertices;
        HIP_TRY(hipMemcpyAsync(c->vpos.as<char>() + off, up.positions, bytes, hipMemcpyHostToDevice, c->stream));
        if (up.normals) {
            HIP_TRY(hipMemcpyAsync(c->vnrm.as<char>() + off, up.normals, bytes, hipMemcpyHostToDevice, c->stream));
            mk.normals_bounded = normals_bounded_of(up.normals, mk);
        }
    }
    SceneDev& s = c->sdev;
    const RefitDev r = refit_dev(c);
    HIP_TRY(launch_refit_triangles(r, any_normals, c->stream));
    HIP_TRY(launch_refit_boxes(r, c->stream));
    float root[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s.num_nodes) HIP_TRY(hipMemcpyAsync(root, c->nodes.p, sizeof(root), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_streams(c));   // the caller's arrays may be freed on return; the root box is here
    if (s.num_nodes) {
        // quantize_nodes' grid over the new padded root; its q_ok beyond the topology's is a finite grid
        FlatBvh rootb;
        rootb.num_nodes = 1;
        rootb.nodes.assign(root, root + 8);
        rootb.nodes[7] = u2f(1u << 24);   // (any leaf word that fits)
        const QuantizedNodes q = quantize_nodes(rootb);
        s.nodes_q_ok = (c->topo_q_ok && q.ok) ? 1u : 0u;
        if (s.nodes_q_ok) {
            s.q_lo = make_float4(q.lo[0], q.lo[1], q.lo[2], 0.0f);
            s.q_s = make_float4(q.s[0], q.s[1], q.s[2], 0.0f);
        }
    }
    if (any_normals) {
        s.normals_bounded = 1u;
        for (const restir_ctx::MeshKeep& mk : c->mesh_keep) s.normals_bounded = s.normals_bounded && mk.normals_bounded ? 1u : 0u;
    }
    return RESTIR_OK;
}

// Another light list over the same geometry: the tree, the triangle records and the kept G-buffer stay.
restir_status restir_set_lights(restir_ctx* c, const restir_light* lights, uint32_t num_lights) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (num_lights && !lights) return fail(RESTIR_ERR_INVALID, "lights is NULL");
    ST_TRY(check_lights(lights, num_lights));
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_set_lights before restir_set_scene");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(sync_streams(c));   // previous frames (either slot) may still read the old tables
    return upload_lights(c, lights, num_lights);
}

restir_status restir_debug_scene_download(restir_ctx* c, float* nodes, uint32_t* nodes_q, float* tri_v0, float* tri_e1,
                                          float* tri_e2, float* tri_n0, float* tri_n1, float* tri_n2) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_debug_scene_download before restir_set_scene");
    HIP_TRY(hipSetDevice(c->device));
    const SceneDev& s = c->sdev;
    const size_t nb = (size_t)s.num_nodes * 32, qb = s.nodes_q_ok ? (size_t)s.num_nodes * 16 : 0, tb = (size_t)s.num_tris * 16;
    const struct { void* dst; const void* src; size_t bytes; } copies[] = {
        {nodes, s.nodes, nb}, {nodes_q, s.nodes_q, qb}, {tri_v0, s.tri_v0, tb}, {tri_e1, s.tri_e1, tb},
        {tri_e2, s.tri_e2, tb}, {tri_n0, s.tri_n0, tb}, {tri_n1, s.tri_n1, tb}, {tri_n2, s.tri_n2, tb}};
    for (const auto& cp : copies)
        if (cp.dst && cp.bytes) HIP_TRY(hipMemcpyAsync(cp.dst, cp.src, cp.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

// visualiseAlphas (render_utils.cpp:189-243) of the accumulators so far: k_romis_vis_t{T} solves and colours the
// 3T images on the device, the host writes them to <renders dir>/<currentTime()>/ (utils.cpp:16-22's format).
static restir_status save_alphas_visualisation(restir_ctx* c, uint32_t W, uint32_t H, uint32_t T) {
    const size_t npx = (size_t)W * H, words = (size_t)3 * T * npx;
    ST_TRY(c->mis_vis.ensure(words * 4));
    HIP_TRY(launch_romis_vis(W, H, T, c->mis_acc.as<float>(), c->mis_vis.as<uint32_t>(), c->stream));
    c->mis_vis_host.resize(words);
    HIP_TRY(hipMemcpyAsync(c->mis_vis_host.data(), c->mis_vis.p, words * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const std::time_t now = std::time(nullptr);
    std::tm tm_local{};
    localtime_r(&now, &tm_local);
    char stamp[64];
    std::strftime(stamp, sizeof(stamp), "%d-%m-%Y %H-%M-%S", &tm_local);
    const std::filesystem::path dir = std::filesystem::path(c->renders_dir) / stamp;
    std::error_code ec;
    std::filesystem::create_directories(dir, ec);
    if (ec) return fail(RESTIR_ERR_INVALID, "alpha visualisation: cannot create %s: %s", dir.c_str(), ec.message().c_str());
    static const char* const kColour[3] = {"Red", "Green", "Blue"};   // enum Color (render_utils.cpp:238)
    for (uint32_t i = 0; i < T; i++)
        for (uint32_t ch = 0; ch < 3; ch++) {
            const std::filesystem::path file =
                dir / ("Distribution " + std::to_string(i) + " - " + kColour[ch] + ".bmp");
            if (!write_bmp_words(file.c_str(), W, H, c->mis_vis_host.data() + (size_t)(3 * i + ch) * npx))
                return fail(RESTIR_ERR_INVALID, "alpha visualisation: cannot write %s", file.c_str());
        }
    return RESTIR_OK;
}

// renderRMIS / renderROMIS (render.cpp:64-265) over the whole image; the caller holds c->mu.
static restir_status render_mis(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t W,
                                uint32_t H, float* out_rgb) {
    if (W == 0 || H == 0) return fail(RESTIR_ERR_INVALID, "empty image %ux%u", W, H);
    ST_TRY(check_romis_window(features, W, H));
    const FeaturesDev f = to_dev(features);
    c->gbuf.valid = false; ahead_drop(c);   // k_primary writes n_t / p_mat below
    ST_TRY(ensure_work(c, W, H, f.N, true));
    ST_TRY(ensure_mis(c, features, W, H));
    ST_TRY(c->rgb.ensure((size_t)W * H * 12));
    c->image_pending(W, H);
    c->stage_ok = false;   // the stage buffers now hold this render's state
    const CameraDev camd = camera_dev(cam);
    const Region view = make_region(W, H, 0, 0, W, H, 0, 0, W, H);
    const uint32_t frame = c->frame_index++;
    SceneDev s;
    ST_TRY(scene_for(c, f, (size_t)W * H, s));
    float4* nt = c->n_t.as<float4>();
    float4* pm = c->p_mat.as<float4>();
    LaunchBufs b;
    b.cam = &camd; b.origin = camd.origin; b.n_t = nt; b.p_mat = pm;
    b.oa = c->ra[0].as<float4>(); b.ob = c->rb[0].as<float4>(); b.dbg = c->dbg[0].as<float2>();
    TIMED(c, RESTIR_K_PRIMARY, launch_primary(route_primary(s, view, c->tuning), s, view, b, c->stream));
    Ask ris_ask;
    ris_ask.dbg = true;
    const Route ris = route_ris(s, view, f, c->tuning, ris_ask);
    TIMED(c, RESTIR_K_MIS, launch_mis_neighbours(s, W, H, f, restir_rng_key(c->seed, frame, RESTIR_STAGE_NEIGHBOURS, 0),
                                                 restir_rng_key(c->seed, frame, RESTIR_STAGE_NEIGHBOURS, 1), nt, pm,
                                                 c->mis_nbr.as<uint32_t>(), c->stream));
    HIP_TRY(hipMemsetAsync(c->mis_acc.p, 0, (size_t)c->mis_rows * W * H * 4, c->stream));
    for (uint32_t it = 0; it < features->max_iterations_mis; it++) {
        b.key = restir_rng_key(c->seed, frame, RESTIR_STAGE_RIS, it);
        TIMED(c, RESTIR_K_RIS, launch_ris(ris, s, view, f, b, c->stream));
        TIMED(c, RESTIR_K_MIS, launch_mis_accumulate(s, W, H, f, camd.origin, nt, pm, c->mis_nbr.as<uint32_t>(),
                                                     c->ra[0].as<float4>(), c->rb[0].as<float4>(), c->dbg[0].as<float2>(), it,
                                                     c->mis_acc.as<float>(), c->mis_smp.as<float>(), c->mis_smp_samples,
                                                     c->tuning, c->stream));
        if (f.mode == RESTIR_MODE_ROMIS && features->save_alphas_visualisation && !c->renders_dir.empty())
            ST_TRY(save_alphas_visualisation(c, W, H, f.K + 1u));   // render.cpp:227-229
    }
    TIMED(c, RESTIR_K_MIS, launch_mis_finish(W, H, f, c->mis_acc.as<float>(), c->rgb.as<float>(), c->stream));
    c->image_produced();
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, (size_t)W * H * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

// restir_render_mis_tile's argument checks, all decided on the host before any device work: the mode, the tile (t = the
// tile, or the whole image for a null one), its ghost ring and the image's R-OMIS window rule.
static restir_status mis_tile_check(const restir_features* features, uint32_t width, uint32_t height, const restir_tile* tile,
                                    restir_tile& t) {
    if (features->ray_trace_mode != RESTIR_MODE_RMIS && features->ray_trace_mode != RESTIR_MODE_ROMIS)
        return fail(RESTIR_ERR_INVALID, "restir_render_mis_tile needs rayTraceMode RMIS or ROMIS (restir_render renders ReSTIR tiles)");
    if (width == 0 || height == 0) return fail(RESTIR_ERR_INVALID, "empty image %ux%u", width, height);
    t = restir_tile{};
    if (tile) {
        t = *tile;
        if (t.global_width != width || t.global_height != height)
            return fail(RESTIR_ERR_INVALID, "tile global size %ux%u != %ux%u", t.global_width, t.global_height, width, height);
        if (t.width == 0 || t.height == 0 || (uint64_t)t.x0 + t.width > width || (uint64_t)t.y0 + t.height > height ||
            t.gx0 > t.x0 || t.gy0 > t.y0 || (uint64_t)t.gx0 + t.gwidth < (uint64_t)t.x0 + t.width ||
            (uint64_t)t.gy0 + t.gheight < (uint64_t)t.y0 + t.height || (uint64_t)t.gx0 + t.gwidth > width ||
            (uint64_t)t.gy0 + t.gheight > height)
            return fail(RESTIR_ERR_INVALID, "inconsistent tile");
    } else {
        t.global_width = width; t.global_height = height;
        t.width = width; t.height = height;
        t.gwidth = width; t.gheight = height;
    }
    // every owned pixel's window, clipped to the image, lies in the computed region (any strategy: Random's window is
    // the same radius) -- the tile kernels index the view planes with it
    const uint64_t g = features->spatial_resample_radius;
    const uint64_t gx0 = t.x0 > g ? t.x0 - g : 0u, gy0 = t.y0 > g ? t.y0 - g : 0u;
    const uint64_t gx1 = std::min<uint64_t>((uint64_t)t.x0 + t.width + g, width);
    const uint64_t gy1 = std::min<uint64_t>((uint64_t)t.y0 + t.height + g, height);
    if (t.gx0 > gx0 || t.gy0 > gy0 || (uint64_t)t.gx0 + t.gwidth < gx1 || (uint64_t)t.gy0 + t.gheight < gy1)
        return fail(RESTIR_ERR_INVALID, "tile ghost zone narrower than the resample radius %llu", (unsigned long long)g);
    return check_romis_window(features, width, height);   // a property of the image, not of the tile
}

static bool tile_is_whole_image(const restir_tile& t) {
    return t.x0 == 0 && t.y0 == 0 && t.width == t.global_width && t.height == t.global_height;
}

// renderRMIS / renderROMIS of the owned rectangle of tile t (mis_tile_check passed; not the whole image): primary rays and
// RIS over the ghost-zoned view, the neighbourhoods, accumulation, solves and screen over the owned pixels (mis.hip's
// tile kernels).  Consumes one frame index; the caller holds c->mu.
static restir_status render_mis_tile(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t W,
                                     uint32_t H, const restir_tile& t, float* out_rgb) {
    const FeaturesDev f = to_dev(features);
    if (f.mode == RESTIR_MODE_ROMIS && features->save_alphas_visualisation && !c->renders_dir.empty())
        return fail(RESTIR_ERR_UNSUPPORTED, "alpha visualisation on a screen tile: the per-distribution bitmaps are whole-image files");
    const size_t vpx = (size_t)t.gwidth * t.gheight, opx = (size_t)t.width * t.height;
    c->gbuf.valid = false; ahead_drop(c);   // k_primary writes n_t / p_mat below
    ST_TRY(ensure_work(c, t.gwidth, t.gheight, f.N, true));
    ST_TRY(ensure_mis(c, features, W, H, t.width, t.height));
    ST_TRY(c->rgb.ensure(opx * 12));
    c->image_pending(t.width, t.height);
    c->stage_ok = false;   // the stage buffers now hold this render's state
    const CameraDev camd = camera_dev(cam);
    const Region view = make_region(W, H, t.gx0, t.gy0, t.gwidth, t.gheight, t.gx0, t.gy0, t.gwidth, t.gheight);
    const MisTile mt{W, H, t.gx0, t.gy0, t.gwidth, t.gheight, t.x0, t.y0, t.width, t.height};
    const uint32_t frame = c->frame_index++;
    SceneDev s;
    ST_TRY(scene_for(c, f, vpx, s));
    float4* nt = c->n_t.as<float4>();
    float4* pm = c->p_mat.as<float4>();
    LaunchBufs b;
    b.cam = &camd; b.origin = camd.origin; b.n_t = nt; b.p_mat = pm;
    b.oa = c->ra[0].as<float4>(); b.ob = c->rb[0].as<float4>(); b.dbg = c->dbg[0].as<float2>();
    TIMED(c, RESTIR_K_PRIMARY, launch_primary(route_primary(s, view, c->tuning), s, view, b, c->stream));
    Ask ris_ask;
    ris_ask.dbg = true;
    const Route ris = route_ris(s, view, f, c->tuning, ris_ask);
    TIMED(c, RESTIR_K_MIS, launch_mis_neighbours(s, mt, f, restir_rng_key(c->seed, frame, RESTIR_STAGE_NEIGHBOURS, 0),
                                                 restir_rng_key(c->seed, frame, RESTIR_STAGE_NEIGHBOURS, 1), nt, pm,
                                                 c->mis_nbr.as<uint32_t>(), c->stream));
    HIP_TRY(hipMemsetAsync(c->mis_acc.p, 0, (size_t)c->mis_rows * opx * 4, c->stream));
    for (uint32_t it = 0; it < features->max_iterations_mis; it++) {
        b.key = restir_rng_key(c->seed, frame, RESTIR_STAGE_RIS, it);
        TIMED(c, RESTIR_K_RIS, launch_ris(ris, s, view, f, b, c->stream));
        TIMED(c, RESTIR_K_MIS, launch_mis_accumulate(s, mt, f, camd.origin, nt, pm, c->mis_nbr.as<uint32_t>(),
                                                     c->ra[0].as<float4>(), c->rb[0].as<float4>(), c->dbg[0].as<float2>(), it,
                                                     c->mis_acc.as<float>(), c->mis_smp.as<float>(), c->mis_smp_samples,
                                                     c->tuning, c->stream));
    }
    TIMED(c, RESTIR_K_MIS, launch_mis_finish(mt, f, c->mis_acc.as<float>(), c->rgb.as<float>(), c->stream));
    c->image_produced();
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, opx * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

// What both frame paths ask of primary rays + RIS over the view: the pdf cache where the layout has one, and
// background-tile flags (MissTiles; knob miss.tiles) -- not with temporal reuse (its output is not the RIS result); the
// spatial shortcuts also need bounded normals (their miss tests)
static Ask frame_ris_ask(const restir_ctx* c, const SceneDev& s, const FrameBufs& fb, bool temporal) {
    Ask a;
    a.rp_out = fb.rp(0) != nullptr;
    // (no lights: no tile's RIS result is the known miss -- the kernel would flag every tile 1 -- and a context that has
    // rendered a lit scene holds that scene's flags: the passes must not read any)
    a.flags = c->tuning.miss_tiles && !temporal && s.normals_bounded && !fb.records && s.num_lights != 0u;
    return a;
}

// The flags the fused primary + RIS kernel writes when its route says so: one byte per 32 x 8 tile of the view, in
// whole words (the spatial pass reads its flag's word)
static restir_status ensure_tile_flags(restir_ctx* c, const Route& ris, const Region& view, uint8_t*& flags) {
    flags = nullptr;
    if (!ris.flags) return RESTIR_OK;
    const size_t tiles = (size_t)((view.vw + 31u) / 32u) * ((view.vh + 7u) / 8u);
    ST_TRY(c->tmiss.ensure((tiles + 3u) & ~(size_t)3u));
    flags = c->tmiss.as<uint8_t>();
    return RESTIR_OK;
}

// What a frame's fused primary + RIS launch `ris` over tile t leaves in the G-buffer planes and the flags (restir_ctx::gbuf)
static restir_ctx::GbufView gbuf_view(const restir_ctx* c, const SceneDev& s, const CameraDev& cam, uint32_t width,
                                      uint32_t height, const restir_tile& t, const Route& ris, const uint8_t* tmiss) {
    restir_ctx::GbufView v;
    v.scene_gen = c->geom_gen;   // the planes hold geometry alone: another light list leaves them valid
    const float camf[9] = {cam.quat.x, cam.quat.y, cam.quat.z, cam.quat.w, cam.origin[0], cam.origin[1], cam.origin[2],
                           cam.half_w, cam.half_h};
    std::memcpy(v.cam, camf, sizeof(v.cam));
    v.width = width; v.height = height;
    v.tile = t;
    v.tex_on = s.tex_on;
    // a tile is flagged background when its pixels' RIS result is the known miss: with lights, and finite ones
    // (kernels.hip k_primary_ris); the G-buffer records themselves hold geometry alone
    v.light_facts = (s.num_lights != 0u ? 1u : 0u) | (s.lights_finite ? 2u : 0u);
    v.flags = ris.flags && tmiss != nullptr;
    v.skip = ris.skip;
    v.map2d = ris.map2d; v.xcd_rows = ris.xcd_rows; v.xcd_cols = ris.xcd_cols; v.items = ris.grid;
    v.n_t = c->n_t.p; v.p_mat = c->p_mat.p; v.uv = s.gbuf_uv; v.tmiss = v.flags ? tmiss : nullptr;
    return v;
}

// The planes hold view `have` (a frame that traced it); a frame that would trace `want` may read them instead when
// every field is equal but the flags and the skip word, where `have` must hold all `want` reads: the flags if it wants
// any, and background tiles' G-buffer records (skip bit 1: not stored) unless it skips them too.  (Bit 0, the
// reservoirs, are every frame's own.)
static bool gbuf_reusable(const restir_ctx::GbufView& have, const restir_ctx::GbufView& want) {
    const restir_tile &a = have.tile, &b = want.tile;
    return have.valid && have.scene_gen == want.scene_gen && !std::memcmp(have.cam, want.cam, sizeof(have.cam)) &&
           have.width == want.width && have.height == want.height && a.global_width == b.global_width &&
           a.global_height == b.global_height && a.gx0 == b.gx0 && a.gy0 == b.gy0 && a.gwidth == b.gwidth &&
           a.gheight == b.gheight && a.x0 == b.x0 && a.y0 == b.y0 && a.width == b.width && a.height == b.height &&
           have.tex_on == want.tex_on && have.light_facts == want.light_facts && have.map2d == want.map2d && have.xcd_rows == want.xcd_rows &&
           have.xcd_cols == want.xcd_cols && have.items == want.items && have.n_t == want.n_t && have.p_mat == want.p_mat &&
           have.uv == want.uv && (!want.flags || (have.flags && have.tmiss == want.tmiss)) &&
           (!(have.skip & 2u) || (want.skip & 2u));
}

// The shadow lists route `r` (the fused last pass over rect pr, Route::lists) reads: kept when they were built for this
// G-buffer, light table, geometry and launch, else built now, on the frame's stream ahead of the pass.
static restir_status ensure_shadow_lists(restir_ctx* c, const Route& r, const SceneDev& s, const Region& pr, const float4* p_mat,
                                         const uint8_t* tmiss, hipStream_t st) {
    ShadowListsDev d{};
    d.s = s;
    d.s.gbuf_uv = nullptr;   // (per launch, unread here: keeps the comparison below to what the lists depend on)
    d.rg = r.region(pr);
    d.p_mat = p_mat;
    d.mt = MissTiles{r.flags ? tmiss : nullptr, r.flags_m, r.gbuf};
    d.cap = std::min(std::max(c->tuning.final_lists_cap, 1u), kSlCap);
    const size_t bytes = (size_t)shadow_list_tiles(d.rg) * sl_stride(s.num_lights) * 16u;
    const restir_ctx::ShadowListsKey& k = c->slists_key;
    const ShadowListsDev& h = c->slists_dev;
    const bool same_launch = h.rg.vx0 == d.rg.vx0 && h.rg.vy0 == d.rg.vy0 && h.rg.vw == d.rg.vw && h.rg.vh == d.rg.vh &&
                             h.rg.rx0 == d.rg.rx0 && h.rg.ry0 == d.rg.ry0 && h.rg.rw == d.rg.rw && h.rg.rh == d.rg.rh &&
                             h.p_mat == d.p_mat && h.mt.flags == d.mt.flags && h.mt.m == d.mt.m && h.cap == d.cap &&
                             h.s.num_lights == s.num_lights && h.s.num_tris == s.num_tris && h.s.light_c2 == s.light_c2 &&
                             h.s.tri_v0 == s.tri_v0 && h.s.num_materials == s.num_materials;
    if (k.valid && c->slists.p && k.gbuf_epoch == c->gbuf_epoch && k.scene_gen == c->scene_gen && k.geom_gen == c->geom_gen &&
        same_launch)
        return RESTIR_OK;
    c->slists_key.valid = false;
    ST_TRY(c->slists.ensure(bytes));
    d.rec = c->slists.as<uint4>();
    HIP_TRY(launch_shadow_lists(d, st));
    c->slists_builds++;
    c->slists_dev = d;
    c->slists_key.valid = true;
    c->slists_key.gbuf_epoch = c->gbuf_epoch;
    c->slists_key.scene_gen = c->scene_gen;
    c->slists_key.geom_gen = c->geom_gen;
    return RESTIR_OK;
}

// The visibility bits route `r` (Route::bits) reads, after ensure_shadow_lists of the same frame: kept when they hold
// the answers of the lists as they stand -- the same build, so the same key, rect and flags -- else built now from
// those lists, on the frame's stream behind their build and ahead of the pass.
static restir_status ensure_shadow_vis(restir_ctx* c, hipStream_t st) {
    const ShadowListsDev& l = c->slists_dev;
    if (c->svis_valid && c->svis.p && c->svis_lists_build == c->slists_builds && c->svis_dev.lists.rec == l.rec) return RESTIR_OK;
    c->svis_valid = false;
    ST_TRY(c->svis.ensure(sv_size(l.rg.rw, l.rg.rh, l.s.num_lights) * sizeof(uint32_t)));
    ShadowVisDev d{l, c->svis.as<uint32_t>()};
    HIP_TRY(launch_shadow_vis(d, st));
    c->shadow_vis_builds++;
    c->svis_dev = d;
    c->svis_lists_build = c->slists_builds;
    c->svis_valid = true;
    return RESTIR_OK;
}

// The p-hat table a route with `phat` reads (k_gbuf_ris_n1_lds_pt_phat over view `rg`): kept when it was built for this
// G-buffer, light table, materials and launch, else built now, on the frame's stream ahead of RIS.  false in `ok`: no
// table (over ris.phat_max_mb, or no memory for it) -- the frame runs without it, which is no error.
static restir_status ensure_phat_table(restir_ctx* c, const SceneDev& s, const Region& rg, const FeaturesDev& f, const float* origin,
                                       const float4* n_t, const float4* p_mat, const uint8_t* tmiss, hipStream_t st, bool& ok) {
    ok = false;
    PhatTableDev d{};
    d.s = s;
    d.rg = rg;
    d.f = f;
    for (int i = 0; i < 3; i++) d.origin[i] = origin[i];
    d.n_t = n_t;
    d.p_mat = p_mat;
    d.tmiss = tmiss;
    const size_t bytes = pt_size(rg.vw, rg.vh, s.num_lights) * sizeof(float);
    if (bytes > (size_t)c->tuning.ris_phat_max_mb << 20) {
        drop_phat_table(c);   // (a table from before the cap was lowered)
        return RESTIR_OK;
    }
    const PhatTableDev& h = c->phat_dev;
    const bool same_launch = h.rg.W == rg.W && h.rg.H == rg.H && h.rg.vx0 == rg.vx0 && h.rg.vy0 == rg.vy0 && h.rg.vw == rg.vw &&
                             h.rg.vh == rg.vh && h.rg.ps == rg.ps && h.rg.map2d == rg.map2d && h.n_t == n_t && h.p_mat == p_mat &&
                             h.tmiss == tmiss && h.s.num_lights == s.num_lights && h.s.light_c2 == s.light_c2 &&
                             h.s.materials == s.materials && h.s.num_materials == s.num_materials && h.s.tex_on == s.tex_on &&
                             h.s.gbuf_uv == s.gbuf_uv && h.f.shading == f.shading &&
                             !std::memcmp(h.origin, d.origin, sizeof(d.origin));
    if (c->phat_key.valid && c->phat.p && c->phat_key.gbuf_epoch == c->gbuf_epoch && c->phat_key.scene_gen == c->scene_gen &&
        same_launch) {
        ok = true;
        return RESTIR_OK;
    }
    c->phat_key.valid = false;
    ahead_drop(c);   // the table is written or freed below: no look-ahead launch may still read it
    if (c->phat.bytes < bytes) {
        // a table that does not fit the device's memory is not an error: the frame evaluates its p-hats
        c->phat.release();
        restir_ctx::PhatRefused& no = c->phat_refused;
        if (no.valid && no.gbuf_epoch == c->gbuf_epoch && no.scene_gen == c->scene_gen && no.bytes == bytes) return RESTIR_OK;
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            no.valid = true;
            no.gbuf_epoch = c->gbuf_epoch;
            no.scene_gen = c->scene_gen;
            no.bytes = bytes;
            return RESTIR_OK;
        }
        no.valid = false;
        c->phat.p = p;
        c->phat.bytes = bytes;
    }
    d.tab = c->phat.as<float>();
    HIP_TRY(launch_phat_table(d, st));
    c->phat_builds++;
    c->phat_dev = d;
    c->phat_key.valid = true;
    c->phat_key.gbuf_epoch = c->gbuf_epoch;
    c->phat_key.scene_gen = c->scene_gen;
    ok = true;
    return RESTIR_OK;
}

}  // extern "C"

namespace {

// A restir_render frame's decisions, taken before it allocates or enqueues anything (plan_frame)
struct FramePlan {
    bool temporal = false;           // a predecessor is combined
    bool fused = false;              // same region: one kernel (kernels.hip k_primary_ris)
    bool temporal_fused = false;     // ... with temporal reuse inside it (k_primary_ris_n{1,2}_lds_pt_temporal)
    bool temporal_handles = false;   // ... which rebuilds the predecessor from its frame handles
    int hkind = -1;                  // the passes' sample-handle kind (spatial_handle_kind; -1: none)
    bool handles = false;            // the passes read and write sample handles (restir_ctx::hnd)
    bool frame_handles = false;      // the last pass writes the returned grid's handles for the next frame
    bool vis = false;                // the last pass's own-pixel shadow rays go on to final shading (a plane of the view)
    uint32_t skip_mode = 0;          // what of background tiles RIS need not store (Ask::skip)
    Route ris;                       // primary + RIS before handles and skip_mode were known: names the tile flags
    Ask ris_ask;                     // what the frame asks of primary + RIS (gbuf_cached: after the allocations)
    // the fused RIS kernel writes background-tile flags (ensure_tile_flags) that the passes and final shading read
    bool flags() const { return fused && !temporal_fused && ris.flags; }
};

// One restir_render frame: the request and what is derived from it, then what each step leaves for the next
struct Frame {
    restir_ctx* c;
    const restir_features* features;
    const restir_frame* prev;
    bool want_next;                  // the caller takes the frame's grid
    uint32_t width, height, N, passes, frame;   // frame: the index the RNG keys take
    restir_tile t;                   // the tile rendered: the caller's, or the whole image
    FeaturesDev f;
    hipStream_t st;
    FrameBufs fb;
    CameraDev camd;
    Region view, owned;
    SceneDev s;
    uint8_t *vis, *tmiss;            // alloc: the own-pixel ray plane and the tile flags, null where the plan has none
    Route last;                      // the route that produced grid cur (rp_out: its pdf cache holds its samples' pdfs)
    int cur;
    // ris_stage: the frame may run the next frame's RIS beside its last pass (restir_ctx::ahead) -- its own key, and its
    // RIS launch as routed, which the look-ahead repeats with the next frame's RNG key into the other plane set
    bool ahead_ok;
    uint32_t ahead_streak;   // the streak of reusing frames this one is in (the knobs *_after count it)
    RisAheadKey ahead_key;
    Route ahead_route;
    LaunchBufs ahead_b;

    Region pass_rect(uint32_t pass) const { return grow_rect(owned, (passes - 1u - pass) * f.R); }
    Ask pass_ask(const FramePlan& p, uint32_t pass, bool rp_ok) const {
        const bool is_last = pass + 1 == passes;
        Ask a;
        a.hin = p.handles ? p.hkind : -1;
        // a pass before the last is read by the next one's handles alone: no reservoir planes
        a.hout = p.handles ? (!is_last || p.frame_handles) : false;
        a.hout_dead = p.handles && !is_last;
        // every neighbour of this pass lies in the region the cache's producer covered (RIS / temporal: the whole view;
        // pass p - 1: the owned rect grown by (P - p) R)
        a.rp_in = a.rp_nb = rp_ok;
        // the last pass's pdf cache has no reader (final shading re-shades; the next frame's temporal pass evaluates its
        // own): not written
        a.rp_out = !is_last && fb.rp(0) != nullptr;
        a.vis = is_last && p.vis;
        a.flags = p.flags();
        // a background pixel holds M = f.M after RIS and after every biased pass; an unbiased pass sums its neighbours'
        // M, which only pass 0 knows
        a.flags_m = (!f.unbiased || pass == 0) ? f.M : 0u;
        a.gbuf = (p.skip_mode & 2u) ? 1u : 0u;
        // final shading inside the last pass (final.fuse), offered where launch_final would read the pass's grid
        // without an own-pixel ray plane; the last pass's rect is the owned rect (grow_rect(owned, 0)), also on
        // ghost-zoned tiles.  Without a returned grid nothing else reads that pass's reservoir planes (the stage and
        // halo paths keep their own buffers and the separate kernels): they are not stored
        a.fin = is_last && !p.vis;
        a.fin_dead = !want_next;
        return a;
    }
    restir_status alloc(const FramePlan& p);
    restir_status ris_stage(const FramePlan& p);
    restir_status ahead_prepare(const FramePlan& p, const Route& ris);
    restir_status ahead_planes(int sets);
    restir_status look_ahead();
    // every pending result marked invalid (counted per launch); this stream waits for their launches
    restir_status ahead_invalidate() {
        auto& a = c->ahead;
        for (int i = 0; i < kRisRingSlots; i++) {
            if (a.ring.slot[i].valid && a.slot_done[i]) HIP_TRY(hipStreamWaitEvent(st, a.slot_done[i], 0));
            a.slot_done[i] = nullptr;
        }
        a.discards += ris_ring_drop(a.ring);
        return RESTIR_OK;
    }
    void ahead_consumed_hint() {
        c->ahead.stop_hint = c->ahead.consumed_ev[fb.set0] = c->ahead.consumed[fb.set0];
        c->ahead.stop_hint_stream = st;
    }
    restir_status spatial_passes(const FramePlan& p);
    restir_status hand_off(const FramePlan& p, restir_frame** out_next, float* out_rgb);
};

// The tile a frame renders (the whole image for a null one), consistent with the image; its computed region must hold
// the ghost zone g = passes * radius the spatial passes read (clipped at the image border)
restir_status frame_tile(const restir_tile* tile, uint32_t width, uint32_t height, uint64_t g, restir_tile& t) {
    t = restir_tile{};
    if (tile) {
        t = *tile;
        if (t.global_width != width || t.global_height != height)
            return fail(RESTIR_ERR_INVALID, "tile global size %ux%u != %ux%u", t.global_width, t.global_height, width, height);
        if (t.width == 0 || t.height == 0 || t.x0 + t.width > width || t.y0 + t.height > height || t.gx0 > t.x0 ||
            t.gy0 > t.y0 || t.gx0 + t.gwidth < t.x0 + t.width || t.gy0 + t.gheight < t.y0 + t.height ||
            t.gx0 + t.gwidth > width || t.gy0 + t.gheight > height)
            return fail(RESTIR_ERR_INVALID, "inconsistent tile");
    } else {
        if (width == 0 || height == 0) return fail(RESTIR_ERR_INVALID, "empty image %ux%u", width, height);
        t.global_width = width; t.global_height = height;
        t.x0 = 0; t.y0 = 0; t.width = width; t.height = height;
        t.gx0 = 0; t.gy0 = 0; t.gwidth = width; t.gheight = height;
    }
    uint32_t gx0 = t.x0 > g ? (uint32_t)(t.x0 - g) : 0u, gy0 = t.y0 > g ? (uint32_t)(t.y0 - g) : 0u;
    uint64_t gx1 = std::min<uint64_t>((uint64_t)t.x0 + t.width + g, width);
    uint64_t gy1 = std::min<uint64_t>((uint64_t)t.y0 + t.height + g, height);
    if (t.gx0 > gx0 || t.gy0 > gy0 || (uint64_t)t.gx0 + t.gwidth < gx1 || (uint64_t)t.gy0 + t.gheight < gy1)
        return fail(RESTIR_ERR_INVALID, "tile ghost zone narrower than passes * radius = %llu", (unsigned long long)g);
    return RESTIR_OK;
}

// Pure host code over the frame's inputs: no HIP call, no allocation, nothing of the context written
FramePlan plan_frame(const Frame& fr) {
    const restir_ctx* c = fr.c;
    const SceneDev& s = fr.s;
    const FeaturesDev& f = fr.f;
    const restir_tile& t = fr.t;
    const uint32_t N = fr.N, passes = fr.passes;
    FramePlan p;
    p.temporal = fr.features->temporal_reuse && fr.prev != nullptr;
    p.ris_ask = frame_ris_ask(c, s, fr.fb, p.temporal);
    p.ris = route_primary_ris(s, fr.view, f, c->tuning, p.ris_ask);
    p.fused = c->tuning.fuse_primary_ris && p.ris.ok;
    // temporal reuse inside the fused kernel: the predecessor's reservoirs are combined while the RIS reservoirs are
    // still in registers (no store / reload, no G-buffer re-read, one launch less)
    p.temporal_fused = p.temporal && p.fused && route_primary_ris_temporal(s, fr.view, f, c->tuning, p.ris_ask).ok;
    // sample handles (k_spatial1h): N = 1 biased passes over a point-light scene, written by the fused RIS kernel and by
    // every pass but the last; 4 + 4 B per pixel and 16 B of slack (the planes are read a word at a time)
    // (point lights: two 4-byte planes; a regular light grid: one float4 plane, k_spatial1g)
    // With temporal reuse the passes read handles when the fused temporal kernel can rebuild the predecessor from its
    // frame handles (point lights, the same scene upload): every M then bounded by RIS's plus the clamp's
    const bool no_ghost = t.gwidth == t.width && t.gheight == t.height;
    p.temporal_handles = p.temporal_fused && no_ghost && fr.prev->hgen != 0 && fr.prev->hgen == c->scene_gen;
    // the M every sub-reservoir can hold entering the passes after temporal reuse: the current M plus each of the N
    // predecessor sub-reservoirs clamped to clampM M + 1 (kernels.hip ris_pixel TEMP)
    const uint64_t m_temporal = (uint64_t)f.M + (uint64_t)N * ((uint64_t)f.clamp_m * f.M + 1u);
    p.hkind = (!p.fused || (p.temporal && !p.temporal_handles))
                  ? -1
                  : spatial_handle_kind(s, fr.view, f, c->tuning, passes, p.temporal ? m_temporal : 0u);
    p.handles = p.hkind >= 0 && (!p.temporal || p.hkind == 0 || p.hkind == 2);
    // the last pass also writes the returned grid's handles (point lights, no ghost ring) for the next frame, bounded as
    // if that frame's temporal reuse had run (its M bound)
    p.frame_handles = p.handles && (p.hkind == 0 || p.hkind == 2) && fr.want_next && no_ghost &&
                      spatial_handle_kind(s, fr.view, f, c->tuning, passes, m_temporal) == p.hkind;
    // the last pass's own-pixel shadow rays (unbiased + visibility reuse, N = 1) go on to final shading
    p.vis = passes && fr.features->unbiased_combination && fr.features->spatial_reuse_visibility_check && N == 1;
    if (p.flags() && passes > 0 && no_ghost) {
        // the first spatial pass substitutes a background tile's known reservoirs (Route::bg_known); the later passes and
        // final shading read the passes' outputs, and with no ghost ring the last pass overwrites the whole returned
        // grid: RIS need not store those reservoirs
        const bool skip_res = route_spatial(s, fr.pass_rect(0), f, c->tuning, fr.pass_ask(p, 0, p.ris.rp_out)).bg_known;
        // a single unbiased pass (k_spatial1u) also substitutes a background pixel's G-buffer records (own and the Z
        // loop's neighbours); final shading writes background tiles from the flags without reading them (its tiles are
        // the RIS tiles here): nor are those stored.  Biased passes (every pass reads the flags) fix their window up
        // instead (MissTiles::gbuf); knob miss.gbuf.
        const uint32_t mg = c->tuning.miss_gbuf;
        Ask with_flags;
        with_flags.flags = true;
        const bool gbuf_ok = mg && route_final(s, fr.owned, f, c->tuning, with_flags).flags &&
                             (f.unbiased ? passes == 1u : (mg == 1u || t.gwidth >= 2048u));
        p.skip_mode = skip_res ? (1u | (gbuf_ok ? 2u : 0u)) : 0u;
    }
    // the handle passes read RIS's samples through the handles alone, and a pass's output is read by the next pass's
    // handles alone: their reservoir planes are dead (the last pass writes the returned grid's owned rect; a tile's
    // ghost ring holds intermediate values, include/restir_c.h)
    p.ris_ask.hout = p.ris_ask.hout_dead = p.handles;
    p.ris_ask.skip = p.skip_mode;
    return p;
}

// What the plan needs allocated: the handle planes, the own-pixel ray plane, the tile flags
restir_status Frame::alloc(const FramePlan& p) {
    if (p.handles)
        for (int i = 0; i < 2; i++) ST_TRY(c->hnd[i].ensure((size_t)t.gwidth * t.gheight * (p.hkind ? 16u : 8u) + 16u));
    if (p.vis) {
        ST_TRY(fb.vis().ensure((size_t)t.gwidth * t.gheight));
        vis = fb.vis().as<uint8_t>();
    }
    if (p.fused && !p.temporal_fused) ST_TRY(ensure_tile_flags(c, p.ris, view, tmiss));
    return RESTIR_OK;
}

// Primary rays + RIS (+ temporal reuse) over the view into grid 0, in one of three launch shapes, and the kept
// G-buffer's bookkeeping
restir_status Frame::ris_stage(const FramePlan& p) {
    Ask ris_ask = p.ris_ask;
    Route& ris = last;
    LaunchBufs b = fb.bufs(camd, restir_rng_key(c->seed, frame, RESTIR_STAGE_RIS, 0), 0, cur);
    b.flags = tmiss;
    auto route_fused = [&](const Ask& a) {
        return p.temporal_fused ? route_primary_ris_temporal(s, view, f, c->tuning, a)
                                : route_primary_ris(s, view, f, c->tuning, a);
    };
    // the view this frame's fused kernel would leave in the G-buffer planes; when they hold it already (the static
    // camera of the reference's viewer loop), the k_gbuf_ris family runs over them instead (tuning "gbuf.reuse")
    restir_ctx::GbufView gv;
    if (p.fused) {
        ris = route_fused(ris_ask);
        gv = gbuf_view(c, s, camd, width, height, t, ris, tmiss);
        ris_ask.gbuf_cached = c->tuning.gbuf_reuse && !fb.records && gbuf_reusable(c->gbuf, gv);
        if (ris_ask.gbuf_cached) {
            // ... and from the ris.phat_after-th such frame with the lights unchanged on, its candidates' target pdfs
            // from the view's p-hat table (ris.phat); this frame's streak is the last one's + 1 (below)
            const uint32_t streak = c->gbuf_streak_lights == c->scene_gen ? c->gbuf_streak + 1u : 1u;
            ris_ask.phat = streak >= c->tuning.ris_phat_after;
            ris = route_fused(ris_ask);
            if (ris.phat) {
                bool have = false;
                ST_TRY(ensure_phat_table(c, s, ris.region(view), f, b.origin, b.n_t, b.p_mat, ris.flags ? tmiss : nullptr, st, have));
                if (have) {
                    b.phat = c->phat.as<float>();
                    c->phat_frames++;
                } else {
                    ris_ask.phat = false;
                    ris = route_fused(ris_ask);
                }
            }
        }
    } else {
        ris = route_ris(s, view, f, c->tuning, ris_ask);
    }
    // RIS look-ahead (frames.ahead): a frame of a still view served by the table, without temporal reuse, whose passes
    // read RIS's handles and pdf cache alone (the reservoir planes are dead) takes its RIS result from the look-ahead
    // the last frame launched when that result is keyed as this frame is, and launches the next frame's behind its own
    // last pass.  Any other frame, and a result keyed otherwise, runs exactly as without: the result is marked invalid
    // and this stream waits for its launch.
    bool took = false;
    const uint32_t streak_now = c->gbuf_streak_lights == c->scene_gen ? c->gbuf_streak + 1u : 1u;
    ahead_streak = streak_now;
    if (c->ahead.on && p.fused && !p.temporal && p.handles && ris.phat && b.phat && ris.kernel == Kernel::kGbufRis &&
        ris.res_dead && ris.hom && ris.rp_out && !ris.dbg && !fb.records && streak_now >= c->ahead.after) {
        ST_TRY(ahead_prepare(p, ris));
        auto& a = c->ahead;
        const int slot = ris_ring_find(a.ring, ahead_key);
        if (slot >= 0) {
            if (a.slot_done[slot]) HIP_TRY(hipStreamWaitEvent(st, a.slot_done[slot], 0));
            a.slot_done[slot] = nullptr;
            ris_ring_take(a.ring, slot);
            a.frames++;
            fb.set0 = a.ring.slot[slot].set;
            took = true;
            // what still waits is the frames' after this one, in order; anything else is stale: all of it goes
            const int n = ris_ring_pending(a.ring);
            bool chain = true;
            for (int i = 1; i <= n; i++) chain = chain && ris_ring_find(a.ring, ris_ahead_nth(ahead_key, (uint32_t)i)) >= 0;
            if (!chain) ST_TRY(ahead_invalidate());
        }
    }
    if (!took) ST_TRY(ahead_invalidate());
    // kept by a frame that reuses it; a frame that traces replaces it once its launch is issued (any error return in
    // between leaves none)
    if (!ris_ask.gbuf_cached) c->gbuf.valid = false;
    // the p-hat table goes with the G-buffer, the lights and the materials it was built from: a context that paused once
    // and moves on does not keep its memory
    if (c->phat.p && (!ris_ask.gbuf_cached || c->phat_key.scene_gen != c->scene_gen)) drop_phat_table(c);
    if (p.temporal_fused) {
        ST_TRY(use_prev(prev, c->device, st, c->pool.get()));   // the predecessor's records are complete (its producer's stream)
        b.tin = TemporalIn{fb.pa(prev), fb.pb(prev), restir_rng_key(c->seed, frame, RESTIR_STAGE_TEMPORAL, 0),
                           p.handles ? fb.fhw(prev) : nullptr, p.handles ? fb.fhm(prev) : nullptr};
        TIMED(c, RESTIR_K_PRIMARY_RIS, launch_primary_ris(ris, s, view, f, b, st));
        used_prev(prev, st, c->pool.get());
    } else if (p.fused) {
        if (ahead_ok) {
            ahead_route = ris;
            ahead_b = b;
        }
        if (!took) TIMED(c, RESTIR_K_PRIMARY_RIS, launch_primary_ris(ris, s, view, f, b, st));   // (took: grid 0 is the look-ahead's)
    } else {
        TIMED(c, RESTIR_K_PRIMARY, launch_primary(route_primary(s, view, c->tuning), s, view, b, st));
        TIMED(c, RESTIR_K_RIS, launch_ris(ris, s, view, f, b, st));
    }
    if (ris_ask.gbuf_cached) {
        c->gbuf_reuses++;
        c->gbuf_streak = c->gbuf_streak_lights == c->scene_gen ? c->gbuf_streak + 1u : 1u;
    } else {
        c->gbuf_streak = 0u;
        if (p.fused && !fb.records) {
            c->gbuf = gv;
            c->gbuf.valid = true;
            c->gbuf_epoch++;
        }
    }
    c->gbuf_streak_lights = c->scene_gen;
    c->last_px = (uint64_t)t.gwidth * t.gheight;   // restir_background_pixels
    c->tmiss_w = tmiss ? t.gwidth : 0u;
    c->tmiss_h = tmiss ? t.gheight : 0u;
    if (p.temporal && !p.temporal_fused) {
        ST_TRY(use_prev(prev, c->device, st, c->pool.get()));   // the predecessor's records are complete (its producer's stream)
        TIMED(c, RESTIR_K_TEMPORAL,
              launch_temporal(s, view, f, restir_rng_key(c->seed, frame, RESTIR_STAGE_TEMPORAL, 0), camd.origin, fb.nt(cur),
                              fb.pm(), fb.ra(cur), fb.rb(cur), fb.pa(prev), fb.pb(prev), fb.ra(cur), fb.rb(cur), nullptr,
                              fb.rp(cur), fb.rp(cur), st));
        used_prev(prev, st, c->pool.get());
    }
    return RESTIR_OK;
}

// What an eligible frame needs of restir_ctx::ahead -- the stream (at the priority frames.ahead_prio asks), the events,
// plane set 1 -- and the frame's own key
restir_status Frame::ahead_prepare(const FramePlan& p, const Route& ris) {
    auto& a = c->ahead;
    if (a.stream && a.stream_prio != a.prio) {   // the knob changed: another stream (ahead_drop waited for the old one)
        ahead_drop(c);
        HIP_TRY(hipStreamDestroy(a.stream));
        a.stream = nullptr;
        a.ready_ok = false;
    }
    if (!a.stream) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&a.stream, hipStreamNonBlocking, a.prio ? least : 0));
        a.stream_prio = a.prio;
    }
    // (the events a launch records within its dispatch, as the timing pairs are: timing_event_create)
    for (int i = 0; i < kRisSets; i++)
        for (hipEvent_t* e : {&a.done[i], &a.consumed[i]})
            if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableSystemFence));
    if (!a.ready) HIP_TRY(hipEventCreateWithFlags(&a.ready, hipEventDisableSystemFence));
    ST_TRY(ahead_planes(2));
    RisAheadKey k;
    k.seed = c->seed; k.frame = frame;
    k.gbuf_epoch = c->gbuf_epoch; k.scene_gen = c->scene_gen; k.geom_gen = c->geom_gen; k.phat_build = c->phat_builds;
    static_assert(sizeof(k.cam) == sizeof(c->gbuf.cam) && sizeof(k.tile) == sizeof(restir_tile) &&
                  sizeof(k.features) == sizeof(FeaturesDev), "RisAheadKey holds the view's and the features' words");
    std::memcpy(k.cam, c->gbuf.cam, sizeof(k.cam));
    k.width = width; k.height = height;
    std::memcpy(k.tile, &t, sizeof(k.tile));
    k.tex_on = s.tex_on;
    std::memcpy(k.features, &f, sizeof(k.features));
    k.passes = passes;
    k.route_grid = ris.grid; k.route_lds = (uint32_t)ris.lds;
    k.route_bits = (ris.how ? 1u : 0u) | (ris.hom ? 2u : 0u) | (ris.res_dead ? 4u : 0u) | (ris.flags ? 8u : 0u) | (ris.skip & 3u) << 4 |
                   (ris.rp_out ? 64u : 0u) | (ris.staged ? 128u : 0u) | (ris.mode & 3u) << 8 | (ris.map2d & 3u) << 10 |
                   ((uint32_t)ris.lt & 7u) << 12 | (ris.n & 3u) << 15 | (p.skip_mode & 3u) << 17;
    k.tuning_gen = a.tuning_gen;
    ahead_key = k;
    ahead_ok = true;
    return RESTIR_OK;
}

// Plane sets 1 .. sets - 1 at the view's size (set 0 is the frame's own)
restir_status Frame::ahead_planes(int sets) {
    auto& a = c->ahead;
    const size_t px = (size_t)t.gwidth * t.gheight;
    for (int i = 0; i < kRisSets - 1; i++) {
        if (i >= sets - 1 && !a.hnd[i].p) continue;   // (a set beyond `sets` that exists follows the view's size too)
        if (a.hnd[i].bytes >= c->hnd[0].bytes && a.rp[i].bytes >= px * 4) continue;
        if (a.hnd[i].p || a.rp[i].p) ahead_drop(c);   // (a result in the smaller planes)
        ST_TRY(a.hnd[i].ensure(c->hnd[0].bytes));
        ST_TRY(a.rp[i].ensure(px * 4));
    }
    return RESTIR_OK;
}

// The next frame's RIS on the look-ahead stream, into the plane set this frame does not read: this frame's own launch
// again under the key (seed, frame + 1, RIS, 0) -- from the batch streak on the next two frames' behind the results that
// already wait, in one launch over the table into two sets neither read nor pending (DESIGN.md §6 "RIS batch").  It reads
// the kept G-buffer, the tile flags and the table, which no frame kernel writes while they stand, and writes planes
// whose last reader's event it waits for.
restir_status Frame::look_ahead() {
    auto& a = c->ahead;
    // how many frames this launch serves (ris_batch_launch): none while enough results wait, one below the batch streak,
    // two from it on -- the frames after the last one a result waits for
    const bool batching = ahead_streak >= std::max(a.batch_after, a.after);
    const int sets = ris_batch_sets(a.batch, a.batch_form);
    if (a.batch == 2u && batching) ST_TRY(ahead_planes(sets));   // (the planes of sets 2 ..: from the first batch on)
    const int pending = ris_ring_pending(a.ring);
    const int n = ris_batch_launch(a.batch, a.batch_form, batching, pending);
    if (!n) return RESTIR_OK;
    int wset[2] = {0, 0}, slots[2] = {0, 0};
    if (!ris_ring_pick(ris_ring_busy(a.ring, fb.set0), n, sets, wset)) return fail(RESTIR_ERR_STATE, "RIS look-ahead: no free plane set");
    if (!a.ready_ok || a.ready_epoch != c->gbuf_epoch || a.ready_build != c->phat_builds) {
        // the G-buffer and the table were written on the frame's stream: once per build
        HIP_TRY(hipEventRecord(a.ready, st));
        HIP_TRY(hipStreamWaitEvent(a.stream, a.ready, 0));
        a.ready_ok = true;
        a.ready_epoch = c->gbuf_epoch;
        a.ready_build = c->phat_builds;
    }
    // (frames.ahead_serial with frames.ahead = 1: behind this frame's last launch, which recorded its set's `consumed`)
    if (a.serial && a.on == 1u && a.consumed_ev[fb.set0]) HIP_TRY(hipStreamWaitEvent(a.stream, a.consumed_ev[fb.set0], 0));
    RisAheadKey keys[2];
    RisBatchOut out[2];
    for (int i = 0; i < n; i++) {
        if (a.consumed_ev[wset[i]]) HIP_TRY(hipStreamWaitEvent(a.stream, a.consumed_ev[wset[i]], 0));
        a.consumed_ev[wset[i]] = nullptr;
        keys[i] = ris_ahead_nth(ahead_key, (uint32_t)(pending + 1 + i));
        FrameBufs o = fb;
        o.set0 = wset[i];
        out[i].key = restir_rng_key(c->seed, keys[i].frame, RESTIR_STAGE_RIS, 0);
        out[i].h = o.h(0);
        out[i].rp = o.rp(0);
    }
    // the launch's done event is its last set's: that set stays busy until both results were taken or dropped
    const hipEvent_t done = a.done[wset[n - 1]];
    a.stop_hint = done;
    a.stop_hint_stream = a.stream;
    if (n == 1) {
        LaunchBufs b = ahead_b;
        b.key = out[0].key;
        b.hout = out[0].h;
        b.rp_out = out[0].rp;
        TIMED(c, RESTIR_K_PRIMARY_RIS, launch_primary_ris(ahead_route, s, view, f, b, a.stream));
    } else {
        TIMED(c, RESTIR_K_PRIMARY_RIS, launch_gbuf_ris_phat_batch(ahead_route, s, view, f, ahead_b, out, a.stream));
    }
    if (!ris_ring_push(a.ring, n, keys, wset, slots)) return fail(RESTIR_ERR_STATE, "RIS look-ahead: the result ring is full");
    for (int i = 0; i < n; i++) a.slot_done[slots[i]] = done;
    return RESTIR_OK;
}

// For each pass: route, launch, from grid cur into its partner; then final shading unless the last pass ran it
restir_status Frame::spatial_passes(const FramePlan& p) {
    LaunchBufs b;
    for (uint32_t pass = 0; pass < passes; pass++) {
        const Region pr = pass_rect(pass);
        const int nxt = cur ^ 1;
        Ask ask = pass_ask(p, pass, last.rp_out);
        // the fused last pass's rays over the view's shadow lists, from the second still frame on (final.lists)
        ask.shadow_lists = ask.fin && c->gbuf_streak >= c->tuning.final_lists_after;
        // ... their answers from the view's visibility bits, from the final.vis_after-th on (final.vis)
        ask.shadow_vis = ask.shadow_lists && c->gbuf_streak >= c->tuning.final_vis_after;
        last = route_spatial(s, pr, f, c->tuning, ask);
        b = fb.bufs(camd, restir_rng_key(c->seed, frame, RESTIR_STAGE_SPATIAL, pass), cur, nxt);
        b.vis = vis;
        b.flags = tmiss;
        if (last.lists) {
            ST_TRY(ensure_shadow_lists(c, last, s, pr, fb.pm(), tmiss, st));
            b.shadow_lists = c->slists.as<uint4>();
            c->shadow_list_frames++;
            if (last.bits) {
                ST_TRY(ensure_shadow_vis(c, st));
                b.shadow_vis = c->svis.as<uint32_t>();
                c->shadow_vis_frames++;
            }
        }
        if (pass + 1 == passes) b.hout = fb.fh(nxt);   // (frame_handles; the route names them)
        // the frame's last launch records the event the look-ahead's next write of grid 0's plane set waits for
        if (ahead_ok && pass + 1 == passes && last.final_done) ahead_consumed_hint();
        TIMED(c, RESTIR_K_SPATIAL, launch_spatial(last, s, pr, f, b, st));
        cur = nxt;
    }
    if (!last.final_done) {
        Ask fin_ask;
        fin_ask.vis = last.vis;
        fin_ask.flags = tmiss != nullptr;
        b = fb.bufs(camd, 0u, cur, cur);
        b.vis = vis;
        b.flags = tmiss;
        if (ahead_ok) ahead_consumed_hint();
        TIMED(c, RESTIR_K_FINAL, launch_final(route_final(s, owned, f, c->tuning, fin_ask), s, owned, f, b, st));
    }
    c->cur = cur;
    return RESTIR_OK;
}

// The frame's grid (cur) to the caller as a frame handle, its image to the caller's memory
restir_status Frame::hand_off(const FramePlan& p, restir_frame** out_next, float* out_rgb) {
    if (out_next) {
        restir_frame* fr = make_frame(c->pool, c->device, st);   // after the final kernel, the records' last reader
        fr->W = width; fr->H = height; fr->vx0 = t.gx0; fr->vy0 = t.gy0; fr->vw = t.gwidth; fr->vh = t.gheight; fr->N = N;
        // hand the final grid's records to the frame (no copy); the context re-allocates lazily
        std::swap(fr->rec, c->rec[cur]);
        fr->records = fb.records;
        fr->hgen = p.frame_handles ? c->scene_gen : 0u;
        fr->hzero = s.num_lights;
        *out_next = fr;
    }
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, fb.rgb().p, (size_t)t.width * t.height * 12, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return RESTIR_OK;
}

}  // namespace

extern "C" {

// renderReSTIR (render.cpp:28-62)
restir_status restir_render(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t width,
                            uint32_t height, const restir_tile* tile, const restir_frame* prev, restir_frame** out_next,
                            float* out_rgb) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    ST_TRY(check_features(features));
    if (out_next) *out_next = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_render before restir_set_scene");
    HIP_TRY(hipSetDevice(c->device));
    if (features->ray_trace_mode != RESTIR_MODE_RESTIR) {   // renderRayTraced's switch (render.cpp:274-279)
        if (tile && (tile->global_width != width || tile->global_height != height || tile->x0 || tile->y0 ||
                     tile->width != width || tile->height != height))
            return fail(RESTIR_ERR_UNSUPPORTED, "R-MIS / R-OMIS render whole images only here (no screen tiles): "
                                                "restir_render_mis_tile renders their tiles");
        return render_mis(c, cam, features, width, height, out_rgb);
    }

    Frame fr{};
    fr.c = c; fr.features = features; fr.width = width; fr.height = height; fr.prev = prev; fr.want_next = out_next != nullptr;
    fr.f = to_dev(features);
    fr.N = fr.f.N;
    fr.passes = features->spatial_reuse ? features->spatial_resampling_passes : 0u;
    fr.st = c->stream;
    restir_tile& t = fr.t;
    ST_TRY(frame_tile(tile, width, height, (uint64_t)fr.passes * fr.f.R, t));
    if (features->temporal_reuse && prev != nullptr)
        ST_TRY(check_prev(c, prev, fr.N, t, width, height, "frame's region", fr.passes > 0));

    // (another view size may reallocate planes a look-ahead launch reads or writes)
    if (t.gwidth != c->vw || t.gheight != c->vh || fr.N != c->N) ahead_drop(c);
    ST_TRY(ensure_records(c, t.gwidth, t.gheight, fr.N, fr.fb));
    c->stage_ok = false;   // ensure_records re-sized the shared view state: the stage API must be reconfigured
    ST_TRY(fr.fb.rgb().ensure((size_t)t.width * t.height * 12));
    c->image_pending(t.width, t.height);

    fr.camd = camera_dev(cam);
    fr.view = fr.fb.region(make_region(width, height, t.gx0, t.gy0, t.gwidth, t.gheight, t.gx0, t.gy0, t.gwidth, t.gheight));
    fr.owned = fr.fb.region(make_region(width, height, t.gx0, t.gy0, t.gwidth, t.gheight, t.x0, t.y0, t.width, t.height));
    fr.frame = c->frame_index++;
    ST_TRY(scene_for(c, fr.f, (size_t)t.gwidth * t.gheight, fr.s, &fr.fb.uv()));

    // the decisions, the allocations they imply, then the launches in stream order
    const FramePlan p = plan_frame(fr);
    ST_TRY(fr.alloc(p));
    ST_TRY(fr.ris_stage(p));
    // the next frame's RIS beside this frame's last pass (frames.ahead; 2: enqueued before the pass, 1: after it)
    if (fr.ahead_ok && c->ahead.on == 2u) ST_TRY(fr.look_ahead());
    ST_TRY(fr.spatial_passes(p));
    if (fr.ahead_ok && c->ahead.on != 2u) ST_TRY(fr.look_ahead());
    c->image_produced();   // the last pass wrote the image
    return fr.hand_off(p, out_next, out_rgb);
}

// One tile (validated) by the whole-image path when it is the whole image, else by the tile path; either consumes one
// frame index.  The caller holds c->mu.
static restir_status render_mis_any(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t width,
                                    uint32_t height, const restir_tile& t, float* out_rgb) {
    if (tile_is_whole_image(t)) return render_mis(c, cam, features, width, height, out_rgb);
    return render_mis_tile(c, cam, features, width, height, t, out_rgb);
}

restir_status restir_render_mis_tile(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t width,
                                     uint32_t height, const restir_tile* tile, float* out_rgb) {
    // the argument checks come first: they need no device (nor a context)
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    ST_TRY(check_features(features));
    restir_tile t;
    ST_TRY(mis_tile_check(features, width, height, tile, t));
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_render_mis_tile before restir_set_scene");
    HIP_TRY(hipSetDevice(c->device));
    return render_mis_any(c, cam, features, width, height, t, out_rgb);
}

restir_status restir_render_mis_tiles(restir_ctx* c, const restir_camera* cam, const restir_features* features,
                                      const restir_tile_layout* layout, float* out_rgb) {
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    if (!out_rgb) return fail(RESTIR_ERR_INVALID, "restir_render_mis_tiles: out_rgb is NULL");
    ST_TRY(check_features(features));
    restir_tile t;
    ST_TRY(restir_layout_tile(layout, 0, features->spatial_resample_radius, &t));   // (checks the layout)
    const uint32_t W = layout->global_width, H = layout->global_height, n = layout->tiles_x * layout->tiles_y;
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_render_mis_tiles before restir_set_scene");
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t frame = c->frame_index;   // every tile renders this frame
    std::vector<float> part;
    for (uint32_t q = 0; q < n; q++) {
        restir_tile tq, tv;
        ST_TRY(restir_layout_tile(layout, q, features->spatial_resample_radius, &tq));
        ST_TRY(mis_tile_check(features, W, H, &tq, tv));
        part.resize((size_t)tv.width * tv.height * 3);
        c->frame_index = frame;
        ST_TRY(render_mis_any(c, cam, features, W, H, tv, part.data()));
        const uint32_t r0 = H - (tv.y0 + tv.height);   // tile rows count from the bottom, image rows from the top
        for (uint32_t r = 0; r < tv.height; r++)
            std::memcpy(out_rgb + ((size_t)(r0 + r) * W + tv.x0) * 3, part.data() + (size_t)r * tv.width * 3,
                        (size_t)tv.width * 12);
    }
    c->frame_index = frame + 1u;
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// motion-compensated temporal reuse (reproject.h; DESIGN.md §6 "Reprojection")
static bool camera_frame_finite(const restir_camera_frame& cf) {
    bool ok = std::isfinite(cf.half_w) && std::isfinite(cf.half_h);
    for (float v : cf.origin) ok = ok && std::isfinite(v);
    for (float v : cf.quat) ok = ok && std::isfinite(v);
    return ok;
}

static ReprojCam reproj_cam(const restir_camera_frame& cf, uint32_t W, uint32_t H) {
    ReprojCam r{};
    r.qx = cf.quat[0]; r.qy = cf.quat[1]; r.qz = cf.quat[2]; r.qw = cf.quat[3];
    r.ox = cf.origin[0]; r.oy = cf.origin[1]; r.oz = cf.origin[2];
    r.half_w = cf.half_w; r.half_h = cf.half_h;
    r.W = W; r.H = H;
    return r;
}

restir_status restir_reproject_pixel(const restir_camera_frame* prev_cam, uint32_t W, uint32_t H, const float P[3],
                                     uint32_t* x, uint32_t* y, float* depth) {
    if (!prev_cam || !P || !x || !y) return fail(RESTIR_ERR_INVALID, "restir_reproject_pixel: NULL argument");
    if (W == 0 || H == 0) return fail(RESTIR_ERR_INVALID, "restir_reproject_pixel: empty image %ux%u", W, H);
    uint32_t sx, sy;
    float d;
    const uint32_t why = reproject_source(reproj_cam(*prev_cam, W, H), P[0], P[1], P[2], sx, sy, d);
    *x = why == kReprojOk ? sx : 0xFFFFFFFFu - why;
    *y = why == kReprojOk ? sy : 0xFFFFFFFFu - why;
    if (depth) *depth = d;
    return RESTIR_OK;
}

restir_status restir_frame_reproject(restir_ctx* c, const restir_frame* prev, const restir_camera* cam_prev,
                                     const restir_camera* cam_cur, restir_frame** out, uint32_t* out_map) {
    // the argument checks come first: they need no device
    if (out) *out = nullptr;
    if (!out) return fail(RESTIR_ERR_INVALID, "restir_frame_reproject: out is NULL");
    if (!cam_prev || !cam_cur) return fail(RESTIR_ERR_INVALID, "restir_frame_reproject: camera is NULL");
    restir_camera_frame cf[2];
    restir_camera_derive(cam_cur, &cf[0]);
    restir_camera_derive(cam_prev, &cf[1]);
    if (!camera_frame_finite(cf[0]) || !camera_frame_finite(cf[1]))
        return fail(RESTIR_ERR_INVALID, "restir_frame_reproject: a camera's derived frame is not finite");
    if (!prev) return fail(RESTIR_ERR_INVALID, "restir_frame_reproject: the predecessor frame is NULL");
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (prev->device != c->device)
        return fail(RESTIR_ERR_INVALID, "temporal predecessor lives on device %d, this context on %d", prev->device, c->device);
    if (prev->vx0 || prev->vy0 || prev->vw != prev->W || prev->vh != prev->H)
        return fail(RESTIR_ERR_UNSUPPORTED, "restir_frame_reproject: the predecessor is a screen tile (its view is not the whole image)");
    if (prev->records)
        return fail(RESTIR_ERR_UNSUPPORTED, "restir_frame_reproject: the predecessor is in the per-pixel records layout");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_frame_reproject before restir_set_scene");
    HIP_TRY(hipSetDevice(c->device));

    const hipStream_t st = c->stream;
    const uint32_t W = prev->W, H = prev->H, N = prev->N;
    const size_t npx = (size_t)W * H;
    for (int i = 0; i < 2; i++) {
        ST_TRY(c->rpj_nt[i].ensure(npx * 16));
        ST_TRY(c->rpj_pm[i].ensure(npx * 16));
    }
    if (out_map) ST_TRY(c->rpj_map.ensure(npx * 4));
    // both G-buffers by the primary-ray launcher over the geometry as it stands now (the texCoord plane is not needed)
    SceneDev s = c->sdev;
    s.gbuf_uv = nullptr;
    s.tex_on = 0u;
    const Region view = make_region(W, H, 0, 0, W, H, 0, 0, W, H);
    const CameraDev camd[2] = {camera_dev(cam_cur), camera_dev(cam_prev)};
    for (int i = 0; i < 2; i++) {
        LaunchBufs b;
        b.cam = &camd[i]; b.origin = camd[i].origin;
        b.n_t = c->rpj_nt[i].as<float4>(); b.p_mat = c->rpj_pm[i].as<float4>();
        TIMED(c, RESTIR_K_PRIMARY, launch_primary(route_primary(s, view, c->tuning), s, view, b, st));
    }
    ST_TRY(use_prev(prev, c->device, st, c->pool.get()));   // the predecessor's records are complete (its producer's stream)
    // the new grid's records, sized as ensure_records sizes a planes frame's (reservoir planes, then the handles' tail)
    const size_t rec_bytes = npx * 2u * N * 16 + (N == 1 ? npx * 8 + 16 : N == 2 ? npx * 16 + 16 : 0);
    DevBuf rec;
    if (!c->pool->take(rec_bytes, st, rec)) ST_TRY(rec.ensure(rec_bytes));
    const bool handles = prev->hgen != 0 && (N == 1 || N == 2);
    ReprojDev r{};
    r.prev_cam = reproj_cam(cf[1], W, H);
    r.N = N;
    r.miss_mat = s.num_materials - 1u;
    r.cur_nt = c->rpj_nt[0].as<float4>(); r.cur_pm = c->rpj_pm[0].as<float4>();
    r.prev_nt = c->rpj_nt[1].as<float4>(); r.prev_pm = c->rpj_pm[1].as<float4>();
    r.ia = prev->rec.as<float4>(); r.ib = r.ia + npx * N;
    r.oa = rec.as<float4>(); r.ob = r.oa + npx * N;
    r.hin = handles ? reinterpret_cast<const float*>(r.ia + 2 * N * npx) : nullptr;
    r.hout = handles ? reinterpret_cast<float*>(r.oa + 2 * N * npx) : nullptr;
    r.zero_handle = prev->hzero << 24;
    r.map = out_map ? c->rpj_map.as<uint32_t>() : nullptr;
    const hipError_t e = launch_reproject(r, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        rec.release();
        return fail(RESTIR_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    }
    used_prev(prev, st, c->pool.get());
    restir_frame* fr = make_frame(c->pool, c->device, st);
    fr->W = W; fr->H = H; fr->vx0 = 0; fr->vy0 = 0; fr->vw = W; fr->vh = H; fr->N = N;
    fr->rec = rec;
    fr->records = false;
    fr->hgen = handles ? prev->hgen : 0u;
    fr->hzero = prev->hzero;
    *out = fr;
    if (out_map) {
        HIP_TRY(hipMemcpyAsync(out_map, c->rpj_map.p, npx * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return RESTIR_OK;
}

restir_status restir_frame_retain(restir_frame* fr) {
    if (!fr) return fail(RESTIR_ERR_INVALID, "frame is NULL");
    fr->refs.fetch_add(1);
    return RESTIR_OK;
}

void restir_frame_release(restir_frame* fr) {
    if (!fr) return;
    if (fr->refs.fetch_sub(1) == 1) {
        // stream-ordered: the records go back to the producing context's pool with the events of the work that
        // touched them (the next user waits on those on its own stream); no device-wide synchronisation
        (void)hipSetDevice(fr->device);
        std::vector<hipEvent_t> busy = std::move(fr->reads);
        if (fr->pool) {
            fr->pool->give(fr->rec, std::move(busy), fr->ready);   // ready: on the pool owner's stream
        } else {
            if (fr->ready) busy.push_back(fr->ready);
            FramePool::Entry e{fr->rec, std::move(busy)};
            FramePool::drain(e);
        }
        fr->rec = DevBuf{};
        delete fr;
    }
}

restir_status restir_frame_info(const restir_frame* fr, uint32_t* width, uint32_t* height, uint32_t* vx0, uint32_t* vy0,
                                uint32_t* vw, uint32_t* vh, uint32_t* n) {
    if (!fr) return fail(RESTIR_ERR_INVALID, "frame is NULL");
    if (width) *width = fr->W;
    if (height) *height = fr->H;
    if (vx0) *vx0 = fr->vx0;
    if (vy0) *vy0 = fr->vy0;
    if (vw) *vw = fr->vw;
    if (vh) *vh = fr->vh;
    if (n) *n = fr->N;
    return RESTIR_OK;
}

restir_status restir_frame_download(const restir_frame* fr, float* pos, float* color, float* w, uint32_t* m) {
    if (!fr) return fail(RESTIR_ERR_INVALID, "frame is NULL");
    HIP_TRY(hipSetDevice(fr->device));
    if (fr->ready) HIP_TRY(hipEventSynchronize(fr->ready));
    const size_t npx = (size_t)fr->vw * fr->vh, N = fr->N;
    // the records as stored: per pixel [n_t, a_0, b_0, a_1, b_1, ...] or planes [a_0 .. a_N-1 | b_0 .. b_N-1]
    const size_t f4 = fr->records ? npx * (1 + 2 * N) : npx * 2 * N;
    std::vector<float> host(4 * f4);
    HIP_TRY(hipMemcpy(host.data(), fr->rec.p, host.size() * 4, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < N; j++)
        for (size_t p = 0; p < npx; p++) {
            const float* a = fr->records ? &host[4 * (p * (1 + 2 * N) + 1 + 2 * j)] : &host[4 * (j * npx + p)];
            const float* b = fr->records ? &host[4 * (p * (1 + 2 * N) + 2 + 2 * j)] : &host[4 * ((N + j) * npx + p)];
            const size_t i = j * npx + p;
            if (pos) { pos[3 * i] = a[0]; pos[3 * i + 1] = a[1]; pos[3 * i + 2] = a[2]; }
            if (w) w[i] = a[3];
            if (color) { color[3 * i] = b[0]; color[3 * i + 1] = b[1]; color[3 * i + 2] = b[2]; }
            if (m) std::memcpy(&m[i], &b[3], 4);
        }
    return RESTIR_OK;
}

restir_status restir_synchronize(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(sync_streams(c));
    return RESTIR_OK;
}

restir_status restir_download_rgb(restir_ctx* c, float* out_rgb, size_t count) {
    if (!c || !out_rgb) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t need = (size_t)c->rgb_w * c->rgb_h * 3;
    if (need == 0) return fail(RESTIR_ERR_STATE, "nothing rendered yet");
    if (count < need) return fail(RESTIR_ERR_INVALID, "buffer holds %zu floats, need %zu", count, need);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, need * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// presenting a frame (include/restir_c.h "presenting a frame")
static void release_images(restir_ctx* c) {
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);   // outstanding copies land before their buffers go
    for (restir_image& im : c->images) {
        im.stage.release();
        if (im.host) (void)hipHostFree(im.host);
        if (im.converted) (void)hipEventDestroy(im.converted);
        if (im.landed) (void)hipEventDestroy(im.landed);
        im = restir_image();
    }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    c->copy_stream = nullptr;
}

// the conversion (or copy) into the slot's staging buffer on the context's stream, the copy to its pinned buffer on the
// copy stream behind it
static restir_status image_enqueue(restir_ctx* c, restir_image* im, uint32_t format, size_t px, size_t bytes) {
    if (format == RESTIR_IMAGE_RGB32F) {
        HIP_TRY(hipMemcpyAsync(im->stage.p, c->rgb.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {
        PresentDev p{};
        p.rgb = c->rgb.as<float>();
        p.out = im->stage.as<uint32_t>();
        p.bgr_flip = format == RESTIR_IMAGE_BGRA8_BOTTOM_UP;
        p.row_px = p.bgr_flip ? c->rgb_w : px;
        p.rows = p.bgr_flip ? c->rgb_h : 1u;
        HIP_TRY(launch_present(p, c->stream));
    }
    HIP_TRY(hipEventRecord(im->converted, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, im->converted, 0));   // the one cross-stream dependency
    HIP_TRY(hipMemcpyAsync(im->host, im->stage.p, bytes, hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(hipEventRecord(im->landed, c->copy_stream));
    return RESTIR_OK;
}

// the caller holds c->mu and has set the device
static restir_status image_begin_locked(restir_ctx* c, uint32_t format, restir_image** out) {
    if (format > (uint32_t)RESTIR_IMAGE_BGRA8_BOTTOM_UP) return fail(RESTIR_ERR_INVALID, "unknown image format %u", format);
    const size_t px = (size_t)c->rgb_w * c->rgb_h;
    if (px == 0) return fail(RESTIR_ERR_STATE, "nothing rendered yet");
    restir_image* im = nullptr;
    for (restir_image& s : c->images)
        if (!s.in_use) { im = &s; break; }
    if (!im)
        return fail(RESTIR_ERR_STATE, "%u snapshots are unreleased (RESTIR_MAX_IMAGES_IN_FLIGHT): restir_image_release one first",
                    RESTIR_MAX_IMAGES_IN_FLIGHT);
    const size_t bytes = px * (format == RESTIR_IMAGE_RGB32F ? 12u : 4u);
    if (!c->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!im->converted) HIP_TRY(hipEventCreateWithFlags(&im->converted, hipEventDisableTiming));
    if (!im->landed) HIP_TRY(hipEventCreateWithFlags(&im->landed, hipEventDisableTiming));
    // a free slot's last copy has landed (restir_image_release waited for it): its buffers may be replaced
    ST_TRY(im->stage.ensure(bytes));
    if (im->host_bytes < bytes) {
        if (im->host) (void)hipHostFree(im->host);
        im->host = nullptr;
        im->host_bytes = 0;
        hipError_t e = hipHostMalloc(&im->host, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { im->host = nullptr; return fail(RESTIR_ERR_HIP, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
        im->host_bytes = bytes;
    }
    const restir_status st = image_enqueue(c, im, format, px, bytes);
    if (st != RESTIR_OK) {
        // part of the work may be enqueued: the slot stays free, so nothing may still write its buffers when it is taken
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->copy_stream);
        return st;
    }
    im->ctx = c;
    im->in_use = true;
    im->width = c->rgb_w;
    im->height = c->rgb_h;
    im->format = format;
    im->bytes = bytes;
    *out = im;
    return RESTIR_OK;
}

static void image_release_locked(restir_image* im) {
    if (!im->in_use) return;
    (void)hipEventSynchronize(im->landed);   // the slot's buffers are re-used only after its copy
    im->in_use = false;
}

restir_status restir_image_begin(restir_ctx* c, uint32_t format, restir_image** out) {
    if (!c || !out) return fail(RESTIR_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return image_begin_locked(c, format, out);
}

restir_status restir_image_info(const restir_image* im, uint32_t* width, uint32_t* height, uint32_t* format, size_t* bytes) {
    if (!im || !im->ctx) return fail(RESTIR_ERR_INVALID, "image is NULL");
    std::lock_guard<std::mutex> lk(im->ctx->mu);
    if (!im->in_use) return fail(RESTIR_ERR_INVALID, "the image has been released");
    if (width) *width = im->width;
    if (height) *height = im->height;
    if (format) *format = im->format;
    if (bytes) *bytes = im->bytes;
    return RESTIR_OK;
}

restir_status restir_image_ready(restir_image* im, int* ready) {
    if (!im || !ready || !im->ctx) return fail(RESTIR_ERR_INVALID, "null argument");
    *ready = 0;
    std::lock_guard<std::mutex> lk(im->ctx->mu);
    if (!im->in_use) return fail(RESTIR_ERR_INVALID, "the image has been released");
    HIP_TRY(hipSetDevice(im->ctx->device));
    const hipError_t e = hipEventQuery(im->landed);
    if (e == hipSuccess) { *ready = 1; return RESTIR_OK; }
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return RESTIR_OK; }
    return fail(RESTIR_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e));
}

restir_status restir_image_wait(restir_image* im, const void** data) {
    if (!im || !data || !im->ctx) return fail(RESTIR_ERR_INVALID, "null argument");
    *data = nullptr;
    hipEvent_t landed;
    const void* host;
    {
        std::lock_guard<std::mutex> lk(im->ctx->mu);
        if (!im->in_use) return fail(RESTIR_ERR_INVALID, "the image has been released");
        HIP_TRY(hipSetDevice(im->ctx->device));
        landed = im->landed;
        host = im->host;
    }
    // outside the mutex: another thread may enqueue the next frame while this one waits for its copy, and only for it
    HIP_TRY(hipEventSynchronize(landed));
    *data = host;
    return RESTIR_OK;
}

void restir_image_release(restir_image* im) {
    if (!im || !im->ctx) return;
    std::lock_guard<std::mutex> lk(im->ctx->mu);
    (void)hipSetDevice(im->ctx->device);
    image_release_locked(im);
}

restir_status restir_download_rgba8(restir_ctx* c, uint8_t* out_rgba, size_t pixels) {
    if (!c || !out_rgba) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t need = (size_t)c->rgb_w * c->rgb_h;
    if (need == 0) return fail(RESTIR_ERR_STATE, "nothing rendered yet");
    if (pixels < need) return fail(RESTIR_ERR_INVALID, "buffer holds %zu pixels, need %zu", pixels, need);
    HIP_TRY(hipSetDevice(c->device));
    restir_image* im = nullptr;
    ST_TRY(image_begin_locked(c, RESTIR_IMAGE_RGBA8, &im));
    const hipError_t e = hipEventSynchronize(im->landed);
    if (e == hipSuccess) std::memcpy(out_rgba, im->host, im->bytes);
    image_release_locked(im);
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(e));
    return RESTIR_OK;
}

restir_status restir_write_image_bmp(restir_ctx* c, const char* path) {
    if (!c || !path) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((size_t)c->rgb_w * c->rgb_h == 0) return fail(RESTIR_ERR_STATE, "nothing rendered yet");
    HIP_TRY(hipSetDevice(c->device));
    restir_image* im = nullptr;
    ST_TRY(image_begin_locked(c, RESTIR_IMAGE_BGRA8_BOTTOM_UP, &im));
    const hipError_t e = hipEventSynchronize(im->landed);
    // stbi_write_bmp's header (screen.cpp bmp_header, shared with restir_encode_bmp) around the snapshot's bytes
    const bool ok = e == hipSuccess && write_bmp_words(path, im->width, im->height, static_cast<const uint32_t*>(im->host));
    image_release_locked(im);
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(e));
    if (!ok) return fail(RESTIR_ERR_INVALID, "cannot write %s", path);
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// accumulating frames (include/restir_c.h "accumulating frames", accum.h).  Nothing here reads or writes
// the still view's caches (gbuf, slists, svis, phat, gbuf_streak): a standing view keeps them while it accumulates.
static void accum_close(restir_ctx* c) {
    c->acc.open = false;
    c->acc.frames = 0;
    c->acc.mean.release();
    c->acc.m2.release();
    c->acc.partials.release();
}

// the caller holds c->mu
static restir_status accum_add_locked(restir_ctx* c) {
    auto& a = c->acc;
    if (!a.open) return fail(RESTIR_ERR_STATE, "restir_accum_add before restir_accum_begin");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_accum_add between restir_halo_begin and restir_halo_end");
    if (c->rgb_from == restir_ctx::RGB_RESOLVED)
        return fail(RESTIR_ERR_STATE, "restir_accum_add: the last image is restir_accum_resolve's or restir_denoise's, not a frame");
    if (c->rgb_from != restir_ctx::RGB_PRODUCED || (size_t)c->rgb_w * c->rgb_h == 0)
        return fail(RESTIR_ERR_STATE, "restir_accum_add: nothing rendered yet");
    if (a.frames > 0 && a.added_serial == c->rgb_serial)
        return fail(RESTIR_ERR_STATE, "restir_accum_add: the last image was added already");
    if (a.frames > 0 && (a.width != c->rgb_w || a.height != c->rgb_h))
        return fail(RESTIR_ERR_STATE, "restir_accum_add: the last image is %ux%u, the accumulation %ux%u", c->rgb_w, c->rgb_h,
                    a.width, a.height);
    if (a.frames >= kAccumMaxFrames) return fail(RESTIR_ERR_STATE, "restir_accum_add: %u frames are folded already", a.frames);
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t count = (uint64_t)c->rgb_w * c->rgb_h * 3u;
    const bool var = (a.flags & RESTIR_ACCUM_VARIANCE) != 0;
    if (a.frames == 0) {   // the empty state: mean = m2 = 0
        restir_status st = a.mean.ensure(count * 4);
        if (st == RESTIR_OK && var) st = a.m2.ensure(count * 4);
        if (st != RESTIR_OK) { accum_close(c); return st; }
        HIP_TRY(hipMemsetAsync(a.mean.p, 0, count * 4, c->stream));
        if (var) HIP_TRY(hipMemsetAsync(a.m2.p, 0, count * 4, c->stream));
        a.width = c->rgb_w;
        a.height = c->rgb_h;
    }
    const float inv_n = 1.0f / (float)(a.frames + 1u);
    HIP_TRY(launch_accum_add(c->rgb.as<float>(), a.mean.as<float>(), var ? a.m2.as<float>() : nullptr, count, inv_n, c->stream));
    a.frames++;
    a.added_serial = c->rgb_serial;
    return RESTIR_OK;
}

static restir_status accum_resolve_locked(restir_ctx* c, const restir_features* tone) {
    auto& a = c->acc;
    if (!a.open || a.frames == 0) return fail(RESTIR_ERR_STATE, "restir_accum_resolve: no frame is accumulated");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_accum_resolve between restir_halo_begin and restir_halo_end");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t px = (uint64_t)a.width * a.height;
    ST_TRY(c->rgb.ensure(px * 12));   // a render of another size may have come between
    c->image_pending(a.width, a.height);
    FeaturesDev d{};
    if (tone) {
        d.tone_map = tone->enable_tone_mapping;
        d.gamma = tone->gamma;
        d.exposure = tone->exposure;
    }
    HIP_TRY(launch_accum_resolve(a.mean.as<float>(), c->rgb.as<float>(), px, d, c->stream));
    c->rgb_from = restir_ctx::RGB_RESOLVED;
    return RESTIR_OK;
}

static void accum_stats_header(const restir_ctx* c, restir_accum_stats* out) {
    *out = restir_accum_stats{};
    out->width = c->acc.width;
    out->height = c->acc.height;
    out->frames = c->acc.frames;
    out->flags = c->acc.flags;
}

static restir_status accum_stats_locked(restir_ctx* c, restir_accum_stats* out) {
    auto& a = c->acc;
    if (!a.open) return fail(RESTIR_ERR_STATE, "restir_accum_stats_get before restir_accum_begin");
    if (!(a.flags & RESTIR_ACCUM_VARIANCE)) return fail(RESTIR_ERR_STATE, "restir_accum_stats_get needs RESTIR_ACCUM_VARIANCE");
    if (a.frames < 2) return fail(RESTIR_ERR_STATE, "restir_accum_stats_get needs two frames, %u are accumulated", a.frames);
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t count = (uint64_t)a.width * a.height * 3u;
    const uint64_t blocks = accum_stats_blocks(count);
    ST_TRY(a.partials.ensure(blocks * sizeof(AccumPartial)));
    const double nn1 = (double)a.frames * (double)(a.frames - 1u);
    HIP_TRY(launch_accum_stats(a.mean.as<float>(), a.m2.as<float>(), count, nn1, a.partials.as<AccumPartial>(), c->stream));
    std::vector<AccumPartial> host(blocks);
    HIP_TRY(hipMemcpyAsync(host.data(), a.partials.p, blocks * sizeof(AccumPartial), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double term = 0.0, value = 0.0;
    uint64_t bad = 0;
    for (const AccumPartial& p : host) {   // in index order
        term += p.term;
        value += p.value;
        bad += p.nonfinite;
    }
    accum_stats_header(c, out);
    out->nonfinite = bad;
    const double counted = (double)(count - bad);   // 0 counted: 0 / 0, which no target meets
    out->est_mse = term / counted;
    out->mean_value = value / counted;
    return RESTIR_OK;
}

restir_status restir_accum_begin(restir_ctx* c, uint32_t flags) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (flags & ~RESTIR_ACCUM_VARIANCE) return fail(RESTIR_ERR_INVALID, "restir_accum_begin: unknown flags 0x%x", flags);
    std::lock_guard<std::mutex> lk(c->mu);
    c->acc.open = true;
    c->acc.flags = flags;
    c->acc.frames = 0;
    c->acc.width = c->acc.height = 0;
    c->acc.added_serial = 0;
    return RESTIR_OK;
}

restir_status restir_accum_add(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    return accum_add_locked(c);
}

restir_status restir_accum_resolve(restir_ctx* c, const restir_features* tone) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    return accum_resolve_locked(c, tone);
}

restir_status restir_accum_stats_get(restir_ctx* c, restir_accum_stats* out) {
    if (!c || !out) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    return accum_stats_locked(c, out);
}

restir_status restir_accum_download(restir_ctx* c, float* mean, float* m2, size_t count) {
    if (!c || !mean) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    auto& a = c->acc;
    if (!a.open || a.frames == 0) return fail(RESTIR_ERR_STATE, "restir_accum_download: no frame is accumulated");
    const size_t need = (size_t)a.width * a.height * 3;
    if (count < need) return fail(RESTIR_ERR_INVALID, "buffer holds %zu floats, need %zu", count, need);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(mean, a.mean.p, need * 4, hipMemcpyDeviceToHost, c->stream));
    if (m2) {
        if (a.flags & RESTIR_ACCUM_VARIANCE)
            HIP_TRY(hipMemcpyAsync(m2, a.m2.p, need * 4, hipMemcpyDeviceToHost, c->stream));
        else
            std::memset(m2, 0, need * 4);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_accum_end(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    accum_close(c);   // (hipFree waits for the kernels that use the planes)
    return RESTIR_OK;
}

restir_status restir_accum_fold(float* mean, float* m2, const float* x, size_t count, uint32_t n) {
    if (!mean || !x) return fail(RESTIR_ERR_INVALID, "null argument");
    if (n == 0 || n > kAccumMaxFrames) return fail(RESTIR_ERR_INVALID, "restir_accum_fold: n = %u outside 1..%u", n, kAccumMaxFrames);
    const float inv_n = 1.0f / (float)n;
    if (m2)
        for (size_t i = 0; i < count; i++) accum_fold_var(x[i], inv_n, mean[i], m2[i]);
    else
        for (size_t i = 0; i < count; i++) accum_fold_mean(x[i], inv_n, mean[i]);
    return RESTIR_OK;
}

// Every step takes the context's mutex for itself (restir_render's own, then the add's): calls on one context are
// serialised by the context, and a caller that shares it between threads orders its calls as for any other sequence.
restir_status restir_render_accumulate(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t width,
                                       uint32_t height, const restir_tile* tile, const restir_accum_request* req,
                                       restir_accum_stats* out_stats, float* out_rgb) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    if (!req) return fail(RESTIR_ERR_INVALID, "request is NULL");
    ST_TRY(check_features(features));
    if (req->flags & ~RESTIR_ACCUM_VARIANCE) return fail(RESTIR_ERR_INVALID, "restir_render_accumulate: unknown flags 0x%x", req->flags);
    if (req->max_frames == 0 || req->max_frames > kAccumMaxFrames)
        return fail(RESTIR_ERR_INVALID, "restir_render_accumulate: max_frames %u outside 1..%u", req->max_frames, kAccumMaxFrames);
    if (req->min_frames > req->max_frames)
        return fail(RESTIR_ERR_INVALID, "restir_render_accumulate: min_frames %u > max_frames %u", req->min_frames, req->max_frames);
    const bool target = req->target_mse > 0.0;
    if (target && !(req->flags & RESTIR_ACCUM_VARIANCE))
        return fail(RESTIR_ERR_INVALID, "restir_render_accumulate: a target needs RESTIR_ACCUM_VARIANCE");
    if (target && req->check_every == 0) return fail(RESTIR_ERR_INVALID, "restir_render_accumulate: a target needs check_every > 0");

    restir_features f = *features;
    f.enable_tone_mapping = 0;   // the mean is tone mapped, not the frames
    const bool chain = f.ray_trace_mode == RESTIR_MODE_RESTIR && f.temporal_reuse;
    ST_TRY(restir_accum_begin(c, req->flags));
    restir_frame* prev = nullptr;
    restir_status st = RESTIR_OK;
    restir_accum_stats stats{};
    for (uint32_t n = 1; n <= req->max_frames; n++) {
        restir_frame* next = nullptr;
        st = restir_render(c, cam, &f, width, height, tile, prev, chain ? &next : nullptr, nullptr);
        if (prev) restir_frame_release(prev);
        prev = next;
        if (st != RESTIR_OK) break;
        st = restir_accum_add(c);
        if (st != RESTIR_OK) break;
        if (target && n >= 2 && n >= req->min_frames && (n - req->min_frames) % req->check_every == 0) {
            st = restir_accum_stats_get(c, &stats);
            if (st != RESTIR_OK || stats.est_mse <= req->target_mse) break;
        }
    }
    if (prev) restir_frame_release(prev);
    ST_TRY(st);
    ST_TRY(restir_accum_resolve(c, features));
    if (out_stats) {
        std::lock_guard<std::mutex> lk(c->mu);
        if ((c->acc.flags & RESTIR_ACCUM_VARIANCE) && c->acc.frames >= 2)
            ST_TRY(accum_stats_locked(c, out_stats));
        else
            accum_stats_header(c, out_stats);
    }
    if (out_rgb) {
        size_t count;
        {
            std::lock_guard<std::mutex> lk(c->mu);
            count = (size_t)c->rgb_w * c->rgb_h * 3;
        }
        ST_TRY(restir_download_rgb(c, out_rgb, count));
    }
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the exact image, the kept reference and the error figures (include/restir_c.h, exact.h, DESIGN.md §6 "Exact image and
// error figures").  Nothing here reads or writes the frame path's G-buffer planes or what is built over them (gbuf,
// tmiss, slists, svis, phat, gbuf_streak), the frame index or the stage buffers.
restir_status restir_render_exact(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t width,
                                  uint32_t height, const restir_tile* tile, float* out_rgb) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    if (!features) return fail(RESTIR_ERR_INVALID, "features is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_render_exact before restir_set_scene");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_render_exact between restir_halo_begin and restir_halo_end");
    if (c->sdev.num_lights > 0 && c->sdev.light_types != (1u << RESTIR_LIGHT_POINT)) {
        const char* what = (c->sdev.light_types & (1u << RESTIR_LIGHT_SEGMENT)) ? "segment" : "parallelogram";
        return fail(RESTIR_ERR_UNSUPPORTED, "restir_render_exact: the scene holds a %s light; the exact image is the finite sum "
                                            "over point lights only", what);
    }
    restir_tile t;
    ST_TRY(frame_tile(tile, width, height, 0, t));
    HIP_TRY(hipSetDevice(c->device));

    // the owned rectangle is the view: the image is pixel-local, a tile's ghost ring is not computed
    const size_t npx = (size_t)t.width * t.height;
    ST_TRY(c->exact_nt.ensure(npx * 16));
    ST_TRY(c->exact_pm.ensure(npx * 16));
    FeaturesDev f{};
    f.shading = features->enable_shading;
    f.texture = features->enable_texture_mapping;
    f.tone_map = features->enable_tone_mapping;
    f.gamma = features->gamma;
    f.exposure = features->exposure;
    SceneDev s;
    ST_TRY(scene_for(c, f, npx, s, &c->exact_uv));
    ST_TRY(c->rgb.ensure(npx * 12));
    c->image_pending(t.width, t.height);
    c->stage_ok = false;   // the image buffer has another size now: the stage API must be reconfigured, as after restir_render

    const CameraDev camd = camera_dev(cam);
    const Region view = make_region(width, height, t.x0, t.y0, t.width, t.height, t.x0, t.y0, t.width, t.height);
    LaunchBufs b;
    b.cam = &camd; b.origin = camd.origin;
    b.n_t = c->exact_nt.as<float4>(); b.p_mat = c->exact_pm.as<float4>();
    set_launch_events(nullptr, nullptr);   // no RESTIR_K_* slot: restir_timings does not see these launches
    HIP_TRY(launch_primary(route_primary(s, view, c->tuning), s, view, b, c->stream));
    HIP_TRY(launch_exact(s, view, f, camd.origin, b.n_t, b.p_mat, c->rgb.as<float>(), c->stream));
    c->image_produced();
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, npx * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

restir_status restir_reference_set(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_reference_set between restir_halo_begin and restir_halo_end");
    const size_t bytes = (size_t)c->rgb_w * c->rgb_h * 12;
    if ((c->rgb_from != restir_ctx::RGB_PRODUCED && c->rgb_from != restir_ctx::RGB_RESOLVED) || bytes == 0)
        return fail(RESTIR_ERR_STATE, "restir_reference_set: nothing rendered yet");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->ref.p || c->ref.bytes < bytes) {   // the old reference stands until the new buffer does
        DevBuf nb;
        ST_TRY(nb.ensure(bytes));
        c->ref.release();
        c->ref = nb;
    }
    c->ref_w = c->rgb_w;
    c->ref_h = c->rgb_h;
    HIP_TRY(hipMemcpyAsync(c->ref.p, c->rgb.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    return RESTIR_OK;
}

restir_status restir_reference_clear(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    c->ref.release();   // (hipFree waits for the kernels that read it)
    c->ref_w = c->ref_h = 0;
    return RESTIR_OK;
}

restir_status restir_reference_info(restir_ctx* c, uint32_t* width, uint32_t* height, int* present) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (width) *width = c->ref_w;
    if (height) *height = c->ref_h;
    if (present) *present = c->ref.p ? 1 : 0;
    return RESTIR_OK;
}

static void error_stats_fill(const ErrorSums& t, restir_error_stats* out) {
    out->counted = t.counted;
    out->nonfinite = t.nonfinite;
    const double n = (double)t.counted;   // 0 counted: 0 / 0
    out->mse = t.se / n;
    out->mae = t.ae / n;
    out->rel_mse = t.rel / n;
    out->bias = t.d / n;
    out->max_abs = t.max_abs;
    out->ref_mean = t.ref / n;
}

restir_status restir_error_get(restir_ctx* c, uint32_t source, restir_error_stats* out) {
    if (!c || !out) return fail(RESTIR_ERR_INVALID, "null argument");
    if (source != RESTIR_ERROR_SRC_IMAGE && source != RESTIR_ERROR_SRC_ACCUM_MEAN)
        return fail(RESTIR_ERR_INVALID, "restir_error_get: unknown source %u", source);
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->ref.p) return fail(RESTIR_ERR_STATE, "restir_error_get before restir_reference_set");
    const float* a;
    uint32_t w, h, frames = 0;
    if (source == RESTIR_ERROR_SRC_IMAGE) {
        if ((c->rgb_from != restir_ctx::RGB_PRODUCED && c->rgb_from != restir_ctx::RGB_RESOLVED) || (size_t)c->rgb_w * c->rgb_h == 0)
            return fail(RESTIR_ERR_STATE, "restir_error_get: nothing rendered yet");
        a = c->rgb.as<float>(); w = c->rgb_w; h = c->rgb_h;
    } else {
        if (!c->acc.open || c->acc.frames == 0) return fail(RESTIR_ERR_STATE, "restir_error_get: no frame is accumulated");
        a = c->acc.mean.as<float>(); w = c->acc.width; h = c->acc.height; frames = c->acc.frames;
    }
    if (w != c->ref_w || h != c->ref_h)
        return fail(RESTIR_ERR_STATE, "restir_error_get: the source is %ux%u, the reference %ux%u", w, h, c->ref_w, c->ref_h);
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t count = (uint64_t)w * h * 3u;
    const uint64_t blocks = error_blocks(count);
    ST_TRY(c->err_partials.ensure(blocks * sizeof(ErrorSums)));
    HIP_TRY(launch_error_stats(a, c->ref.as<float>(), count, c->err_partials.as<ErrorSums>(), c->stream));
    std::vector<ErrorSums> host(blocks);
    HIP_TRY(hipMemcpyAsync(host.data(), c->err_partials.p, blocks * sizeof(ErrorSums), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ErrorSums total;
    error_zero(total);
    for (const ErrorSums& p : host) error_merge(total, p);   // in index order
    *out = restir_error_stats{};
    out->width = w; out->height = h; out->source = source; out->frames = frames;
    error_stats_fill(total, out);
    return RESTIR_OK;
}

restir_status restir_error_measure(const float* a, const float* r, size_t count, restir_error_stats* out) {
    if (!a || !r || !out) return fail(RESTIR_ERR_INVALID, "null argument");
    if (count == 0) return fail(RESTIR_ERR_INVALID, "restir_error_measure: count is 0");
    ErrorSums total;
    error_measure_host(a, r, count, total);
    *out = restir_error_stats{};
    error_stats_fill(total, out);
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// denoising the last image (include/restir_c.h "denoising the last image", denoise.h, DESIGN.md §6 "Denoising a frame").
// Like the exact image, nothing here reads or writes the frame path's G-buffer planes or what is built over them, the
// frame index or the stage buffers.
// The guide planes restir_denoise and restir_denoise_lum share.  denoise_guides_alloc compares the view with the kept
// planes' key and sizes the planes where it differs; denoise_guides_trace then traces them (once per view).  The caller
// holds c->mu and has set the device.
struct DenoiseView {
    CameraDev camd;
    restir_ctx::DenoiseKey want;
    bool keep = false;
};

static restir_status denoise_guides_alloc(restir_ctx* c, const restir_camera* cam, uint32_t width, uint32_t height,
                                          const restir_tile& t, DenoiseView& v) {
    const size_t npx = (size_t)t.width * t.height;
    v.camd = camera_dev(cam);
    const CameraDev& camd = v.camd;
    restir_ctx::DenoiseKey& want = v.want;
    want.valid = true;
    want.geom_gen = c->geom_gen;
    const float camf[9] = {camd.quat.x, camd.quat.y, camd.quat.z, camd.quat.w, camd.origin[0], camd.origin[1], camd.origin[2],
                           camd.half_w, camd.half_h};
    std::memcpy(want.cam, camf, sizeof(want.cam));
    want.width = width; want.height = height;
    want.tile = t;
    const restir_ctx::DenoiseKey& have = c->dn_key;
    v.keep = have.valid && have.geom_gen == want.geom_gen && !std::memcmp(have.cam, want.cam, sizeof(have.cam)) &&
             have.width == want.width && have.height == want.height && !std::memcmp(&have.tile, &want.tile, sizeof(restir_tile));
    if (!v.keep) {
        c->dn_key.valid = false;
        c->dn_var_px = 0;   // the variance planes live with the guides
        ST_TRY(c->dn_nt.ensure(npx * 16));
        ST_TRY(c->dn_pf.ensure(npx * 16));
        ST_TRY(c->dn_ga.ensure(npx * 16));
    }
    return RESTIR_OK;
}

static restir_status denoise_guides_trace(restir_ctx* c, uint32_t width, uint32_t height, const restir_tile& t, DenoiseView& v) {
    if (v.keep) return RESTIR_OK;
    const size_t npx = (size_t)t.width * t.height;
    FeaturesDev f{};
    SceneDev s;
    ST_TRY(scene_for(c, f, npx, s, &c->dn_uv));
    const Region view = make_region(width, height, t.x0, t.y0, t.width, t.height, t.x0, t.y0, t.width, t.height);
    LaunchBufs b;
    b.cam = &v.camd; b.origin = v.camd.origin;
    b.n_t = c->dn_nt.as<float4>(); b.p_mat = c->dn_pf.as<float4>();
    HIP_TRY(launch_primary(route_primary(s, view, c->tuning), s, view, b, c->stream));
    HIP_TRY(launch_denoise_guides(b.n_t, b.p_mat, c->dn_ga.as<float4>(), npx, s.num_materials - 1u, c->stream));
    c->dn_key = v.want;
    c->dn_guide_builds++;
    return RESTIR_OK;
}

restir_status restir_denoise(restir_ctx* c, const restir_camera* cam, uint32_t width, uint32_t height, const restir_tile* tile,
                             const restir_denoise_params* params, const restir_features* tone, float* out_rgb) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    ST_TRY(denoise_params_check(params, "restir_denoise"));
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_denoise before restir_set_scene");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_denoise between restir_halo_begin and restir_halo_end");
    restir_tile t;
    ST_TRY(frame_tile(tile, width, height, 0, t));
    if ((c->rgb_from != restir_ctx::RGB_PRODUCED && c->rgb_from != restir_ctx::RGB_RESOLVED) || (size_t)c->rgb_w * c->rgb_h == 0)
        return fail(RESTIR_ERR_STATE, "restir_denoise: nothing rendered yet");
    if (t.width != c->rgb_w || t.height != c->rgb_h)
        return fail(RESTIR_ERR_STATE, "restir_denoise: the last image is %ux%u, the owned rectangle %ux%u", c->rgb_w, c->rgb_h,
                    t.width, t.height);
    HIP_TRY(hipSetDevice(c->device));

    const size_t npx = (size_t)t.width * t.height;
    DenoiseView view;
    // every buffer first: a refused allocation leaves the image as it was
    const uint32_t levels = params->iterations;
    ST_TRY(denoise_guides_alloc(c, cam, width, height, t, view));
    ST_TRY(c->dn_tmp[0].ensure(npx * 12));
    if (levels > 2u) ST_TRY(c->dn_tmp[1].ensure(npx * 12));
    set_launch_events(nullptr, nullptr);   // no RESTIR_K_* slot: restir_timings does not see these launches
    ST_TRY(denoise_guides_trace(c, width, height, t, view));
    c->stage_ok = false;   // like restir_render_exact: the stage API is to be configured again

    FeaturesDev tf{};
    if (tone) {
        tf.tone_map = tone->enable_tone_mapping;
        tf.gamma = tone->gamma;
        tf.exposure = tone->exposure;
    }
    // level 0 reads the image (a copy of it when it is the last level too), level i the level before, the last writes
    // the image: rgb -> tmp0 -> tmp1 -> tmp0 -> ... -> rgb
    float* rgb = c->rgb.as<float>();
    const float* in = rgb;
    c->rgb_from = restir_ctx::RGB_PENDING;   // (a launch the device refuses leaves the buffer without an image)
    if (levels == 1u) {
        HIP_TRY(hipMemcpyAsync(c->dn_tmp[0].p, rgb, npx * 12, hipMemcpyDeviceToDevice, c->stream));
        in = c->dn_tmp[0].as<float>();
    }
    for (uint32_t level = 0; level < levels; level++) {
        const bool last = level + 1u == levels;
        float* out = last ? rgb : c->dn_tmp[level & 1u].as<float>();
        HIP_TRY(launch_denoise_level(in, out, c->dn_nt.as<float4>(), c->dn_ga.as<float4>(), c->dn_pf.as<float4>(), t.width, t.height,
                                     level, params->normal_power_log2, params->sigma_plane, last ? &tf : nullptr, c->stream));
        in = out;
    }
    c->rgb_from = restir_ctx::RGB_RESOLVED;
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, npx * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

// restir_denoise with the variance-guided luminance term (include/restir_c.h "denoising with a variance-guided
// luminance term").  The colour takes restir_denoise's way through the scratch images; the variance alternates between
// dn_var[0] and dn_var[1], level i reading dn_var[i & 1].
restir_status restir_denoise_lum(restir_ctx* c, const restir_camera* cam, uint32_t width, uint32_t height, const restir_tile* tile,
                                 const restir_denoise_lum_params* params, const restir_features* tone, float* out_rgb) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    ST_TRY(denoise_lum_params_check(params, "restir_denoise_lum"));
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_denoise_lum before restir_set_scene");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_denoise_lum between restir_halo_begin and restir_halo_end");
    restir_tile t;
    ST_TRY(frame_tile(tile, width, height, 0, t));
    const bool from_accum = params->variance_source == RESTIR_DENOISE_VAR_ACCUM;
    const auto& a = c->acc;
    if (from_accum) {
        if (!a.open) return fail(RESTIR_ERR_STATE, "restir_denoise_lum: RESTIR_DENOISE_VAR_ACCUM without an open accumulation");
        if (!(a.flags & RESTIR_ACCUM_VARIANCE))
            return fail(RESTIR_ERR_STATE, "restir_denoise_lum: RESTIR_DENOISE_VAR_ACCUM needs RESTIR_ACCUM_VARIANCE");
        if (a.frames < 2)
            return fail(RESTIR_ERR_STATE, "restir_denoise_lum: RESTIR_DENOISE_VAR_ACCUM needs two frames, %u are accumulated", a.frames);
        if (t.width != a.width || t.height != a.height)
            return fail(RESTIR_ERR_STATE, "restir_denoise_lum: the accumulation is %ux%u, the owned rectangle %ux%u", a.width,
                        a.height, t.width, t.height);
    } else {
        if ((c->rgb_from != restir_ctx::RGB_PRODUCED && c->rgb_from != restir_ctx::RGB_RESOLVED) || (size_t)c->rgb_w * c->rgb_h == 0)
            return fail(RESTIR_ERR_STATE, "restir_denoise_lum: nothing rendered yet");
        if (t.width != c->rgb_w || t.height != c->rgb_h)
            return fail(RESTIR_ERR_STATE, "restir_denoise_lum: the last image is %ux%u, the owned rectangle %ux%u", c->rgb_w,
                        c->rgb_h, t.width, t.height);
    }
    HIP_TRY(hipSetDevice(c->device));

    const size_t npx = (size_t)t.width * t.height;
    const restir_denoise_params& geo = params->geo;
    const uint32_t levels = geo.iterations;
    DenoiseView view;
    // every buffer first: a refused allocation leaves the image as it was
    ST_TRY(denoise_guides_alloc(c, cam, width, height, t, view));
    ST_TRY(c->dn_tmp[0].ensure(npx * 12));
    if (levels > 2u) ST_TRY(c->dn_tmp[1].ensure(npx * 12));
    c->dn_var_px = 0;
    ST_TRY(c->dn_var[0].ensure(npx * 4));
    ST_TRY(c->dn_var[1].ensure(npx * 4));
    if (from_accum && (c->rgb.bytes < npx * 12 || !c->rgb.p)) {   // a render of another size may have come between
        c->rgb_from = restir_ctx::RGB_NONE;
        ST_TRY(c->rgb.ensure(npx * 12));
    }
    set_launch_events(nullptr, nullptr);   // no RESTIR_K_* slot: restir_timings does not see these launches
    ST_TRY(denoise_guides_trace(c, width, height, t, view));
    c->stage_ok = false;

    FeaturesDev tf{};
    if (tone) {
        tf.tone_map = tone->enable_tone_mapping;
        tf.gamma = tone->gamma;
        tf.exposure = tone->exposure;
    }
    const float4 *n_t = c->dn_nt.as<float4>(), *ga = c->dn_ga.as<float4>(), *pf = c->dn_pf.as<float4>();
    float* rgb = c->rgb.as<float>();
    if (from_accum) {
        // the mean becomes the image, as restir_accum_resolve(ctx, NULL) would write it; the accumulation is only read
        c->image_pending(a.width, a.height);
        const float inv = 1.0f / ((float)a.frames * (float)(a.frames - 1u));
        HIP_TRY(launch_denoise_var_accum(a.mean.as<float>(), a.m2.as<float>(), rgb, c->dn_var[0].as<float>(), npx, inv, c->stream));
    } else {
        c->rgb_from = restir_ctx::RGB_PENDING;   // (a launch the device refuses leaves the buffer without an image)
        HIP_TRY(launch_denoise_var_spatial(rgb, c->dn_var[0].as<float>(), n_t, ga, pf, t.width, t.height, geo.normal_power_log2,
                                           geo.sigma_plane, c->stream));
    }
    const float* in = rgb;
    if (levels == 1u) {
        HIP_TRY(hipMemcpyAsync(c->dn_tmp[0].p, rgb, npx * 12, hipMemcpyDeviceToDevice, c->stream));
        in = c->dn_tmp[0].as<float>();
    }
    for (uint32_t level = 0; level < levels; level++) {
        const bool last = level + 1u == levels;
        float* out = last ? rgb : c->dn_tmp[level & 1u].as<float>();
        HIP_TRY(launch_denoise_level_lum(in, out, c->dn_var[level & 1u].as<float>(), c->dn_var[(level + 1u) & 1u].as<float>(), n_t, ga,
                                         pf, t.width, t.height, level, geo.normal_power_log2, geo.sigma_plane, params->sigma_lum,
                                         last ? &tf : nullptr, c->stream));
        in = out;
    }
    c->rgb_from = restir_ctx::RGB_RESOLVED;
    c->dn_var_last = levels & 1u;
    c->dn_var_px = npx;
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, npx * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

restir_status restir_denoise_lum_variance_download(restir_ctx* c, float* var, size_t count) {
    if (!c || !var) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->dn_var_px == 0) return fail(RESTIR_ERR_STATE, "restir_denoise_lum_variance_download: no restir_denoise_lum result is kept");
    if (count < c->dn_var_px) return fail(RESTIR_ERR_INVALID, "buffer holds %zu floats, need %zu", count, c->dn_var_px);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(var, c->dn_var[c->dn_var_last].p, c->dn_var_px * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_denoise_guide_builds(restir_ctx* c, uint64_t* out) {
    if (!c || !out) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->dn_guide_builds;
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the reprojected image history (include/restir_c.h "a reprojected image history", history.h, DESIGN.md §6 "Image
// history").  Like the denoiser, nothing here reads or writes the frame path's G-buffer planes or what is built over
// them, the frame index or the stage buffers; an advance leaves the image as it is.
static void history_close(restir_ctx* c) {
    auto& hs = c->hist;
    hs.open = hs.have = false;
    hs.width = hs.height = 0;
    hs.planes.release();
    hs.map.release();
}

restir_status restir_history_begin(restir_ctx* c, const restir_history_params* params) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    ST_TRY(history_params_check(params, "restir_history_begin"));
    std::lock_guard<std::mutex> lk(c->mu);
    auto& hs = c->hist;
    hs.open = true;
    hs.have = false;
    hs.params = *params;
    hs.width = hs.height = 0;
    hs.set = 0;
    hs.added_serial = 0;
    hs.advances = hs.resets = 0;
    return RESTIR_OK;
}

restir_status restir_history_advance(restir_ctx* c, const restir_camera* cam, uint32_t width, uint32_t height, uint32_t* out_map) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (!cam) return fail(RESTIR_ERR_INVALID, "restir_history_advance: camera is NULL");
    if (width == 0 || height == 0) return fail(RESTIR_ERR_INVALID, "restir_history_advance: empty image %ux%u", width, height);
    restir_camera_frame cf;
    restir_camera_derive(cam, &cf);
    if (!camera_frame_finite(cf)) return fail(RESTIR_ERR_INVALID, "restir_history_advance: the camera's derived frame is not finite");
    std::lock_guard<std::mutex> lk(c->mu);
    auto& hs = c->hist;
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_history_advance before restir_set_scene");
    if (!hs.open) return fail(RESTIR_ERR_STATE, "restir_history_advance before restir_history_begin");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_history_advance between restir_halo_begin and restir_halo_end");
    if (c->rgb_from == restir_ctx::RGB_RESOLVED)
        return fail(RESTIR_ERR_STATE, "restir_history_advance: the last image is a resolve's or a denoiser's, not a frame");
    if (c->rgb_from != restir_ctx::RGB_PRODUCED || (size_t)c->rgb_w * c->rgb_h == 0)
        return fail(RESTIR_ERR_STATE, "restir_history_advance: nothing rendered yet");
    if (hs.width && (hs.width != width || hs.height != height))
        return fail(RESTIR_ERR_STATE, "restir_history_advance: the view is %ux%u, the history %ux%u", width, height, hs.width, hs.height);
    if (c->rgb_w != width || c->rgb_h != height)
        return fail(RESTIR_ERR_UNSUPPORTED, "restir_history_advance: the last image is %ux%u, not the whole %ux%u view (a screen tile's?)",
                    c->rgb_w, c->rgb_h, width, height);
    if (hs.added_serial == c->rgb_serial) return fail(RESTIR_ERR_STATE, "restir_history_advance: the last image was folded already");
    restir_tile t;
    ST_TRY(frame_tile(nullptr, width, height, 0, t));
    HIP_TRY(hipSetDevice(c->device));

    // every buffer first: a refused allocation leaves the image as it was (and closes the history)
    const size_t npx = (size_t)width * height;
    DenoiseView view;
    restir_status st = denoise_guides_alloc(c, cam, width, height, t, view);
    if (st == RESTIR_OK) st = hs.planes.ensure(npx * 16 * 6);
    if (st == RESTIR_OK && out_map) st = hs.map.ensure(npx * 4);
    if (st != RESTIR_OK) { history_close(c); return st; }
    set_launch_events(nullptr, nullptr);   // no RESTIR_K_* slot: restir_timings does not see these launches
    ST_TRY(denoise_guides_trace(c, width, height, t, view));
    c->stage_ok = false;   // like restir_denoise: the stage API is to be configured again

    restir_camera_frame pf;
    restir_camera_derive(&hs.cam, &pf);
    HistoryDev a{};
    a.prev_cam = reproj_cam(hs.have ? pf : cf, width, height);
    a.miss_mat = c->sdev.num_materials - 1u;
    a.max_frames = hs.params.max_frames;
    a.fresh = hs.have ? 0u : 1u;
    a.cur_nt = c->dn_nt.as<float4>(); a.cur_pf = c->dn_pf.as<float4>(); a.cur_ga = c->dn_ga.as<float4>();
    a.x = c->rgb.as<float>();
    float4* pl = hs.planes.as<float4>();
    const int in = hs.set, out = hs.set ^ 1;
    a.in_a = pl + (size_t)(3 * in) * npx; a.in_b = a.in_a + npx; a.in_c = a.in_b + npx;
    a.out_a = pl + (size_t)(3 * out) * npx; a.out_b = a.out_a + npx; a.out_c = a.out_b + npx;
    a.map = out_map ? hs.map.as<uint32_t>() : nullptr;
    a.gather = hs.gather;
    HIP_TRY(launch_history_advance(a, c->stream));
    hs.set = out;
    hs.have = true;
    hs.width = width; hs.height = height;
    hs.cam = *cam;
    hs.added_serial = c->rgb_serial;
    hs.advances++;
    if (out_map) {
        HIP_TRY(hipMemcpyAsync(out_map, hs.map.p, npx * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

// the mode is plain context state: no frame, no cache and no open history is touched
restir_status restir_history_gather_set(restir_ctx* c, uint32_t gather) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (gather > RESTIR_HISTORY_GATHER_BILINEAR) return fail(RESTIR_ERR_INVALID, "restir_history_gather_set: gather %u (0 or 1)", gather);
    std::lock_guard<std::mutex> lk(c->mu);
    c->hist.gather = gather;
    return RESTIR_OK;
}

restir_status restir_history_gather_get(restir_ctx* c, uint32_t* gather) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (!gather) return fail(RESTIR_ERR_INVALID, "restir_history_gather_get: gather is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    *gather = c->hist.gather;
    return RESTIR_OK;
}

restir_status restir_history_resolve(restir_ctx* c, const restir_features* tone) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    auto& hs = c->hist;
    if (!hs.open || !hs.have) return fail(RESTIR_ERR_STATE, "restir_history_resolve: the history holds no advance");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_history_resolve between restir_halo_begin and restir_halo_end");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t px = (uint64_t)hs.width * hs.height;
    ST_TRY(c->rgb.ensure(px * 12));   // a render of another size may have come between
    c->image_pending(hs.width, hs.height);
    FeaturesDev d{};
    if (tone) {
        d.tone_map = tone->enable_tone_mapping;
        d.gamma = tone->gamma;
        d.exposure = tone->exposure;
    }
    HIP_TRY(launch_history_resolve(hs.planes.as<float4>() + (size_t)(3 * hs.set + 1) * px, c->rgb.as<float>(), px, d, c->stream));
    c->rgb_from = restir_ctx::RGB_RESOLVED;
    return RESTIR_OK;
}

// restir_denoise_lum's levels over the history's mean; the initial plane and the packed mean image come from
// k_history_var_fused, or (tuning history.var_fused = 0) from the three-launch form that computes the spatial estimate everywhere
restir_status restir_history_denoise(restir_ctx* c, const restir_denoise_lum_params* params, const restir_features* tone,
                                     float* out_rgb) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    ST_TRY(denoise_lum_params_check(params, "restir_history_denoise"));
    std::lock_guard<std::mutex> lk(c->mu);
    auto& hs = c->hist;
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_history_denoise before restir_set_scene");
    if (!hs.open || !hs.have) return fail(RESTIR_ERR_STATE, "restir_history_denoise: the history holds no advance");
    if (c->halo.active) return fail(RESTIR_ERR_STATE, "restir_history_denoise between restir_halo_begin and restir_halo_end");
    restir_tile t;
    ST_TRY(frame_tile(nullptr, hs.width, hs.height, 0, t));
    HIP_TRY(hipSetDevice(c->device));

    const size_t npx = (size_t)hs.width * hs.height;
    const restir_denoise_params& geo = params->geo;
    const uint32_t levels = geo.iterations;
    DenoiseView view;
    // every buffer first: a refused allocation leaves the image as it was
    ST_TRY(denoise_guides_alloc(c, &hs.cam, hs.width, hs.height, t, view));
    ST_TRY(c->dn_tmp[0].ensure(npx * 12));
    if (levels > 2u) ST_TRY(c->dn_tmp[1].ensure(npx * 12));
    c->dn_var_px = 0;
    ST_TRY(c->dn_var[0].ensure(npx * 4));
    ST_TRY(c->dn_var[1].ensure(npx * 4));
    if (c->rgb.bytes < npx * 12 || !c->rgb.p) {   // a render of another size may have come between
        c->rgb_from = restir_ctx::RGB_NONE;
        ST_TRY(c->rgb.ensure(npx * 12));
    }
    set_launch_events(nullptr, nullptr);   // no RESTIR_K_* slot
    ST_TRY(denoise_guides_trace(c, hs.width, hs.height, t, view));
    c->stage_ok = false;

    FeaturesDev tf{};
    if (tone) {
        tf.tone_map = tone->enable_tone_mapping;
        tf.gamma = tone->gamma;
        tf.exposure = tone->exposure;
    }
    const float4 *n_t = c->dn_nt.as<float4>(), *ga = c->dn_ga.as<float4>(), *pf = c->dn_pf.as<float4>();
    const float4* hb = hs.planes.as<float4>() + (size_t)(3 * hs.set + 1) * npx;
    float* rgb = c->rgb.as<float>();
    // the mean becomes the image, as restir_history_resolve(ctx, NULL) would write it; the history is only read
    c->image_pending(hs.width, hs.height);
    if (hs.var_fused) {
        HIP_TRY(launch_history_var_fused(hb, hb + npx, rgb, c->dn_var[0].as<float>(), n_t, ga, pf, t.width, t.height,
                                         hs.params.spatial_below, geo.normal_power_log2, geo.sigma_plane, c->stream));
    } else {   // the spatial estimate everywhere, the history's entries written over it: the same bits in three launches
        HIP_TRY(launch_history_resolve(hb, rgb, npx, FeaturesDev{}, c->stream));
        HIP_TRY(launch_denoise_var_spatial(rgb, c->dn_var[0].as<float>(), n_t, ga, pf, t.width, t.height, geo.normal_power_log2,
                                           geo.sigma_plane, c->stream));
        HIP_TRY(launch_history_var(hb, hb + npx, c->dn_var[0].as<float>(), npx, hs.params.spatial_below, c->stream));
    }
    const float* in = rgb;
    if (levels == 1u) {
        HIP_TRY(hipMemcpyAsync(c->dn_tmp[0].p, rgb, npx * 12, hipMemcpyDeviceToDevice, c->stream));
        in = c->dn_tmp[0].as<float>();
    }
    for (uint32_t level = 0; level < levels; level++) {
        const bool last = level + 1u == levels;
        float* out = last ? rgb : c->dn_tmp[level & 1u].as<float>();
        HIP_TRY(launch_denoise_level_lum(in, out, c->dn_var[level & 1u].as<float>(), c->dn_var[(level + 1u) & 1u].as<float>(), n_t, ga,
                                         pf, t.width, t.height, level, geo.normal_power_log2, geo.sigma_plane, params->sigma_lum,
                                         last ? &tf : nullptr, c->stream));
        in = out;
    }
    c->rgb_from = restir_ctx::RGB_RESOLVED;
    c->dn_var_last = levels & 1u;
    c->dn_var_px = npx;
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, npx * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

restir_status restir_history_download(restir_ctx* c, float* mean, float* S, uint32_t* n, size_t pixels) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    auto& hs = c->hist;
    if (!hs.open || !hs.have) return fail(RESTIR_ERR_STATE, "restir_history_download: the history holds no advance");
    const size_t npx = (size_t)hs.width * hs.height;
    if (pixels < npx) return fail(RESTIR_ERR_INVALID, "buffer holds %zu pixels, need %zu", pixels, npx);
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> host(npx * 8);   // the (mean, n) and (S, material) planes
    HIP_TRY(hipMemcpyAsync(host.data(), hs.planes.as<float4>() + (size_t)(3 * hs.set + 1) * npx, npx * 32, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < npx; i++) {
        const float* b = host.data() + 4 * i;
        const float* s = host.data() + 4 * (npx + i);
        if (mean) std::memcpy(mean + 3 * i, b, 12);
        if (S) std::memcpy(S + 3 * i, s, 12);
        if (n) n[i] = f2u(b[3]);
    }
    return RESTIR_OK;
}

restir_status restir_history_frames(restir_ctx* c, uint64_t* advances, uint64_t* resets) {
    if (!c || !advances || !resets) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->hist.open) return fail(RESTIR_ERR_STATE, "restir_history_frames before restir_history_begin");
    *advances = c->hist.advances;
    *resets = c->hist.resets;
    return RESTIR_OK;
}

restir_status restir_history_end(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    history_close(c);   // (hipFree waits for the kernels that use the planes)
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// stage API (parity tests): a whole width x height image, reservoir slot 0 = "current", slot 1 = "prev"
restir_status restir_stage_configure(restir_ctx* c, uint32_t width, uint32_t height, uint32_t n) {
    if (!c || width == 0 || height == 0 || n < 1 || n > RESTIR_MAX_N) return fail(RESTIR_ERR_INVALID, "bad stage size");
    std::lock_guard<std::mutex> lk(c->mu);
    c->gbuf.valid = false; ahead_drop(c);   // the stages write the frame path's G-buffer planes
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(ensure_work(c, width, height, n, true));
    ST_TRY(c->rgb.ensure((size_t)width * height * 12));
    c->image_pending(width, height);
    c->stage_rg = make_region(width, height, 0, 0, width, height, 0, 0, width, height);
    c->stage_ok = true;
    c->cur = 0;
    return RESTIR_OK;
}

static restir_status stage_buffer(restir_ctx* c, restir_buffer which, DevBuf** out, size_t* bytes) {
    const size_t npx = (size_t)c->vw * c->vh;
    const int cur = c->cur, prv = c->cur ^ 1;
    switch (which) {
        case RESTIR_BUF_GBUF_N_T: *out = &c->n_t; *bytes = npx * 16; break;
        case RESTIR_BUF_GBUF_P_MAT: *out = &c->p_mat; *bytes = npx * 16; break;
        case RESTIR_BUF_RES_A: *out = &c->ra[cur]; *bytes = npx * c->N * 16; break;
        case RESTIR_BUF_RES_B: *out = &c->rb[cur]; *bytes = npx * c->N * 16; break;
        case RESTIR_BUF_RES_DBG: *out = &c->dbg[cur]; *bytes = npx * c->N * 8; break;
        case RESTIR_BUF_PREV_A: *out = &c->ra[prv]; *bytes = npx * c->N * 16; break;
        case RESTIR_BUF_PREV_B: *out = &c->rb[prv]; *bytes = npx * c->N * 16; break;
        case RESTIR_BUF_PREV_DBG: *out = &c->dbg[prv]; *bytes = npx * c->N * 8; break;
        case RESTIR_BUF_RGB: *out = &c->rgb; *bytes = (size_t)c->rgb_w * c->rgb_h * 12; break;
        case RESTIR_BUF_GBUF_UV:
            if (!c->sdev.num_textures) return fail(RESTIR_ERR_INVALID, "gbuf_uv: the scene has no textures");
            ST_TRY(c->uv.ensure(npx * 8));
            *out = &c->uv; *bytes = npx * 8; break;
        case RESTIR_BUF_MIS_NBR:
            if (!c->mis_cap) return fail(RESTIR_ERR_STATE, "MIS buffers: call restir_stage_mis_capacity first");
            *out = &c->mis_nbr; *bytes = (size_t)(1u + c->mis_cap) * npx * 4; break;
        case RESTIR_BUF_MIS_ACC:
            if (!c->mis_cap) return fail(RESTIR_ERR_STATE, "MIS buffers: call restir_stage_mis_capacity first");
            *out = &c->mis_acc; *bytes = (size_t)c->mis_rows * npx * 4; break;
        default: return fail(RESTIR_ERR_INVALID, "unknown buffer %d", (int)which);
    }
    return RESTIR_OK;
}

restir_status restir_stage_upload(restir_ctx* c, restir_buffer which, const void* host, size_t bytes) {
    if (!c || !host) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    c->gbuf.valid = false; ahead_drop(c);
    if (!c->stage_ok) return fail(RESTIR_ERR_STATE, "restir_stage_configure first");
    DevBuf* b;
    size_t need;
    ST_TRY(stage_buffer(c, which, &b, &need));
    if (bytes != need) return fail(RESTIR_ERR_INVALID, "buffer %d: %zu bytes given, %zu expected", (int)which, bytes, need);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(b->p, host, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (which == RESTIR_BUF_RGB) c->image_produced();
    return RESTIR_OK;
}

restir_status restir_stage_download(restir_ctx* c, restir_buffer which, void* host, size_t bytes) {
    if (!c || !host) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    c->gbuf.valid = false; ahead_drop(c);   // (stage_buffer may allocate the uv plane)
    if (!c->stage_ok) return fail(RESTIR_ERR_STATE, "restir_stage_configure first");
    DevBuf* b;
    size_t need;
    ST_TRY(stage_buffer(c, which, &b, &need));
    if (bytes != need) return fail(RESTIR_ERR_INVALID, "buffer %d: %zu bytes given, %zu expected", (int)which, bytes, need);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(host, b->p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

#define STAGE_PRELUDE()                                                             \
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");                         \
    std::lock_guard<std::mutex> lk(c->mu);                                          \
    c->gbuf.valid = false; ahead_drop(c);                                                        \
    if (!c->stage_ok) return fail(RESTIR_ERR_STATE, "restir_stage_configure first"); \
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_set_scene first");      \
    HIP_TRY(hipSetDevice(c->device));                                               \

// The stage API's buffers: a stage reads the current grid and writes it in place (RIS) or, `advance`, its partner
static LaunchBufs stage_bufs(restir_ctx* c, const CameraDev& cam, uint32_t key, bool advance) {
    const int cur = c->cur, out = advance ? cur ^ 1 : cur;
    LaunchBufs b;
    b.key = key; b.cam = &cam; b.origin = cam.origin;
    b.n_t = c->n_t.as<float4>(); b.p_mat = c->p_mat.as<float4>();
    b.ia = c->ra[cur].as<float4>(); b.ib = c->rb[cur].as<float4>();
    b.oa = c->ra[out].as<float4>(); b.ob = c->rb[out].as<float4>();
    b.dbg = c->dbg[out].as<float2>();
    b.rgb = c->rgb.as<float>();
    return b;
}

restir_status restir_stage_primary(restir_ctx* c, const restir_camera* cam) {
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    STAGE_PRELUDE();
    const CameraDev camd = camera_dev(cam);
    FeaturesDev d{};
    d.texture = 1u;
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    TIMED(c, RESTIR_K_PRIMARY, launch_primary(route_primary(sd, c->stage_rg, c->tuning), sd, c->stage_rg,
                                              stage_bufs(c, camd, 0u, false), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

static restir_status stage_features(restir_ctx* c, const restir_features* f, FeaturesDev& d) {
    ST_TRY(check_features(f));
    if (f->num_samples_in_reservoir != c->N)
        return fail(RESTIR_ERR_INVALID, "N=%u but stage configured for N=%u", f->num_samples_in_reservoir, c->N);
    d = to_dev(f);
    return RESTIR_OK;
}

restir_status restir_stage_ris(restir_ctx* c, const restir_camera* cam, const restir_features* f, uint32_t key, int debug) {
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    const CameraDev camd = camera_dev(cam);
    Ask ask;
    ask.dbg = debug != 0;
    TIMED(c, RESTIR_K_RIS, launch_ris(route_ris(sd, c->stage_rg, d, c->tuning, ask), sd, c->stage_rg, d,
                                      stage_bufs(c, camd, key, false), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_stage_temporal(restir_ctx* c, const restir_camera* cam, const restir_features* f, uint32_t key,
                                    int debug) {
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    const CameraDev camd = camera_dev(cam);
    const int cur = c->cur, prv = cur ^ 1;
    TIMED(c, RESTIR_K_TEMPORAL,
          launch_temporal(sd, c->stage_rg, d, key, camd.origin, c->n_t.as<float4>(), c->p_mat.as<float4>(),
                          c->ra[cur].as<float4>(), c->rb[cur].as<float4>(), c->ra[prv].as<float4>(), c->rb[prv].as<float4>(),
                          c->ra[cur].as<float4>(), c->rb[cur].as<float4>(), debug ? c->dbg[cur].as<float2>() : nullptr,
                          nullptr, nullptr, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_stage_spatial(restir_ctx* c, const restir_camera* cam, const restir_features* f, uint32_t key,
                                   int debug) {
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    const CameraDev camd = camera_dev(cam);
    const int cur = c->cur, nxt = cur ^ 1;
    Ask ask;
    ask.dbg = debug != 0;
    TIMED(c, RESTIR_K_SPATIAL, launch_spatial(route_spatial(sd, c->stage_rg, d, c->tuning, ask), sd, c->stage_rg, d,
                                              stage_bufs(c, camd, key, true), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->cur = nxt;   // the pass output becomes "current" (RES_*), its input "prev" (PREV_*)
    return RESTIR_OK;
}

restir_status restir_stage_final(restir_ctx* c, const restir_camera* cam, const restir_features* f) {
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    const CameraDev camd = camera_dev(cam);
    TIMED(c, RESTIR_K_FINAL, launch_final(route_final(sd, c->stage_rg, d, c->tuning, Ask{}), sd, c->stage_rg, d,
                                          stage_bufs(c, camd, 0u, false), c->stream));
    c->image_produced();
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_stage_mis_capacity(restir_ctx* c, const restir_features* f, uint32_t* out_cap) {
    if (!out_cap) return fail(RESTIR_ERR_INVALID, "out_cap is NULL");
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    ST_TRY(ensure_mis(c, f, c->vw, c->vh));
    *out_cap = c->mis_cap;
    return RESTIR_OK;
}

restir_status restir_stage_neighbours(restir_ctx* c, const restir_features* f, uint32_t key_similar, uint32_t key_dissimilar) {
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    ST_TRY(ensure_mis(c, f, c->vw, c->vh));
    TIMED(c, RESTIR_K_MIS, launch_mis_neighbours(sd, c->vw, c->vh, d, key_similar, key_dissimilar, c->n_t.as<float4>(),
                                                 c->p_mat.as<float4>(), c->mis_nbr.as<uint32_t>(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_stage_mis_accumulate(restir_ctx* c, const restir_camera* cam, const restir_features* f, uint32_t iteration) {
    if (!cam) return fail(RESTIR_ERR_INVALID, "camera is NULL");
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    ST_TRY(check_romis_window(f, c->vw, c->vh));
    ST_TRY(ensure_mis(c, f, c->vw, c->vh));
    const CameraDev camd = camera_dev(cam);
    const int cur = c->cur;
    if (iteration == 0) HIP_TRY(hipMemsetAsync(c->mis_acc.p, 0, (size_t)c->mis_rows * c->vw * c->vh * 4, c->stream));
    TIMED(c, RESTIR_K_MIS, launch_mis_accumulate(sd, c->vw, c->vh, d, camd.origin, c->n_t.as<float4>(), c->p_mat.as<float4>(),
                                                 c->mis_nbr.as<uint32_t>(), c->ra[cur].as<float4>(), c->rb[cur].as<float4>(),
                                                 c->dbg[cur].as<float2>(), iteration, c->mis_acc.as<float>(),
                                                 c->mis_smp.as<float>(), c->mis_smp_samples, c->tuning, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_stage_mis_finish(restir_ctx* c, const restir_features* f) {
    STAGE_PRELUDE();
    FeaturesDev d;
    ST_TRY(stage_features(c, f, d));
    SceneDev sd;
    ST_TRY(scene_for(c, d, (size_t)c->vw * c->vh, sd));
    if (!c->mis_cap) return fail(RESTIR_ERR_STATE, "MIS buffers: run restir_stage_mis_accumulate first");
    TIMED(c, RESTIR_K_MIS, launch_mis_finish(c->vw, c->vh, d, c->mis_acc.as<float>(), c->rgb.as<float>(), c->stream));
    c->image_produced();
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_debug_cod_solve(restir_ctx* c, uint32_t n, const float* A, const float* b, float* x, size_t count) {
    if (!c || (count && (!A || !b || !x))) return fail(RESTIR_ERR_INVALID, "null argument");
    if (n < 1 || n > RESTIR_ROMIS_MAX_TECHNIQUES) return fail(RESTIR_ERR_INVALID, "n = %u outside 1..%u", n, RESTIR_ROMIS_MAX_TECHNIQUES);
    if (count > 0xFFFFFFFFull) return fail(RESTIR_ERR_INVALID, "count too large");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf bA, bb, bx;
    ST_TRY(bA.upload(A, count * n * n * 4, c->stream));
    ST_TRY(bb.upload(b, count * n * 4, c->stream));
    ST_TRY(bx.ensure(count * n * 4));
    hipError_t e = launch_debug_cod(n, bA.as<float>(), bb.as<float>(), bx.as<float>(), (uint32_t)count, c->stream);
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "debug cod launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(x, bx.p, count * n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bA.release(); bb.release(); bx.release();
    return RESTIR_OK;
}

restir_status restir_debug_math(restir_ctx* c, const float* x, const float* y, float* out_pow, float* out_exp, size_t n) {
    if (!c || (n && (!x || !y || !out_pow || !out_exp))) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf bx, by, bp, be;
    ST_TRY(bx.upload(x, n * 4, c->stream));
    ST_TRY(by.upload(y, n * 4, c->stream));
    ST_TRY(bp.ensure(n * 4));
    ST_TRY(be.ensure(n * 4));
    hipError_t e = launch_debug_math(bx.as<float>(), by.as<float>(), bp.as<float>(), be.as<float>(), (uint32_t)n, c->stream);
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "debug math launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out_pow, bp.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_exp, be.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bx.release(); by.release(); bp.release(); be.release();
    return RESTIR_OK;
}

restir_status restir_background_pixels(restir_ctx* c, uint64_t* background, uint64_t* computed) {
    if (!c || !background || !computed) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *background = 0;
    *computed = c->last_px;
    if (!c->tmiss_w || !c->tmiss.p) return RESTIR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t ntx = (c->tmiss_w + 31u) / 32u, nty = (c->tmiss_h + 7u) / 8u;
    std::vector<uint8_t> flags((size_t)ntx * nty);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(flags.data(), c->tmiss.p, flags.size(), hipMemcpyDeviceToHost));
    uint64_t bg = 0;
    for (uint32_t ty = 0; ty < nty; ty++)
        for (uint32_t tx = 0; tx < ntx; tx++)
            if (flags[(size_t)ty * ntx + tx] == 0u)   // flag 0: a background tile (kernels.hip primary_ris_body)
                bg += (uint64_t)std::min(32u, c->tmiss_w - 32u * tx) * std::min(8u, c->tmiss_h - 8u * ty);
    *background = bg;
    return RESTIR_OK;
}

restir_status restir_gbuf_reuses(restir_ctx* c, uint64_t* out_frames) {
    if (!c || !out_frames) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_frames = c->gbuf_reuses;
    return RESTIR_OK;
}

restir_status restir_shadow_list_frames(restir_ctx* c, uint64_t* out_frames) {
    if (!c || !out_frames) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_frames = c->shadow_list_frames;
    return RESTIR_OK;
}

restir_status restir_shadow_vis_frames(restir_ctx* c, uint64_t* out_frames) {
    if (!c || !out_frames) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_frames = c->shadow_vis_frames;
    return RESTIR_OK;
}

restir_status restir_shadow_vis_builds(restir_ctx* c, uint64_t* out_builds) {
    if (!c || !out_builds) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_builds = c->shadow_vis_builds;
    return RESTIR_OK;
}

restir_status restir_phat_frames(restir_ctx* c, uint64_t* out_frames) {
    if (!c || !out_frames) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_frames = c->phat_frames;
    return RESTIR_OK;
}

restir_status restir_phat_builds(restir_ctx* c, uint64_t* out_builds) {
    if (!c || !out_builds) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_builds = c->phat_builds;
    return RESTIR_OK;
}

restir_status restir_ahead_frames(restir_ctx* c, uint64_t* out_frames) {
    if (!c || !out_frames) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_frames = c->ahead.frames;
    return RESTIR_OK;
}

restir_status restir_ahead_discards(restir_ctx* c, uint64_t* out_discards) {
    if (!c || !out_discards) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_discards = c->ahead.discards;
    return RESTIR_OK;
}

// restir_debug_phat between its buffer's allocation and its release
static restir_status debug_phat_run(restir_ctx* c, const PhatTableDev& d, uint32_t light, size_t n, DevBuf& bo, float* out) {
    ST_TRY(bo.ensure(n * sizeof(float)));
    hipError_t e = launch_debug_phat(d, light, bo.as<float>(), c->stream);
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "debug phat launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, bo.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_debug_phat(restir_ctx* c, uint32_t light, uint32_t width, uint32_t height, float* out_phat) {
    if (!c || !out_phat) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->phat_key.valid || !c->phat.p || !c->gbuf.valid || c->phat_key.gbuf_epoch != c->gbuf_epoch ||
        c->phat_key.scene_gen != c->scene_gen)
        return fail(RESTIR_ERR_STATE, "restir_debug_phat: no p-hat table of the kept G-buffer (a frame builds it)");
    const PhatTableDev& d = c->phat_dev;
    if (width != d.rg.rw || height != d.rg.rh)
        return fail(RESTIR_ERR_INVALID, "restir_debug_phat: the table covers %ux%u pixels, not %ux%u", d.rg.rw, d.rg.rh, width, height);
    if (light >= d.s.num_lights) return fail(RESTIR_ERR_INVALID, "restir_debug_phat: light %u >= %u", light, d.s.num_lights);
    DevBuf bo;
    const restir_status st = debug_phat_run(c, d, light, (size_t)width * height, bo, out_phat);
    bo.release();
    return st;
}

// restir_debug_shadow_vis between its buffer's allocation and its release
static restir_status debug_shadow_vis_run(restir_ctx* c, const ShadowVisDev& d, uint32_t light, size_t n, DevBuf& bo, uint8_t* out) {
    ST_TRY(bo.ensure(n));
    hipError_t e = launch_debug_shadow_vis(d, light, bo.as<uint8_t>(), c->stream);
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "debug shadow vis launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, bo.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_debug_shadow_vis(restir_ctx* c, uint32_t light, uint32_t width, uint32_t height, uint8_t* out_bits) {
    if (!c || !out_bits) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const restir_ctx::ShadowListsKey& k = c->slists_key;
    if (!c->has_scene || !c->gbuf.valid || !k.valid || k.gbuf_epoch != c->gbuf_epoch || k.scene_gen != c->scene_gen ||
        k.geom_gen != c->geom_gen || !c->svis_valid || !c->svis.p || c->svis_lists_build != c->slists_builds)
        return fail(RESTIR_ERR_STATE, "restir_debug_shadow_vis: no visibility bits of the kept G-buffer (a frame builds them)");
    const ShadowVisDev& d = c->svis_dev;
    if (light >= d.lists.s.num_lights) return fail(RESTIR_ERR_INVALID, "light %u of %u", light, d.lists.s.num_lights);
    if (width != d.lists.rg.rw || height != d.lists.rg.rh)
        return fail(RESTIR_ERR_INVALID, "the plane is %u x %u, the bits' rectangle %u x %u", width, height, d.lists.rg.rw,
                    d.lists.rg.rh);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf bo;
    const restir_status st = debug_shadow_vis_run(c, d, light, (size_t)width * height, bo, out_bits);
    bo.release();   // on every path
    return st;
}

// restir_debug_shadow_lists between its buffers' allocation and their release
static restir_status debug_shadow_lists_run(restir_ctx* c, const ShadowListsDev& d, uint32_t light, size_t n, DevBuf& bb, DevBuf& bl,
                                            uint8_t* out_bvh, uint8_t* out_list) {
    ST_TRY(bb.ensure(n));
    ST_TRY(bl.ensure(n));
    hipError_t e = launch_debug_shadow_lists(d, light, bb.as<uint8_t>(), bl.as<uint8_t>(), c->stream);
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "debug shadow lists launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out_bvh, bb.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_list, bl.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RESTIR_OK;
}

restir_status restir_debug_shadow_lists(restir_ctx* c, uint32_t light, uint32_t width, uint32_t height, uint8_t* out_bvh,
                                        uint8_t* out_list) {
    if (!c || !out_bvh || !out_list) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const restir_ctx::ShadowListsKey& k = c->slists_key;
    if (!c->has_scene || !c->gbuf.valid || !k.valid || k.gbuf_epoch != c->gbuf_epoch || k.scene_gen != c->scene_gen ||
        k.geom_gen != c->geom_gen)
        return fail(RESTIR_ERR_STATE, "restir_debug_shadow_lists: no shadow lists of the kept G-buffer (a frame builds them)");
    const ShadowListsDev& d = c->slists_dev;
    if (light > d.s.num_lights) return fail(RESTIR_ERR_INVALID, "light %u of %u (+ the zero sample)", light, d.s.num_lights);
    if (width != d.rg.rw || height != d.rg.rh)
        return fail(RESTIR_ERR_INVALID, "the planes are %u x %u, the lists' rectangle %u x %u", width, height, d.rg.rw, d.rg.rh);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf bb, bl;
    const restir_status st = debug_shadow_lists_run(c, d, light, (size_t)width * height, bb, bl, out_bvh, out_list);
    bb.release(); bl.release();   // on every path
    return st;
}

restir_status restir_scene_info(restir_ctx* c, struct restir_scene_info* out) {
    if (!c || !out) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_scene_info before restir_set_scene");
    const SceneDev& s = c->sdev;
    *out = {};
    out->num_nodes = s.num_nodes;
    out->num_tris = s.num_tris;
    out->bvh_lds_bytes = bvh_lds_bytes(s);
    out->num_lights = s.num_lights;
    out->light_types = s.light_types;
    out->lights_pgram = s.lights_pgram;
    out->lights_grid = s.lights_grid;
    out->lights_regular = s.lights_regular;
    out->grid_ny_log2 = s.grid_ny_log2;
    out->light_scale = s.light_scale;
    out->nodes_q_ok = s.nodes_q_ok;
    return RESTIR_OK;
}

restir_status restir_measure_read_bandwidth(restir_ctx* c, uint64_t bytes, uint32_t iters, double* out_gbps) {
    if (!c || !out_gbps || iters == 0 || bytes < (1u << 20)) return fail(RESTIR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n4 = (size_t)(bytes / 16);
    DevBuf buf, sink;
    ST_TRY(buf.ensure(n4 * 16));
    ST_TRY(sink.ensure(1 << 20));
    HIP_TRY(hipMemsetAsync(buf.p, 0, n4 * 16, c->stream));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipError_t e = launch_read_stream(buf.as<float4>(), n4, sink.as<float>(), c->stream);   // warm
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
    for (uint32_t i = 0; i < iters && e == hipSuccess; i++) e = launch_read_stream(buf.as<float4>(), n4, sink.as<float>(), c->stream);
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    buf.release();
    sink.release();
    if (e != hipSuccess) return fail(RESTIR_ERR_HIP, "read-bandwidth kernel: %s", hipGetErrorString(e));
    *out_gbps = (double)n4 * 16.0 * iters / (ms * 1e-3) / 1e9;
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// halo-mode frames (include/restir_c.h "Reservoir halo exchange"): the stages of restir_render with the
// ghost-zone recomputation replaced by an exchange of the owned border strips before each spatial pass
namespace {
restir_status to_segs(const restir_halo_segment* g, uint32_t n, HaloSegs& hs, uint64_t& bytes) {
    if (n > RESTIR_MAX_HALO_SEGS) return fail(RESTIR_ERR_INVALID, "halo: %u segments", n);
    hs = HaloSegs{};
    hs.n = n;
    uint64_t px = 0;
    bytes = 0;
    for (uint32_t i = 0; i < n; i++) {
        hs.x0[i] = g[i].x0; hs.y0[i] = g[i].y0; hs.w[i] = g[i].width; hs.h[i] = g[i].height;
        hs.px0[i] = (uint32_t)px;
        px += (uint64_t)g[i].width * g[i].height;
        bytes += g[i].bytes;
    }
    if (px >= (1ull << 31)) return fail(RESTIR_ERR_INVALID, "halo: %llu pixels", (unsigned long long)px);
    hs.px0[n] = (uint32_t)px;
    return RESTIR_OK;
}
}  // namespace

restir_status restir_halo_begin(restir_ctx* c, const restir_camera* cam, const restir_features* features, uint32_t width,
                                uint32_t height, uint32_t tiles_x, uint32_t tiles_y, uint32_t rank, const restir_frame* prev,
                                uint64_t* send_bytes, uint64_t* recv_bytes) {
    restir_tile_layout L;
    ST_TRY(restir_layout_even(width, height, tiles_x, tiles_y, &L));
    return restir_halo_begin_layout(c, cam, features, &L, rank, prev, send_bytes, recv_bytes);
}

restir_status restir_halo_begin_layout(restir_ctx* c, const restir_camera* cam, const restir_features* features,
                                       const restir_tile_layout* layout, uint32_t rank, const restir_frame* prev,
                                       uint64_t* send_bytes, uint64_t* recv_bytes) {
    if (!c || !cam) return fail(RESTIR_ERR_INVALID, "null argument");
    ST_TRY(check_features(features));
    ST_TRY(layout_check(layout));
    std::lock_guard<std::mutex> lk(c->mu);
    c->gbuf.valid = false; ahead_drop(c);   // a halo frame writes the same G-buffer planes and flags (and keeps the tracing kernels)
    if (!c->has_scene) return fail(RESTIR_ERR_STATE, "restir_halo_begin before restir_set_scene");
    HIP_TRY(hipSetDevice(c->device));
    const FeaturesDev f = to_dev(features);
    const uint32_t passes = features->spatial_reuse ? features->spatial_resampling_passes : 0u;
    const uint32_t width = layout->global_width, height = layout->global_height;
    const uint32_t tiles_x = layout->tiles_x, tiles_y = layout->tiles_y;
    restir_tile t{};
    ST_TRY(restir_layout_tile(layout, rank, passes ? f.R : 0u, &t));
    // plan into locals, validate everything, then commit to c->halo (a failure leaves no half-updated plan)
    restir_halo_segment sg[RESTIR_MAX_HALO_SEGS], rg_[RESTIR_MAX_HALO_SEGS];
    uint32_t n = 0;
    HaloSegs send{}, recv{};
    uint64_t send_b = 0, recv_b = 0;
    if (passes) {   // no spatial pass, no exchange: skip the plan (and its segment cap)
        n = RESTIR_MAX_HALO_SEGS;
        ST_TRY(restir_layout_halo_plan(layout, rank, f.R, f.N, sg, rg_, &n));
        ST_TRY(to_segs(sg, n, send, send_b));
        ST_TRY(to_segs(rg_, n, recv, recv_b));
    }
    const bool temporal = features->temporal_reuse && prev != nullptr;
    if (temporal) {
        ST_TRY(check_prev(c, prev, f.N, t, width, height, "tile's view", false));
        ST_TRY(use_prev(prev, c->device, c->stream, c->pool.get()));
    }
    auto& h = c->halo;
    h.active = false;
    FrameBufs fb;
    ST_TRY(ensure_records(c, t.gwidth, t.gheight, f.N, fb));
    c->stage_ok = false;
    h.send = send; h.recv = recv; h.send_bytes = send_b; h.recv_bytes = recv_b;
    for (uint32_t i = 0; i < n; i++) { h.send_rank[i] = sg[i].rank; h.recv_rank[i] = rg_[i].rank; }
    halo_ops_from(sg, rg_, n, h.ops);
    h.nops = 2 * n;
    h.rank = rank;
    h.nranks = tiles_x * tiles_y;
    h.interior_done = false;
    ST_TRY(c->rgb.ensure((size_t)t.width * t.height * 12));
    c->image_pending(t.width, t.height);
    h.W = width; h.H = height;
    h.view = fb.region(make_region(width, height, t.gx0, t.gy0, t.gwidth, t.gheight, t.gx0, t.gy0, t.gwidth, t.gheight));
    h.owned = fb.region(make_region(width, height, t.gx0, t.gy0, t.gwidth, t.gheight, t.x0, t.y0, t.width, t.height));
    h.fb_records = fb.records;
    h.f = f;
    h.camd = camera_dev(cam);
    h.frame = c->frame_index++;
    h.pass = 0;
    h.passes = passes;
    h.cur = 0;
    SceneDev s;
    ST_TRY(scene_for(c, f, (size_t)t.gwidth * t.gheight, s));
    float4* pm = c->p_mat.as<float4>();
    // G-buffer on the whole view (the spatial passes read the neighbours' depth / normal / position).  Without temporal
    // reuse: restir_render's fused primary + RIS kernel over the whole view, with its background-tile flags (the ring's
    // RIS results are the ones its owner computes -- same G-buffer, same global-pixel keys -- and the exchange before
    // the first pass overwrites them with those same values), so the passes and final shading write background tiles
    // without reading them; the ring's RIS costs (ring / tile) of the RIS time.  Otherwise primary rays on the view
    // and RIS / temporal reuse on the owned rectangle.
    const Ask ris_ask = frame_ris_ask(c, s, fb, temporal);
    const Route ris = route_primary_ris(s, h.view, f, c->tuning, ris_ask);
    LaunchBufs b = fb.bufs(h.camd, restir_rng_key(c->seed, h.frame, RESTIR_STAGE_RIS, 0), 0, 0);
    h.tmiss = nullptr;
    if (!temporal && c->tuning.fuse_primary_ris && ris.ok) {
        ST_TRY(ensure_tile_flags(c, ris, h.view, h.tmiss));
        b.flags = h.tmiss;
        TIMED(c, RESTIR_K_PRIMARY_RIS, launch_primary_ris(ris, s, h.view, f, b, c->stream));
    } else {
        TIMED(c, RESTIR_K_PRIMARY, launch_primary(route_primary(s, h.view, c->tuning), s, h.view, b, c->stream));
        TIMED(c, RESTIR_K_RIS, launch_ris(route_ris(s, h.owned, f, c->tuning, ris_ask), s, h.owned, f, b, c->stream));
    }
    if (temporal)
        TIMED(c, RESTIR_K_TEMPORAL,
              launch_temporal(s, h.owned, f, restir_rng_key(c->seed, h.frame, RESTIR_STAGE_TEMPORAL, 0), h.camd.origin, fb.nt(0),
                              pm, fb.ra(0), fb.rb(0), fb.pa(prev), fb.pb(prev), fb.ra(0), fb.rb(0), nullptr, fb.rp(0),
                              fb.rp(0), c->stream));
    if (temporal) used_prev(prev, c->stream, c->pool.get());
    h.rp_ok = fb.rp(0) != nullptr;
    h.active = true;
    if (send_bytes) *send_bytes = h.send_bytes;
    if (recv_bytes) *recv_bytes = h.recv_bytes;
    return RESTIR_OK;
}

restir_status restir_halo_pack(restir_ctx* c, void* buf, uint64_t bytes, int host_memory) {
    if (!c || (bytes && !buf)) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    auto& h = c->halo;
    if (!h.active || h.pass >= h.passes) return fail(RESTIR_ERR_STATE, "restir_halo_pack outside a halo frame's passes");
    if (bytes != h.send_bytes) return fail(RESTIR_ERR_INVALID, "halo send buffer is %llu bytes, plan needs %llu",
                                           (unsigned long long)bytes, (unsigned long long)h.send_bytes);
    HIP_TRY(hipSetDevice(c->device));
    float4* dst = static_cast<float4*>(buf);
    if (host_memory) { ST_TRY(c->halo_scratch.ensure(bytes)); dst = c->halo_scratch.as<float4>(); }
    const FrameBufs fb{c, h.fb_records, (size_t)h.view.vw * h.view.vh, h.f.N};
    HIP_TRY(launch_halo_pack(h.view, h.send, h.f.N, fb.ra(h.cur), fb.rb(h.cur), dst, c->stream));
    if (host_memory && bytes) HIP_TRY(hipMemcpyAsync(buf, dst, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's transport reads the buffer next
    return RESTIR_OK;
}

restir_status restir_halo_unpack(restir_ctx* c, const void* buf, uint64_t bytes, int host_memory) {
    if (!c || (bytes && !buf)) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    auto& h = c->halo;
    if (!h.active || h.pass >= h.passes) return fail(RESTIR_ERR_STATE, "restir_halo_unpack outside a halo frame's passes");
    if (bytes != h.recv_bytes) return fail(RESTIR_ERR_INVALID, "halo recv buffer is %llu bytes, plan needs %llu",
                                           (unsigned long long)bytes, (unsigned long long)h.recv_bytes);
    HIP_TRY(hipSetDevice(c->device));
    const float4* src = static_cast<const float4*>(buf);
    if (host_memory && bytes) {
        ST_TRY(c->halo_scratch.ensure(bytes));
        HIP_TRY(hipMemcpyAsync(c->halo_scratch.p, buf, bytes, hipMemcpyHostToDevice, c->stream));
        src = c->halo_scratch.as<float4>();
    }
    const FrameBufs fb{c, h.fb_records, (size_t)h.view.vw * h.view.vh, h.f.N};
    HIP_TRY(launch_halo_unpack(h.view, h.recv, h.f.N, src, fb.ra(h.cur), fb.rb(h.cur), c->stream));
    if (host_memory) HIP_TRY(hipStreamSynchronize(c->stream));   // the host buffer may be reused on return
    return RESTIR_OK;
}

// The owned rectangle of a halo pass split into the interior -- pixels at least R from every side that faces
// another tile, whose neighbourhoods (+-R, clamped to the image) stay inside the owned rectangle -- and up to
// four border strips (bottom / top full width, left / right between them) that read the exchanged ring.
// Per-pixel results do not depend on how the rectangle is split into launches (keyed RNG by global pixel id).
struct HaloSplit {
    Region part[5];   // part[0] = interior (may be empty), part[1..nb] = border strips
    uint32_t nb;
};
static HaloSplit halo_split(const Region& owned, uint32_t R) {
    const uint32_t x0 = owned.rx0, y0 = owned.ry0, x1 = x0 + owned.rw, y1 = y0 + owned.rh;
    const uint32_t l = x0 > 0 ? R : 0u, r = x1 < owned.W ? R : 0u, b = y0 > 0 ? R : 0u, t = y1 < owned.H ? R : 0u;
    const uint32_t ix0 = x0 + std::min(l, owned.rw), ix1 = std::max(ix0, x1 - std::min(r, owned.rw));
    const uint32_t iy0 = y0 + std::min(b, owned.rh), iy1 = std::max(iy0, y1 - std::min(t, owned.rh));
    auto rect = [&](uint32_t ax0, uint32_t ay0, uint32_t ax1, uint32_t ay1) {
        Region q = owned;
        q.rx0 = ax0; q.ry0 = ay0; q.rw = ax1 - ax0; q.rh = ay1 - ay0;
        return q;
    };
    HaloSplit hs{};
    hs.part[0] = rect(ix0, iy0, ix1, iy1);
    hs.nb = 0;
    if (iy0 > y0) hs.part[1 + hs.nb++] = rect(x0, y0, x1, iy0);
    if (y1 > iy1) hs.part[1 + hs.nb++] = rect(x0, iy1, x1, y1);
    if (iy1 > iy0 && ix0 > x0) hs.part[1 + hs.nb++] = rect(x0, iy0, ix0, iy1);
    if (iy1 > iy0 && x1 > ix1) hs.part[1 + hs.nb++] = rect(ix1, iy0, x1, iy1);
    return hs;
}

// one launch of the current pass over `rg` (a part of the owned rectangle); the pdf cache stays valid only if
// every part wrote it.  The cache covers the owned rectangle only (the exchange moves reservoirs, not their
// pdfs), so only the interior -- whose neighbourhoods stay inside it -- may read it at neighbour pixels.
static restir_status halo_spatial_part(restir_ctx* c, const Region& rg, bool interior, bool& rp_written) {
    auto& h = c->halo;
    const int nxt = h.cur ^ 1;
    const FrameBufs fb{c, h.fb_records, (size_t)h.view.vw * h.view.vh, h.f.N};
    SceneDev sd;
    ST_TRY(scene_for(c, h.f, (size_t)h.view.vw * h.view.vh, sd));
    Ask ask;
    ask.rp_in = h.rp_ok;
    ask.rp_nb = h.rp_ok && interior;
    ask.rp_out = fb.rp(nxt) != nullptr;
    // background tiles (restir_render's MissTiles): every ring pixel holds its owner's value, which for a background
    // tile is the known one
    ask.flags = h.tmiss != nullptr;
    ask.flags_m = (!h.f.unbiased || h.pass == 0) ? h.f.M : 0u;
    const Route r = route_spatial(sd, rg, h.f, c->tuning, ask);
    LaunchBufs b = fb.bufs(h.camd, restir_rng_key(c->seed, h.frame, RESTIR_STAGE_SPATIAL, h.pass), h.cur, nxt);
    b.flags = h.tmiss;
    TIMED(c, RESTIR_K_SPATIAL, launch_spatial(r, sd, rg, h.f, b, c->stream));
    rp_written = rp_written && r.rp_out;
    return RESTIR_OK;
}

static restir_status halo_interior_locked(restir_ctx* c) {
    auto& h = c->halo;
    if (!h.active || h.pass >= h.passes || h.interior_done)
        return fail(RESTIR_ERR_STATE, "restir_halo_spatial_interior: no pass pending");
    HIP_TRY(hipSetDevice(c->device));
    const HaloSplit hs = halo_split(h.owned, h.f.R);
    h.part_rp = true;
    if (hs.part[0].rw && hs.part[0].rh) ST_TRY(halo_spatial_part(c, hs.part[0], true, h.part_rp));
    h.interior_done = true;
    return RESTIR_OK;
}

static restir_status halo_border_locked(restir_ctx* c) {
    auto& h = c->halo;
    if (!h.active || h.pass >= h.passes || !h.interior_done)
        return fail(RESTIR_ERR_STATE, "restir_halo_spatial_border before the pass's interior");
    HIP_TRY(hipSetDevice(c->device));
    const HaloSplit hs = halo_split(h.owned, h.f.R);
    for (uint32_t i = 1; i <= hs.nb; i++) ST_TRY(halo_spatial_part(c, hs.part[i], false, h.part_rp));
    h.rp_ok = h.part_rp;
    h.cur ^= 1;
    h.pass++;
    h.interior_done = false;
    return RESTIR_OK;
}

restir_status restir_halo_spatial_interior(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    return halo_interior_locked(c);
}

restir_status restir_halo_spatial_border(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    return halo_border_locked(c);
}

restir_status restir_halo_spatial(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->halo.interior_done) ST_TRY(halo_interior_locked(c));
    return halo_border_locked(c);
}

// ---- native RCCL transport ----------------------------------------------------------------------------
}  // extern "C"

namespace {
struct RcclApi {
    bool ok = false;
    std::string why;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    decltype(&ncclCommCount) comm_count = nullptr;
    decltype(&ncclCommUserRank) comm_user_rank = nullptr;
};

const RcclApi& rccl_api() {
    static RcclApi api = [] {
        RcclApi a;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { a.why = dlerror() ? dlerror() : "librccl.so.1 not found"; return a; }
        bool all = true;
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
            all = all && fn != nullptr;
        };
        sym(a.get_unique_id, "ncclGetUniqueId");
        sym(a.comm_init_rank, "ncclCommInitRank");
        sym(a.comm_destroy, "ncclCommDestroy");
        sym(a.send, "ncclSend");
        sym(a.recv, "ncclRecv");
        sym(a.group_start, "ncclGroupStart");
        sym(a.group_end, "ncclGroupEnd");
        sym(a.error_string, "ncclGetErrorString");
        sym(a.comm_count, "ncclCommCount");
        sym(a.comm_user_rank, "ncclCommUserRank");
        a.ok = all;
        if (!all) a.why = "librccl lacks a symbol";
        return a;
    }();
    return api;
}
}  // namespace

extern "C" {

#define RCCL_TRY(expr)                                                                                            \
    do {                                                                                                          \
        const ncclResult_t rc_ = (expr);                                                                          \
        if (rc_ != ncclSuccess)                                                                                   \
            return fail(RESTIR_ERR_COMM, "%s: %s", #expr, rccl_api().error_string(rc_));                           \
    } while (0)

// inside an open ncclGroupStart: close the group before reporting the error, so the thread's RCCL group state
// does not leak into the next call
#define RCCL_GROUP_TRY(expr)                                                                                      \
    do {                                                                                                          \
        const ncclResult_t rc_ = (expr);                                                                          \
        if (rc_ != ncclSuccess) {                                                                                 \
            (void)rccl_api().group_end();                                                                         \
            return fail(RESTIR_ERR_COMM, "%s: %s", #expr, rccl_api().error_string(rc_));                           \
        }                                                                                                         \
    } while (0)

static void release_rccl(restir_ctx* c) {
    auto& q = c->rccl;
    // the context stream may still hold an unpack that waits on the transfer, and the communication stream the
    // transfer itself: drain both before the communicator and the streams go
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (q.stream) (void)hipStreamSynchronize(q.stream);
    if (q.comm && q.owned && rccl_api().ok) (void)rccl_api().comm_destroy(static_cast<ncclComm_t>(q.comm));
    q.comm = nullptr;
    q.owned = false;
    if (q.packed) (void)hipEventDestroy(q.packed);
    if (q.moved) (void)hipEventDestroy(q.moved);
    if (q.stream) (void)hipStreamDestroy(q.stream);
    q.packed = q.moved = nullptr;
    q.stream = nullptr;
    q.nranks = 0;
    q.rank = -1;
    q.send.release();
    q.recv.release();
}

// the communication stream and the pass's two events (a communicator's, or a record-only pass's)
static restir_status comm_stream_locked(restir_ctx* c) {
    auto& q = c->rccl;
    if (!q.stream) HIP_TRY(hipStreamCreateWithFlags(&q.stream, hipStreamNonBlocking));
    if (!q.packed) HIP_TRY(hipEventCreateWithFlags(&q.packed, hipEventDisableTiming));
    if (!q.moved) HIP_TRY(hipEventCreateWithFlags(&q.moved, hipEventDisableTiming));
    return RESTIR_OK;
}

static restir_status attach_comm_locked(restir_ctx* c, void* comm, bool owned) {
    auto& q = c->rccl;
    ST_TRY(comm_stream_locked(c));
    if (q.comm && q.owned) RCCL_TRY(rccl_api().comm_destroy(static_cast<ncclComm_t>(q.comm)));
    q.comm = comm;
    q.owned = owned;
    int n = 0, r = -1;
    RCCL_TRY(rccl_api().comm_count(static_cast<ncclComm_t>(comm), &n));
    RCCL_TRY(rccl_api().comm_user_rank(static_cast<ncclComm_t>(comm), &r));
    q.nranks = n;
    q.rank = r;
    c->halo_record = false;   // a communicator ends record-only mode: its passes move real reservoirs
    c->halo_log.clear();
    return RESTIR_OK;
}

restir_status restir_rccl_unique_id(void* out, size_t bytes) {
    if (!out || bytes < RESTIR_RCCL_ID_BYTES) return fail(RESTIR_ERR_INVALID, "restir_rccl_unique_id: need %u bytes", RESTIR_RCCL_ID_BYTES);
    static_assert(sizeof(ncclUniqueId) == RESTIR_RCCL_ID_BYTES, "ncclUniqueId size");
    const RcclApi& api = rccl_api();
    if (!api.ok) return fail(RESTIR_ERR_UNSUPPORTED, "RCCL unavailable: %s", api.why.c_str());
    ncclUniqueId id;
    RCCL_TRY(api.get_unique_id(&id));
    std::memcpy(out, &id, sizeof(id));
    return RESTIR_OK;
}

restir_status restir_halo_attach_rccl(restir_ctx* c, const void* unique_id, uint32_t nranks, uint32_t rank) {
    if (!c || !unique_id || nranks == 0 || rank >= nranks) return fail(RESTIR_ERR_INVALID, "restir_halo_attach_rccl: bad argument");
    const RcclApi& api = rccl_api();
    if (!api.ok) return fail(RESTIR_ERR_UNSUPPORTED, "RCCL unavailable: %s", api.why.c_str());
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    ncclComm_t comm = nullptr;
    RCCL_TRY(api.comm_init_rank(&comm, (int)nranks, id, (int)rank));
    return attach_comm_locked(c, comm, true);
}

restir_status restir_halo_attach_comm(restir_ctx* c, void* nccl_comm) {
    if (!c || !nccl_comm) return fail(RESTIR_ERR_INVALID, "restir_halo_attach_comm: null argument");
    const RcclApi& api = rccl_api();
    if (!api.ok) return fail(RESTIR_ERR_UNSUPPORTED, "RCCL unavailable: %s", api.why.c_str());
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return attach_comm_locked(c, nccl_comm, false);
}

restir_status restir_halo_pass(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    auto& h = c->halo;
    auto& q = c->rccl;
    const bool rec = c->halo_record;
    if (!q.comm && !rec) return fail(RESTIR_ERR_STATE, "restir_halo_pass before restir_halo_attach_rccl / _comm");
    if (!h.active || h.pass >= h.passes || h.interior_done) return fail(RESTIR_ERR_STATE, "restir_halo_pass: no pass pending");
    // the plan's peers are tile ranks: the communicator must hold exactly the tiles, with this context's tile at
    // its own rank, or the halos would go to the wrong peers
    if (!rec && (q.nranks != (int)h.nranks || q.rank != (int)h.rank))
        return fail(RESTIR_ERR_INVALID, "restir_halo_pass: communicator rank %d of %d, halo frame is tile %u of %u",
                    q.rank, q.nranks, h.rank, h.nranks);
    for (uint32_t i = 0; i < h.nops; i++)
        if (h.ops[i].peer >= h.nranks || h.ops[i].peer == h.rank)
            return fail(RESTIR_ERR_INVALID, "restir_halo_pass: operation %u peer %u outside the %u tiles", i, h.ops[i].peer,
                        h.nranks);
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(comm_stream_locked(c));
    ST_TRY(q.send.ensure(std::max<uint64_t>(h.send_bytes, 16)));
    ST_TRY(q.recv.ensure(std::max<uint64_t>(h.recv_bytes, 16)));
    const uint32_t pass = h.pass;
    auto log = [&](uint32_t what, uint32_t stream, uint32_t peer = 0, uint64_t off = 0, uint64_t bytes = 0) {
        if (rec) c->halo_log.push_back(restir_halo_event{what, stream, peer, pass, off, bytes});
    };
    const FrameBufs fb{c, h.fb_records, (size_t)h.view.vw * h.view.vh, h.f.N};
    // context stream: pack (after the previous pass's transfer released the send buffer -- stream order:
    // the previous pass waited on q.moved before its unpack)
    HIP_TRY(launch_halo_pack(h.view, h.send, h.f.N, fb.ra(h.cur), fb.rb(h.cur), q.send.as<float4>(), c->stream));
    log(RESTIR_HALO_EV_PACK, 0, 0, 0, h.send_bytes);
    HIP_TRY(hipEventRecord(q.packed, c->stream));
    log(RESTIR_HALO_EV_RECORD, 0, 0);
    // communication stream: the grouped point-to-point transfer of every plan segment (restir_halo_ops' list)
    HIP_TRY(hipStreamWaitEvent(q.stream, q.packed, 0));
    log(RESTIR_HALO_EV_WAIT, 1, 0);
    if (h.nops) {
        if (rec) {   // nothing moves: a zeroed receive buffer stands in for the transfer
            HIP_TRY(hipMemsetAsync(q.recv.p, 0, h.recv_bytes, q.stream));
        } else {
            RCCL_TRY(rccl_api().group_start());
        }
        log(RESTIR_HALO_EV_GROUP_START, 1);
        const ncclComm_t comm = static_cast<ncclComm_t>(q.comm);
        for (uint32_t i = 0; i < h.nops; i++) {
            const restir_halo_op& o = h.ops[i];
            if (o.kind == RESTIR_HALO_OP_SEND) {
                if (!rec) RCCL_GROUP_TRY(rccl_api().send(static_cast<const char*>(q.send.p) + o.offset, o.bytes, ncclUint8,
                                                         (int)o.peer, comm, q.stream));
                log(RESTIR_HALO_EV_SEND, 1, o.peer, o.offset, o.bytes);
            } else {
                if (!rec) RCCL_GROUP_TRY(rccl_api().recv(static_cast<char*>(q.recv.p) + o.offset, o.bytes, ncclUint8,
                                                         (int)o.peer, comm, q.stream));
                log(RESTIR_HALO_EV_RECV, 1, o.peer, o.offset, o.bytes);
            }
        }
        if (!rec) RCCL_TRY(rccl_api().group_end());
        log(RESTIR_HALO_EV_GROUP_END, 1);
    }
    HIP_TRY(hipEventRecord(q.moved, q.stream));
    log(RESTIR_HALO_EV_RECORD, 1, 1);
    // context stream: the interior overlaps the transfer; unpack + border strips after it
    ST_TRY(halo_interior_locked(c));
    log(RESTIR_HALO_EV_INTERIOR, 0);
    HIP_TRY(hipStreamWaitEvent(c->stream, q.moved, 0));
    log(RESTIR_HALO_EV_WAIT, 0, 1);
    HIP_TRY(launch_halo_unpack(h.view, h.recv, h.f.N, q.recv.as<float4>(), fb.ra(h.cur), fb.rb(h.cur), c->stream));
    log(RESTIR_HALO_EV_UNPACK, 0, 0, 0, h.recv_bytes);
    ST_TRY(halo_border_locked(c));
    log(RESTIR_HALO_EV_BORDER, 0);
    return RESTIR_OK;
}

restir_status restir_halo_record(restir_ctx* c, int on) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    c->halo_record = on != 0;
    c->halo_log.clear();
    return RESTIR_OK;
}

restir_status restir_halo_log(restir_ctx* c, restir_halo_event* out, uint32_t* count) {
    if (!c || !count || (*count && !out)) return fail(RESTIR_ERR_INVALID, "restir_halo_log: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t n = c->halo_log.size();
    if (*count < n) {
        *count = (uint32_t)n;
        return fail(RESTIR_ERR_INVALID, "restir_halo_log: capacity for %zu entries needed", n);
    }
    std::copy(c->halo_log.begin(), c->halo_log.end(), out);
    *count = (uint32_t)n;
    c->halo_log.clear();
    return RESTIR_OK;
}

restir_status restir_halo_end(restir_ctx* c, restir_frame** out_next, float* out_rgb) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    if (out_next) *out_next = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    auto& h = c->halo;
    if (!h.active || h.pass != h.passes)
        return fail(RESTIR_ERR_STATE, "restir_halo_end after %u of %u spatial passes", h.pass, h.passes);
    HIP_TRY(hipSetDevice(c->device));
    const FrameBufs fb{c, h.fb_records, (size_t)h.view.vw * h.view.vh, h.f.N};
    SceneDev sd;
    ST_TRY(scene_for(c, h.f, (size_t)h.view.vw * h.view.vh, sd));
    Ask ask;
    ask.flags = h.tmiss != nullptr;
    LaunchBufs b = fb.bufs(h.camd, 0u, h.cur, h.cur);
    b.flags = h.tmiss;
    TIMED(c, RESTIR_K_FINAL, launch_final(route_final(sd, h.owned, h.f, c->tuning, ask), sd, h.owned, h.f, b, c->stream));
    c->image_produced();
    c->cur = h.cur;
    h.active = false;
    if (out_next) {
        restir_frame* fr = make_frame(c->pool, c->device, c->stream);
        fr->W = h.W; fr->H = h.H; fr->vx0 = h.view.vx0; fr->vy0 = h.view.vy0; fr->vw = h.view.vw; fr->vh = h.view.vh;
        fr->N = h.f.N;
        std::swap(fr->rec, c->rec[h.cur]);
        fr->records = h.fb_records;
        *out_next = fr;
    }
    if (out_rgb) {
        HIP_TRY(hipMemcpyAsync(out_rgb, c->rgb.p, (size_t)h.owned.rw * h.owned.rh * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RESTIR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// timing
restir_status restir_enable_timing(restir_ctx* c, int enable) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    c->timing = enable != 0;
    if (c->timing) {
        // the events the timed launches take, created here rather than by the launches themselves: a
        // hipEventCreate costs microseconds of host time inside whatever region is being timed
        HIP_TRY(hipSetDevice(c->device));
        const size_t want = 512;   // bench.py's default timed region (200 frames x 2) without growing; more on demand
        while (c->free_events.size() + c->pending.size() * 2 < want) {
            hipEvent_t e = nullptr;
            HIP_TRY(timing_event_create(c, &e));
            c->free_events.push_back(e);
        }
    }
    return RESTIR_OK;
}

restir_status restir_timings(restir_ctx* c, double* ms, uint64_t* launches) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(collect_timings(c));
    for (int k = 0; k < RESTIR_K_COUNT; k++) {
        if (ms) ms[k] = c->ms[k];
        if (launches) launches[k] = c->launches[k];
    }
    return RESTIR_OK;
}

restir_status restir_set_tuning(restir_ctx* c, const char* key, int value) {
    if (!c || !key) return fail(RESTIR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    // A knob may change what a frame leaves in the G-buffer planes: the next one traces.  Not these five: the timing
    // knobs choose which launches carry an event pair and how it is created, the two *_after knobs on which reusing frame
    // a cache is built -- none of them reaches a kernel's arguments or launch shape, so no stored byte of the G-buffer,
    // the tile flags, the shadow lists or the visibility bits can differ (DESIGN.md §6 "Knobs that keep the caches")
    static const char* const kKeepsCaches[] = {"timing.mask", "timing.every", "timing.fence", "final.lists_after", "final.vis_after",
                                              "ris.phat_after", "frames.ahead_after", "history.var_fused"};
    bool keeps = false;
    for (const char* k : kKeepsCaches) keeps = keeps || !std::strcmp(key, k);
    if (!keeps) { c->gbuf.valid = false; ahead_drop(c); c->ahead.tuning_gen++; }
    Tuning& t = c->tuning;
    const uint32_t v = (uint32_t)value;
    if (!std::strcmp(key, "primary.lds")) t.primary_lds = v;
    else if (!std::strcmp(key, "ris.lds")) t.ris_lds = v;
    else if (!std::strcmp(key, "spatial.xcd_rows")) t.spatial_xcd_rows = v;
    else if (!std::strcmp(key, "spatial.xcd_cols")) t.spatial_xcd_cols = v;
    else if (!std::strcmp(key, "ris.late")) t.ris_late = v;
    else if (!std::strcmp(key, "miss.tiles")) t.miss_tiles = v;
    else if (!std::strcmp(key, "miss.gbuf")) t.miss_gbuf = v;
    else if (!std::strcmp(key, "final.miss")) t.final_miss = v;
    else if (!std::strcmp(key, "spatial.lean")) t.spatial_lean = v;
    else if (!std::strcmp(key, "spatial.th")) { if (v > 2) return fail(RESTIR_ERR_INVALID, "spatial.th: 0 (auto), 1 or 2"); t.spatial_th = v; }
    else if (!std::strcmp(key, "spatial.handles")) t.spatial_handles = v;
    else if (!std::strcmp(key, "spatial.gather")) t.spatial_gather = v;
    else if (!std::strcmp(key, "spatial.n2h")) t.spatial_n2h = v;
    else if (!std::strcmp(key, "fuse.primary_ris")) t.fuse_primary_ris = v;
    else if (!std::strcmp(key, "fuse.temporal")) t.fuse_temporal = v;
    else if (!std::strcmp(key, "timing.mask")) t.timing_mask = v;
    else if (!std::strcmp(key, "timing.every")) { t.timing_every = v ? v : 1u; for (auto& q : c->timing_seq) q = 0; }
    else if (!std::strcmp(key, "timing.fence")) {
        // the pooled events carry the old flags: drop the free ones (recreated on demand)
        if (t.timing_fence != v) {
            HIP_TRY(hipSetDevice(c->device));
            ST_TRY(collect_timings(c));   // pending pairs return to the pool first
            for (hipEvent_t e : c->free_events) (void)hipEventDestroy(e);
            c->free_events.clear();
        }
        t.timing_fence = v;
    }
    else if (!std::strcmp(key, "ris.compact")) t.ris_compact = v;
    else if (!std::strcmp(key, "bvh.max_leaf")) t.bvh_max_leaf = v;
    else if (!std::strcmp(key, "final.sort")) t.final_sort = v;
    else if (!std::strcmp(key, "final.qbvh")) t.final_qbvh = v;
    else if (!std::strcmp(key, "final.fuse")) t.final_fuse = v;
    else if (!std::strcmp(key, "final.lists")) {
        t.final_lists = v;
        if (!v) { HIP_TRY(hipSetDevice(c->device)); drop_shadow_lists(c); }
    }
    else if (!std::strcmp(key, "final.lists_after")) { if (v < 1) return fail(RESTIR_ERR_INVALID, "final.lists_after: >= 1"); t.final_lists_after = v; }
    else if (!std::strcmp(key, "final.lists_cap")) { if (v < 1 || v > kSlCap) return fail(RESTIR_ERR_INVALID, "final.lists_cap: 1 .. 15"); t.final_lists_cap = v; }
    else if (!std::strcmp(key, "final.vis")) {
        t.final_vis = v;
        if (!v) { HIP_TRY(hipSetDevice(c->device)); drop_shadow_vis(c); }
    }
    else if (!std::strcmp(key, "final.vis_after")) {
        if (v < t.final_lists_after) return fail(RESTIR_ERR_INVALID, "final.vis_after: >= final.lists_after (%u)", t.final_lists_after);
        t.final_vis_after = v;
    }
    else if (!std::strcmp(key, "ris.phat")) {
        t.ris_phat = v;
        if (!v) { HIP_TRY(hipSetDevice(c->device)); drop_phat_table(c); }
    }
    else if (!std::strcmp(key, "ris.phat_after")) { if (v < 1) return fail(RESTIR_ERR_INVALID, "ris.phat_after: >= 1"); t.ris_phat_after = v; }
    else if (!std::strcmp(key, "ris.phat_max_mb")) t.ris_phat_max_mb = v;
    else if (!std::strcmp(key, "frames.ahead")) { if (v > 2) return fail(RESTIR_ERR_INVALID, "frames.ahead: 0 (off), 1 or 2 (RIS enqueued first)"); c->ahead.on = v; }
    else if (!std::strcmp(key, "frames.ahead_after")) { if (v < 1) return fail(RESTIR_ERR_INVALID, "frames.ahead_after: >= 1"); c->ahead.after = v; }
    else if (!std::strcmp(key, "frames.batch")) { if (v < 1 || v > 2) return fail(RESTIR_ERR_INVALID, "frames.batch: 1 or 2 (frames per look-ahead launch)"); c->ahead.batch = v; }
    else if (!std::strcmp(key, "frames.batch_after")) { if (v < 1) return fail(RESTIR_ERR_INVALID, "frames.batch_after: >= 1"); c->ahead.batch_after = v; }
    else if (!std::strcmp(key, "frames.batch_form")) { if (v > 1) return fail(RESTIR_ERR_INVALID, "frames.batch_form: 0 or 1"); c->ahead.batch_form = v; }
    else if (!std::strcmp(key, "frames.ahead_serial")) { if (v > 1) return fail(RESTIR_ERR_INVALID, "frames.ahead_serial: 0 or 1"); c->ahead.serial = v; }
    else if (!std::strcmp(key, "frames.ahead_prio")) { if (v > 1) return fail(RESTIR_ERR_INVALID, "frames.ahead_prio: 0 or 1"); c->ahead.prio = v; }
    else if (!std::strcmp(key, "primary.tl")) t.primary_tl = v;
    else if (!std::strcmp(key, "gbuf.reuse")) t.gbuf_reuse = v;
    else if (!std::strcmp(key, "mis.chunk")) t.mis_chunk = v;   // applies from the next ensure_mis
    else if (!std::strcmp(key, "layout.records")) t.records = v;   // frame-path buffer layout
    else if (!std::strcmp(key, "final.lds")) t.final_lds = v;
    else if (!std::strcmp(key, "history.var_fused")) { if (v > 1) return fail(RESTIR_ERR_INVALID, "history.var_fused: 0 or 1"); c->hist.var_fused = v; }
    else return fail(RESTIR_ERR_INVALID, "unknown tuning key '%s'", key);
    return RESTIR_OK;
}

restir_status restir_reset_timings(restir_ctx* c) {
    if (!c) return fail(RESTIR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(collect_timings(c));
    for (int k = 0; k < RESTIR_K_COUNT; k++) { c->ms[k] = 0.0; c->launches[k] = 0; }
    return RESTIR_OK;
}

}  // extern "C"
