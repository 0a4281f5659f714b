// route.h -- which kernel each frame stage runs, decided once.  One pure host function per frame launcher (launch.h)
// takes the scene, the features, the knobs, the region and what the caller asks of the stage, and returns a Route: the
// kernel, its launch shape, and what the launch reads and writes.  The frame paths (restir.cpp) compute the routes
// first and read their buffer decisions off them; the launchers (kernels.hip) launch what a route names and derive no
// condition again.  Host only: no kernel symbols.
#pragma once

#include <algorithm>

#include "launch_shape.h"
#include "shadow_lists.h"
#include "phat_table.h"
#include "shadow_vis.h"

namespace romis {

// A kernel family; Route's dbg / th / n / lt / staged / unbiased / vis_kernel select the member (RIS: ris_members.h).
enum class Kernel : uint8_t {
    kNone,                 // an empty rect: nothing to launch
    kPrimary,              // k_primary[_lds]
    kRis,                  // k_ris_<member>
    kPrimaryRis,           // k_primary_ris_<member>
    kPrimaryRisTemporal,   // k_primary_ris_<temporal member>
    kSpatial,              // k_spatial_n{N}_{biased | unbiased}: any N, K, R and layout
    kSpatial1u,            // k_spatial1u[_vis][_dbg]: N = 1 unbiased, lean
    kSpatial1Ntl,          // k_spatial1_ntl[_t2][_dbg]: N = 1 biased, lean, over the reservoir planes
    kSpatial1g,            // k_spatial1g_t2[_dbg]: ... over light-grid handles (kind 1)
    kSpatial1hg,           // k_spatial1hg_t2[_dbg]: ... over point-light handles (kind 0), gathered
    kSpatial1hgFinal,      // k_spatial1hg_t2_final: ... with final shading in the same kernel
    kSpatial1h,            // k_spatial1h[_t2][_dbg]: ... over point-light handles, staged in LDS
    kSpatial2Ntl,          // k_spatial2_ntl[_dbg]: N = 2 biased, lean, over the reservoir planes
    kSpatial2hg,           // k_spatial2hg[_t2][_dbg]: ... over 16-byte handle records (kind 2)
    kFinal,                // k_final_n{N}[_lds]
    kFinalSorted,          // k_final_n{1,2}_sorted: one tile per block, the shadow rays binned by target
    kFinalSortedQ,         // k_final_n{1,2}_sorted_q: ... over the 16-byte BVH nodes
    kGbufRis,              // k_gbuf_ris_<member>: kPrimaryRis over a cached G-buffer
    kGbufRisTemporal,      // k_gbuf_ris_<temporal member>
};

// The automatic XCD chunks (spatial.xcd_rows / spatial.xcd_cols left at auto) of a lean spatial kernel
enum class XcdChunks : uint8_t {
    kL2Rows,    // whole tile rows, as many as one XCD's L2 holds
    kOneRow,    // one tile row (the staged and gathered sample-handle kernels on 32 x 16 tiles)
    kThirds,    // 32 x 8 tiles: from 24 tiles a row 2-D chunks of 8 rows x a third of the row, else kL2Rows
    kGrid4x8,   // light-grid handles, 32 x 16 tiles: from 64 tiles a row 2-D chunks of 4 x 8 tiles, else kL2Rows
};

// What a caller wants of a stage.  Every field is a wish: the route says what the chosen kernel does with it.
struct Ask {
    bool dbg = false;         // a debug plane
    int hin = -1;             // spatial: the input's handle kind (spatial_handle_kind; -1: the reservoir planes)
    bool hout = false;        // output handles
    bool hout_dead = false;   // ... which are the output's only reader (Handles::res_dead)
    bool rp_in = false;       // a valid target-pdf cache of the input (own pixel)
    bool rp_nb = false;       // ... that covers every neighbour too
    bool rp_out = false;      // a target-pdf cache of the output
    bool vis = false;         // the own-pixel ray plane: out of a spatial pass, into final shading
    bool flags = false;       // tile flags (MissTiles): out of primary + RIS, into the passes and final shading
    uint32_t flags_m = 0;     // spatial: the M a background pixel holds at the input (MissTiles::m)
    uint32_t gbuf = 0;        // spatial: RIS did not store background tiles' G-buffer either (MissTiles::gbuf)
    uint32_t skip = 0;        // primary + RIS: what of background tiles no reader needs (bit 0 reservoirs, 1 G-buffer)
    bool fin = false;         // spatial: final shading of the pass's rect may run in the same kernel
    bool fin_dead = false;    // ... and then nothing else reads the pass's reservoir planes
    // primary + RIS: the view's G-buffer and tile flags are in memory from an earlier frame (restir_render's GbufView):
    // the k_gbuf_ris family reads them and traces nothing
    bool gbuf_cached = false;
    // spatial: the view's shadow lists (shadow_lists.h) are built: a fused last pass may trace its rays over them
    bool shadow_lists = false;
    // ... and its visibility bits (shadow_vis.h) may be built too: such a pass reads its rays' answers
    bool shadow_vis = false;
    // primary + RIS over a cached G-buffer: the view's p-hat table (phat_table.h) may be built: the N = 1 point-light
    // member then reads its candidates' target pdfs from it
    bool phat = false;
};

struct Route {
    Kernel kernel = Kernel::kNone;
    bool ok = true;            // the stage has a kernel for this scene (the fused primary + RIS forms: else two kernels)
    // the family member
    bool dbg = false, staged = false, unbiased = false, vis_kernel = false;
    uint32_t n = 0;            // the kernel's N (0: the any-N kernel)
    uint32_t th = 1;           // tile height in 8-row units
    int lt = kLtGeneral;       // RIS light-table form
    XcdChunks chunks = XcdChunks::kL2Rows;
    // the launch shape
    uint32_t grid = 0, block = kBlock;
    size_t lds = 0;
    uint32_t map2d = 0, xcd_rows = 0, xcd_cols = 0;   // Region's, as the kernel gets them
    // what the launch reads and writes (false / 0: the kernel gets a null pointer / a zero word there)
    bool res_in = false;       // spatial: reads the input's reservoir planes (else its handles)
    int hin = -1;              // spatial: the handle kind read (-1: none)
    bool hin_m = false;        // ... with the m plane (kind 0)
    bool how = false, hom = false;   // output handles written: the w plane / records, the m plane
    uint32_t res_dead = 0;     // the output's reservoir planes are not stored
    bool rp_in = false, rp_nb = false, rp_out = false;   // target-pdf cache read (own pixel, neighbours), written
    bool vis = false;          // own-pixel ray plane written (spatial) / read (final)
    bool flags = false;        // tile flags written (primary + RIS) / read (spatial, final)
    uint32_t flags_m = 0, gbuf = 0;   // MissTiles::m / ::gbuf as passed
    // spatial: a background tile's reservoirs are substituted through the flags, never read (the N = 1 lean kernels):
    // with no ghost ring RIS need not store them
    bool bg_known = false;
    uint32_t skip = 0;         // primary + RIS: the skip_res word
    uint32_t mode = 0;         // primary + RIS: ris.late | primary.tl << 1
    uint32_t bvh_lds = 0;      // kSpatial: shadow rays over the BVH staged in LDS
    bool final_done = false;   // spatial: final shading ran in this kernel
    bool lists = false;        // ... its rays over the shadow lists (k_spatial1hg_t2_final_lists)
    bool bits = false;         // ... their answers read from the visibility bits (k_spatial1hg_t2_final_vis; `vis` is the ray plane)
    uint32_t miss = 1;         // final: the miss shortcut is allowed (final.miss)
    bool phat = false;         // kGbufRis: the candidates' target pdfs read from the p-hat table (k_gbuf_ris_n1_lds_pt_phat)

    Region region(Region rg) const {
        rg.map2d = map2d; rg.xcd_rows = xcd_rows; rg.xcd_cols = xcd_cols;
        return rg;
    }
};

namespace route_detail {

inline bool empty(const Region& rg) { return rg.rw == 0 || rg.rh == 0; }

// one block per 32 x 8 tile (map2d) or per 256 row-major pixels
inline void items(Route& r, const Region& rg, uint32_t map2d) {
    r.map2d = map2d;
    r.block = kBlock;
    r.grid = map2d ? ((rg.rw + kTileW - 1) / kTileW) * ((rg.rh + kTileH - 1) / kTileH) : (rg.rw * rg.rh + kBlock - 1) / kBlock;
}

// The RIS light-table form (ris_pixel's LT) for this scene and N: the compact tables of the _pt / _grid kernels
// (N = 1, 2) when the scene's lights allow them and ris.compact is on, else the general records.
inline int ris_light_form(const SceneDev& s, const FeaturesDev& f, const Tuning& tu) {
    if (!tu.ris_compact || s.num_lights == 0 || (f.N != 1 && f.N != 2)) return kLtGeneral;
    if (s.light_types == 1u) return kLtPoint;
    // N = 1 (at N = 2 the form spills): ris.compact = 2 keeps the grid table (A/B runs)
    if (s.lights_regular && tu.ris_compact == 1u && f.N == 1) return kLtRegular;
    if (s.lights_grid) return kLtGrid;
    if (s.lights_pgram) return kLtPgram;
    return kLtGeneral;
}

// The light table of route r's form staged in LDS behind `before` bytes, when it fits and ris.lds is on
inline void stage_lights(Route& r, const SceneDev& s, const Tuning& tu, size_t before) {
    const size_t lights = (size_t)lt_stride(r.lt) * s.num_lights * 16;
    r.staged = tu.ris_lds && s.num_lights > 0 && before + lights <= kLdsBudget;
    r.lds = before + (r.staged ? lights : 0);
}

// Blocks for xcd_tile's order over ntx x nty tiles (r.xcd_rows, r.xcd_cols set): every XCD gets as many as the one
// that owns the most chunks.
inline uint32_t xcd_grid(const Route& r, uint32_t ntx, uint32_t nty) {
    if (r.xcd_rows == 0u) return ntx * nty;
    const uint32_t cw = (r.xcd_cols == 0u || r.xcd_cols >= ntx) ? ntx : r.xcd_cols;
    const uint32_t chunks = ((nty + r.xcd_rows - 1u) / r.xcd_rows) * ((ntx + cw - 1u) / cw);
    return 8u * ((chunks + 7u) / 8u) * r.xcd_rows * cw;
}

// The shape of a lean spatial kernel: one block of 256 th threads per 32 x 8 th tile of the rect in xcd_tile's order,
// rounded to the XCD that owns the most tiles.  xcd_rows / xcd_cols: the knobs where they are explicit (an explicit
// spatial.xcd_rows counts rows of the kernel's own tiles), else the kernel's rule.
inline void lean_shape(Route& r, const Region& rg, const Tuning& tu, Kernel k, uint32_t th, XcdChunks rule, size_t lds) {
    r.kernel = k; r.th = th; r.chunks = rule; r.lds = lds;
    r.block = th * kBlock;
    const uint32_t ntx = (rg.rw + kTileW - 1) / kTileW, nty = (rg.rh + th * kTileH - 1) / (th * kTileH);
    const bool auto_rows = tu.spatial_xcd_rows == kXcdRowsAuto, auto_cols = tu.spatial_xcd_cols == kXcdColsAuto;
    r.xcd_rows = tu.spatial_xcd_rows;
    r.xcd_cols = auto_cols ? 0u : tu.spatial_xcd_cols;
    if (auto_rows) {
        // a chunk's records (n_t, p_mat, res_a, res_b: 64 B/px over 8-px tile rows) within one XCD's 4 MB L2:
        // 4 tile rows at 1920 px, 2 at 3840 (kbench: 4K 239 -> 225 us with 2, 1080p best with 4; r2bb); half as many
        // of the twice as tall 32 x 16 tile rows
        r.xcd_rows = std::max(1u, std::min(8u, 8192u / std::max(rg.rw, 1u)) / th);
        // the handle kernels: one 32 x 16 row (k_spatial1h_t2 at C2: 66.1 / 65.7 us against 66.7 / 66.3 with two,
        // 72.9 / 72.5 with four; profiles/r5/probes/r5p23)
        if (rule == XcdChunks::kOneRow) r.xcd_rows = 1u;
    }
    if (rule == XcdChunks::kThirds && auto_cols && r.xcd_rows && ntx >= 24u) {
        // 2-D chunks: 8 tile rows x a third of the tile row (an odd number of chunks per chunk row, so the
        // round-robin XCDs cover every column).  C2: fetch 83 -> 66 B/px at the same time (profiles/r4/r4g,
        // r4h): the window rows a chunk's consecutive tile rows share stay in the XCD's L2.
        if (auto_rows) r.xcd_rows = 8u;
        r.xcd_cols = (ntx + 2u) / 3u;
    }
    if (rule == XcdChunks::kGrid4x8 && auto_rows && auto_cols && ntx >= 64u) {
        // wide frames: 2-D chunks of 4 x 8 tiles (128 x 64 px), so the +-R window rows of vertically adjacent tiles
        // are re-read from one XCD's L2: C4f HBM traffic 1.30 -> 1.01x algorithmic (FETCH 770 -> 541 MB a launch),
        // spatial 404.5 -> 398.2 us (round 6, profiles/r6/probes/s4)
        r.xcd_rows = 4u;
        r.xcd_cols = 8u;
    }
    r.grid = xcd_grid(r, ntx, nty);
}

}  // namespace route_detail

// genPrimaryRayHits: the BVH in LDS when it fits (primary.lds)
inline Route route_primary(const SceneDev& s, const Region& rg, const Tuning& tu) {
    Route r;
    if (route_detail::empty(rg)) return r;
    r.kernel = Kernel::kPrimary;
    route_detail::items(r, rg, 1u);
    r.staged = tu.primary_lds && bvh_lds_bytes(s) <= kLdsBudget;
    r.lds = r.staged ? bvh_lds_bytes(s) : 0;
    return r;
}

// genCanonicalSamples; asks: dbg, rp_out
inline Route route_ris(const SceneDev& s, const Region& rg, const FeaturesDev& f, const Tuning& tu, const Ask& ask) {
    Route r;
    if (route_detail::empty(rg)) return r;
    r.kernel = Kernel::kRis;
    route_detail::items(r, rg, 0u);
    r.n = f.N <= 2u ? f.N : 0u;
    r.lt = route_detail::ris_light_form(s, f, tu);
    route_detail::stage_lights(r, s, tu, 0);
    r.dbg = ask.dbg;
    r.rp_out = ask.rp_out && f.N == 1;
    return r;
}

// Both in one kernel over the same region, the BVH in LDS (!ok: it does not fit); asks: dbg, rp_out, flags with skip,
// hout with hout_dead, gbuf_cached (the same member of the k_gbuf_ris family: the BVH in LDS only for the initial
// visibility rays, so the light table stands alone there otherwise)
inline Route route_primary_ris(const SceneDev& s, const Region& rg, const FeaturesDev& f, const Tuning& tu, const Ask& ask) {
    Route r;
    const size_t bvh = bvh_lds_bytes(s);
    r.ok = bvh <= kLdsBudget;
    r.lt = route_detail::ris_light_form(s, f, tu);
    // sample handles beside the reservoirs: point lights (N = 1: W and M | index; N = 2: 16-byte records) and a
    // regular light grid (N = 1: one float4)
    r.how = ask.hout && (r.lt == kLtPoint || r.lt == kLtRegular);
    r.hom = r.how && r.lt == kLtPoint && f.N == 1;
    r.res_dead = r.how && ask.hout_dead ? 1u : 0u;
    // MissTiles flags: one 32 x 8 tile per block, N <= 2; RIS's skips need the flags
    r.flags = ask.flags && f.N <= 2;
    r.skip = r.flags ? ask.skip : 0u;
    r.n = f.N <= 2u ? f.N : 0u;
    r.dbg = ask.dbg;
    r.rp_out = ask.rp_out && f.N == 1;
    r.mode = (tu.ris_late ? 1u : 0u) | (tu.primary_tl ? 2u : 0u);
    route_detail::stage_lights(r, s, tu, bvh);
    if (!r.ok || route_detail::empty(rg)) return r;
    r.kernel = Kernel::kPrimaryRis;
    route_detail::items(r, rg, 1u);
    if (ask.gbuf_cached) {
        // the same family member (r.staged as the fused kernel decided it), its LDS without the BVH where no ray needs it
        r.kernel = Kernel::kGbufRis;
        r.lds = (f.initial_vis ? bvh : 0) + (r.staged ? (size_t)lt_stride(r.lt) * s.num_lights * 16 : 0);
        // ... with its candidates' target pdfs from the view's p-hat table (ris.phat): the staged N = 1 point-light
        // member writing both handle planes, no initial visibility rays, a shape the table's kernel serves (pt_fast)
        r.phat = ask.phat && tu.ris_phat && r.n == 1u && r.lt == kLtPoint && r.staged && r.hom && !f.initial_vis && !ask.dbg &&
                 pt_fast(s.num_lights, f.M);
        if (r.phat) r.lds = pt_lds_bytes(s.num_lights);
    }
    return r;
}

// ... with temporal reuse in the same kernel (fuse.temporal): N = 1 / 2, point lights, the light table in LDS; asks:
// dbg, rp_out, hout with hout_dead
inline Route route_primary_ris_temporal(const SceneDev& s, const Region& rg, const FeaturesDev& f, const Tuning& tu,
                                        const Ask& ask) {
    Route r = route_primary_ris(s, rg, f, tu, ask);
    r.ok = r.ok && tu.fuse_temporal && (f.N == 1 || f.N == 2) && r.lt == kLtPoint && r.staged;
    r.flags = false;   // (no background tiles: the output is not the RIS result)
    r.skip = 0u;
    r.hom = r.how;     // both planes at N = 1 and 2
    r.phat = r.phat && r.ok;   // (k_gbuf_ris_n1_lds_pt_phat_temporal)
    if (r.kernel != Kernel::kNone)
        r.kernel = !r.ok ? Kernel::kNone : ask.gbuf_cached ? Kernel::kGbufRisTemporal : Kernel::kPrimaryRisTemporal;
    return r;
}

// Final shading; asks: vis, flags
inline Route route_final(const SceneDev& s, const Region& rg, const FeaturesDev& f, const Tuning& tu, const Ask& ask) {
    Route r;
    r.miss = tu.final_miss ? 1u : 0u;   // final.miss = 0: no miss shortcut (A/B runs)
    if (route_detail::empty(rg)) return r;
    route_detail::items(r, rg, 1u);
    r.n = f.N <= 2u ? f.N : 0u;
    const size_t bvh = bvh_lds_bytes(s);
    r.staged = tu.final_lds && bvh <= kLdsBudget;
    if (tu.final_sort && r.staged && r.n) {   // one tile per block
        // 16-byte nodes (occluded_q)
        const bool q = (tu.final_qbvh == 1u || (tu.final_qbvh == 2u && f.N == 2)) && s.nodes_q_ok;
        r.kernel = q ? Kernel::kFinalSortedQ : Kernel::kFinalSorted;
        r.lds = q ? ((size_t)s.num_nodes + (size_t)3 * s.num_tris) * 16 : bvh;
        r.vis = ask.vis && f.N == 1;
        r.flags = ask.flags;   // background tiles are written from the flags without being read
    } else {
        r.kernel = Kernel::kFinal;
        r.lds = r.staged ? bvh : 0;
    }
    return r;
}

// One spatial pass over rg's rect; asks: all but skip
inline Route route_spatial(const SceneDev& s, const Region& rg, const FeaturesDev& f, const Tuning& tu, const Ask& ask) {
    using namespace route_detail;
    Route r;
    if (empty(rg)) return r;
    r.n = f.N <= 2u ? f.N : 0u;
    r.dbg = ask.dbg;
    r.unbiased = f.unbiased != 0;
    r.map2d = 2u;   // 32 x 8 tiles of 8 x 8 waves (the lean kernels' XCD tile order, xcd_tile)
    const size_t bvh = bvh_lds_bytes(s);
    const bool bvh_fits = bvh <= kLdsBudget;
    // the lean kernels: SoA planes whose byte offsets fit 32 bits (N = 2: those of both sub-reservoir planes)
    const bool soa = tu.spatial_lean && f.K <= kLeanK && rg.ps == 1u;
    const bool lean1 = soa && f.N == 1 && (size_t)rg.vw * rg.vh * 16u <= 0xFFFFFFFFull;
    const bool lean2 = soa && f.N == 2 && (size_t)rg.js * 16u + (size_t)rg.vw * rg.vh * 16u <= 0xFFFFFFFFull;
    const bool window = !f.unbiased && f.R <= kLdsSpatialR;   // the biased ones stage the +-R window
    const size_t pt_table = (size_t)(2u * s.num_lights + 2u) * 16u;   // point lights: positions, colours, the zero sample
    const bool lean = (lean1 && (window || (f.unbiased && (!f.spatial_vis || bvh_fits)))) || (lean2 && window);
    if (!lean) {
        r.kernel = Kernel::kSpatial;
        items(r, rg, 2u);
        r.res_in = true;
        r.bvh_lds = (f.unbiased && f.spatial_vis && bvh_fits) ? 1u : 0u;
        r.lds = r.bvh_lds ? bvh : 0;
        return r;
    }
    // every lean kernel takes the tile flags; the N = 1 ones substitute a background tile's known reservoirs
    r.flags = ask.flags;
    r.flags_m = ask.flags ? ask.flags_m : 0u;
    r.gbuf = ask.flags ? ask.gbuf : 0u;
    r.bg_known = r.flags && f.N == 1;
    if (f.unbiased) {
        // combineUnbiased, N = 1: one block per tile in the XCD order of the biased pass (xcd_tile)
        lean_shape(r, rg, tu, Kernel::kSpatial1u, 1u, XcdChunks::kL2Rows, f.spatial_vis ? bvh : 0);
        r.vis_kernel = f.spatial_vis != 0;
        r.res_in = true;
        r.rp_in = ask.rp_in; r.rp_nb = ask.rp_in && ask.rp_nb; r.rp_out = ask.rp_out;
        r.vis = r.vis_kernel && ask.vis;   // the own-pixel shadow ray, for final shading (N = 1)
        return r;
    }
    r.res_dead = ask.hout && ask.hout_dead ? 1u : 0u;
    if (f.N == 2) {
        // N = 2 biased: no pdf cache
        if (ask.hin == 2) {
            // handle records (k_spatial2hg[_t2]): 32 x 8 TH tiles, TH = spatial.th (auto 1)
            const uint32_t th = tu.spatial_th == 2u ? 2u : 1u;
            lean_shape(r, rg, tu, Kernel::kSpatial2hg, th, XcdChunks::kL2Rows, (size_t)apron_max(th) * 16u + pt_table);
            r.hin = 2;
            r.how = ask.hout;
        } else {
            lean_shape(r, rg, tu, Kernel::kSpatial2Ntl, 1u, XcdChunks::kL2Rows, kApronMax * 16u);
            r.res_in = true;
            r.res_dead = 0u;
        }
        return r;
    }
    // N = 1 biased: one block per tile
    r.rp_in = ask.rp_in; r.rp_out = ask.rp_out;
    if (ask.hin == 1 && tu.spatial_th != 1u) {
        // light-grid handles: k_spatial1_ntl_t2's tiles, the colours behind the window
        lean_shape(r, rg, tu, Kernel::kSpatial1g, 2u, XcdChunks::kGrid4x8, apron_max(2) * 16u + (size_t)s.num_lights * 16u);
        r.hin = 1;
        r.how = ask.hout;
    } else if (ask.hin == 0 && tu.spatial_gather && tu.spatial_th != 1u) {
        // sample handles gathered instead of staged (spatial.gather; round 6): 32 x 16 tiles, the automatic XCD
        // chunk one tile row as for k_spatial1h_t2
        const size_t lds = (size_t)apron_max(2) * 16u + pt_table;
        r.hin = 0; r.hin_m = true;
        r.how = r.hom = ask.hout;
        // Final shading in the same kernel (final.fuse) when launch_final would run k_final_n1_sorted over the same
        // rect: no debug plane, no pdf cache out, and the ray phase's LDS -- the BVH, the rays, the histogram, in
        // the bytes of the window and the light table -- within the budget.  The caller offers it only when
        // launch_final would get no own-pixel ray plane.
        const size_t lds_fin = bvh + (size_t)kFinLdsF4 * 16u;
        const Route fin = route_final(s, rg, f, tu, Ask{});
        if (ask.fin && tu.final_fuse && !ask.dbg && !ask.rp_out && fin.kernel == Kernel::kFinalSorted &&
            std::max(lds, lds_fin) <= kLdsBudget) {
            lean_shape(r, rg, tu, Kernel::kSpatial1hgFinal, 2u, XcdChunks::kOneRow, std::max(lds, lds_fin));
            r.final_done = true;
            r.miss = fin.miss;
            // the rays over the view's shadow lists (final.lists) where the caller holds them: one-byte triangle indices
            r.lists = ask.shadow_lists && tu.final_lists && s.num_tris <= kSlMaxTris;
            // ... answered from the view's visibility bits (final.vis): at most kSvMaxWords words per pixel
            r.bits = r.lists && ask.shadow_vis && tu.final_vis && s.num_lights > 0u && sv_words(s.num_lights) <= kSvMaxWords;
            // nothing else reads the pass's reservoir planes (no returned grid): the fused kernel does not store them
            if (ask.fin_dead) r.res_dead = 1u;
        } else {
            lean_shape(r, rg, tu, Kernel::kSpatial1hg, 2u, XcdChunks::kOneRow, lds);
        }
    } else if (ask.hin == 0) {
        // sample handles staged in LDS: 32 x 8 TH tiles, TH = spatial.th (auto: 2 -- C2 66.9 us against 76.2 for
        // 32 x 8, 70.6 / 68.4 for 32 x 24 / 32 x 32, kbench, profiles/r5); 32 x 8 tiles take k_spatial1_ntl's chunks
        const uint32_t th = tu.spatial_th ? tu.spatial_th : 2u;
        lean_shape(r, rg, tu, Kernel::kSpatial1h, th, th > 1u ? XcdChunks::kOneRow : XcdChunks::kThirds,
                   (size_t)h_lds_f4(th) * 16u + pt_table);
        r.hin = 0; r.hin_m = true;
        r.how = r.hom = ask.hout;
    } else {
        // 32x16 tiles (k_spatial1_ntl_t2) where the auto XCD chunk is at most 2 tile rows (wide images): C4 222 ->
        // 203 us, C2 76.8 -> 79.0 (cfg_kbench, profiles/r3/r3k); spatial.th = 1 / 2 forces either
        const uint32_t th = tu.spatial_th ? tu.spatial_th : (8192u / std::max(rg.rw, 1u) <= 2u ? 2u : 1u);
        if (th >= 2u) lean_shape(r, rg, tu, Kernel::kSpatial1Ntl, 2u, XcdChunks::kL2Rows, apron_max(2) * 16u);
        else lean_shape(r, rg, tu, Kernel::kSpatial1Ntl, 1u, XcdChunks::kThirds, kApronMax * 16u);
        r.res_in = true;
        r.res_dead = 0u;
    }
    return r;
}

// The handle kind restir_render's biased passes read instead of the reservoir planes: 0 point-light handles (8 B per
// pixel, k_spatial1h / k_spatial1hg), 1 light-grid handles (16 B, k_spatial1g), 2 N = 2 point-light records (16 B,
// k_spatial2hg; spatial.n2h), -1 none.  The fused primary + RIS kernel must write that kind over `view`, the passes
// must have a kernel that reads it, and every M `passes` passes can produce must fit the handle's M field.
// m0: the largest M entering the passes when it exceeds RIS's f.M (temporal reuse); 0 = f.M
inline int spatial_handle_kind(const SceneDev& s, const Region& view, const FeaturesDev& f, const Tuning& tu,
                               uint32_t passes, uint64_t m0 = 0) {
    if (!tu.spatial_handles || passes == 0) return -1;
    Ask out;
    out.hout = true;
    const Route ris = route_primary_ris(s, view, f, tu, out);
    if (!ris.ok || !ris.how) return -1;
    const int hk = ris.hom ? 0 : f.N == 2 ? 2 : 1;
    // the light index field: 8 bits with index L the zero sample (point lights); <= 16 KB of colours in LDS (a grid)
    if (s.num_lights > (hk == 1 ? 1024u : 254u) || (hk == 2 && !tu.spatial_n2h)) return -1;
    Ask in;
    in.hin = hk;
    if (route_spatial(s, view, f, tu, in).hin != hk) return -1;
    // every M: RIS M (or m0: after temporal reuse), then each biased pass sums at most K + 1 inputs
    const uint32_t mmax = hk == 1 ? kHandleMG : kHandleM;
    uint64_t m = m0 ? m0 : f.M;
    for (uint32_t p = 0; p < passes && m <= mmax; p++) m *= (uint64_t)(f.K + 1u);
    return m <= mmax ? hk : -1;
}

}  // namespace romis
