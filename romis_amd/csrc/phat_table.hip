// phat_table.hip -- the p-hat table of a still view (phat_table.h has the layout, DESIGN.md §6 "P-hat table" the
// reasoning): k_phat_table builds it, k_gbuf_ris_n1_lds_pt_phat is k_gbuf_ris_n1_lds_pt with its candidates' target pdfs
// read from it, k_debug_phat unpacks one light's plane.  Compiled with -ffp-contract=off like every other kernel:
// target_pdf() here is the frame kernel's.  A translation unit of its own: no other kernel's code changes with it.
#include "kernels_common.h"
#include "launch.h"
#include "launch_events.h"
#include "phat_table.h"

namespace romis {
namespace {

// The tile's flag (gbuf_ris_body's rule): its word by a scalar load; no flags: every tile is live
__device__ __forceinline__ bool pt_tile_live(const uint8_t* tmiss, uint32_t tile) {
    if (!tmiss) return true;
    const auto* w = (const __attribute__((address_space(4))) uint32_t*)(tmiss + (tile & ~3u));
    return ((*w >> (8u * (tile & 3u))) & 0xFFu) != 0u;
}
// ris_pixel's c_end != 0: the pixel runs the candidate loop (pm: its p_mat record)
__device__ __forceinline__ bool pt_runs_loop(const SceneDev& s, float4 pm) {
    const uint32_t m = min(__float_as_uint(pm.w), s.num_materials - 1u);
    return !(m == s.num_materials - 1u && s.lights_finite && !__builtin_isnan(pm.x + pm.y + pm.z));
}

// One block of 256 threads per 32 x 8 tile of the view, thread t at the pixel the frame kernel's thread t holds.  The
// block loops over the L lights in chunks of 16: light i is the same for all lanes (no divergence on the light), each
// lane evaluates target_pdf(px, light_c2[i], light_c2[L + i], tb) -- ris_pixel's call for candidate light i -- into its
// wave's LDS tile, which the wave then stores as 64-byte row segments (four lanes per row).  A lane whose pixel never
// runs the candidate loop evaluates nothing and stores zeros; a background tile's block returns at once.  Every index
// is in range: the pixel by work_pixel's test, the lights by the loop's bound, the rows by pt_size.
__global__ __launch_bounds__(kPtTilePx) void k_phat_table(PhatTableDev d) {
    const SceneDev& s = d.s;
    const Region& rg = d.rg;
    const uint32_t tile = blockIdx.x;
    if (tile >= work_items(rg)) return;
    if (!pt_tile_live(d.tmiss, tile)) return;   // block-uniform
    const GlTabs tb = gl_stage_tables();
    __shared__ float s_out[4][64][20];   // [wave][row][16 lights + pad]: 16-byte aligned rows, 20 KB
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t L = s.num_lights, rf = pt_row_floats(L);
    uint32_t x, y;
    size_t p;
    const bool live = work_pixel(rg, tile, x, y, p);
    bool held = false;
    Px px{};
    if (live) {
        const float4 pm = d.p_mat[p];
        held = pt_runs_loop(s, pm);
        if (held) px = make_px(s, d.n_t[gidx(rg, p)], pm, mk(d.origin[0], d.origin[1], d.origin[2]), p);
    }
    float* const rows = d.tab + pt_index(pt_row_of_thread(tile, wave << 6), rf, 0u);
    for (uint32_t i0 = 0; i0 < rf; i0 += 16u) {
#pragma unroll 1
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t i = i0 + k;   // wave-uniform
            float v = 0.0f;
            if (held && i < L) v = target_pdf(s, d.f, px, xyz(s.light_c2[i]), xyz(s.light_c2[L + i]), tb);
            s_out[wave][lane][k] = v;
        }
        __syncthreads();
        // 64 rows x 64 bytes: lane l stores float4 (l & 3) of rows (l >> 2) + 16 j
        const uint32_t c4 = (lane & 3u) * 4u;
        if (i0 + c4 < rf) {
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t r = (lane >> 2) + 16u * j;
                *reinterpret_cast<float4*>(rows + (size_t)r * rf + i0 + c4) = *reinterpret_cast<const float4*>(&s_out[wave][r][c4]);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_debug_phat(PhatTableDev d, uint32_t light, float* out) {
    const Region& rg = d.rg;
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x & 31u), y = blockIdx.y * kTileH + (threadIdx.x >> 5);
    if (x >= rg.rw || y >= rg.rh) return;
    const uint32_t ntx = (rg.rw + kTileW - 1u) / kTileW;
    const size_t p = (size_t)(rg.ry0 + y - rg.vy0) * rg.vw + (rg.rx0 + x - rg.vx0);
    float r = -1.0f;
    if (pt_tile_live(d.tmiss, (y / kTileH) * ntx + x / kTileW) && pt_runs_loop(d.s, d.p_mat[p]))
        r = d.tab[pt_index(pt_row(rg.rw, x, y), pt_row_floats(d.s.num_lights), light)];
    out[(size_t)y * rg.rw + x] = r;
}

}  // namespace
}  // namespace romis

// k_gbuf_ris_n1_lds_pt (kernels.hip gbuf_ris_body + ris_pixel<1, kLtPoint>) with candidate c's target pdf read from the
// table: candidate c of pixel p draws light i = uniform_index(draw(ps, 4c), L), and its p-hat is row(p)[i].  One block
// per 32 x 8 tile, thread t at the frame kernel's pixel.  Each wave takes its 64 pixels in four steps of 16: it copies the
// step's 16 rows (one contiguous span) into its own LDS with coalesced 16-byte loads, then four lanes per pixel share the
// pixel's M candidates, a contiguous chunk each:
//   A  every lane: for its candidates, the draw, the row entry and the weight w_c (ris_pixel's `weight`);
//   B  wsum_c = wsum_(c-1) + w_c from sub_init's FLT_MIN, c = 0 .. M - 1 in order -- the reference's left-to-right float
//      sum, the only serial part;
//   C  every lane: accept_u(rand01(draw(ps, 4c + 3)), w_c, wsum_c) for its candidates; the accepted candidate is the
//      highest c that accepted (ris_pixel's `best` after its loop);
//   D  one lane per pixel: the accepted candidate's row entry, its p-hat.
// The tail is ris_pixel's, per pixel: the same values to the same planes.  A pixel with no accepted candidate evaluates
// target_pdf of the initial sample as ris_pixel does (powf's tables staged for it).
//
// The kernel serves pt_fast shapes (M <= 32, L <= 128; the route keeps the table-free kernel for the rest).  A lane's
// weights and sums stay in registers: B runs as G rounds in which every lane adds its chunk onto the total its left
// neighbour held after the round before (one DPP move) -- after round r the lanes 0 .. r of a pixel hold the reference's
// prefixes, so 32 adds a step in all; the accepted candidate is a maximum over the pixel's G lanes (DPP moves); the next
// step's rows are in flight in registers while this step computes; and a wave touches only its own LDS, so after the
// prologue it never waits for the block.  G = kPtLanesPerPx = 4 ships; ROMIS_PT_G builds the forms with 2 and 8 lanes
// per pixel that profiles/phat_table/forms.json compares (the table's layout does not depend on G).
#ifndef ROMIS_PT_G
#define ROMIS_PT_G 4
#endif
#ifndef ROMIS_PT_WAVE_SYNC
#define ROMIS_PT_WAVE_SYNC 1   // 0: block barriers (A/B)
#endif
#ifndef ROMIS_PT_PREFETCH
#define ROMIS_PT_PREFETCH 1    // 0: a step's rows are loaded when it starts: one buffer, nothing in flight (A/B)
#endif
#ifndef ROMIS_PT_LDS2
#define ROMIS_PT_LDS2 0        // 1: two row buffers per wave in LDS, a step's rows stored while the step before computes (A/B)
#endif
namespace romis {
namespace {

constexpr uint32_t kG = ROMIS_PT_G;            // lanes per pixel
constexpr uint32_t kStepPx = 64u / kG;         // pixels a wave takes per step
constexpr uint32_t kSteps = kG;                // steps over a wave's 64 pixels
constexpr uint32_t kChunk = 32u / kG;          // pt_fast: candidates per lane at most
constexpr uint32_t kRowF4 = kStepPx * 128u / 256u;   // pt_fast: float4s of a step's rows per lane at most
static_assert(kG == 2u || kG == 4u || kG == 8u, "2, 4 or 8 lanes per pixel");
static_assert(ROMIS_PT_G != 4 || (kStepPx == kPtStepPx && kG == kPtLanesPerPx), "the shipped form is phat_table.h's");

// Orders a wave's LDS writes before its later reads by other lanes: the LDS serves a wave's instructions in order, so
// only the compiler must keep them in order
__device__ __forceinline__ void pt_wave_sync() {
#if ROMIS_PT_WAVE_SYNC
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
    __syncthreads();
#endif
}
// lane n reads lane n - 1's value (the first lane of a row of 16 keeps its own)
__device__ __forceinline__ float pt_from_left(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x111, 0xF, 0xF, false));
}
// the maximum over a pixel's kG lanes (aligned groups of 2, 4 or 8 lanes)
__device__ __forceinline__ uint32_t pt_group_max(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1, 0, 3, 2]
    if (kG >= 4u) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2, 3, 0, 1]
    if (kG >= 8u) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    return v;
}

template <bool TEMP>
__device__ __forceinline__ void pt_ris_body(const SceneDev& s, const Region& rg, const FeaturesDev& f, uint32_t key, v3 origin,
                                            const float4* __restrict__ n_t, const float4* __restrict__ p_mat,
                                            float4* __restrict__ ra, float4* __restrict__ rb, float2* __restrict__ rdbg,
                                            float* __restrict__ rp, const uint8_t* __restrict__ tmiss, uint32_t skip_res,
                                            float* __restrict__ hw, uint32_t* __restrict__ hm, uint32_t res_dead,
                                            const float* __restrict__ tab, TemporalIn tin = TemporalIn{nullptr, nullptr, 0u}) {
    const uint32_t tile = blockIdx.x;
    if (tile >= work_items(rg)) return;   // block-uniform
    const bool any = pt_tile_live(tmiss, tile);
    if (!any && (skip_res & 1u)) return;
    __shared__ uint32_t s_best[kPtTilePx];   // accepted candidate + 1 (0: none)
    __shared__ float s_wsum[kPtTilePx], s_pd[kPtTilePx];
    __shared__ uint8_t s_loop[kPtTilePx];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t L = s.num_lights, M = f.M, rf = pt_row_floats(L);
    uint32_t x, y;
    size_t p;
    const bool live = work_pixel(rg, tile, x, y, p);
    float4 nt = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pm = nt;
    if (live) {
        nt = n_t[gidx(rg, p)];
        pm = p_mat[p];
    }
    const bool loop = live && any && pt_runs_loop(s, pm);
    s_best[t] = 0u;
    s_wsum[t] = ROMIS_FLT_MIN;
    s_pd[t] = 0.0f;
    s_loop[t] = loop ? 1u : 0u;
    const GlTabs tb = gl_stage_tables<false>();
    __syncthreads();
    if (any) {
        const uint32_t q = lane / kG, j = lane % kG;
        const uint32_t chunk = (M + kG - 1u) / kG;
        const uint32_t c0 = min(j * chunk, M), c1 = min(c0 + chunk, M);
        const float invL = 1.0f / (float)L;
        auto weight = [&](float pd) { return s.light_scale != 0.0f ? pd * s.light_scale : pd / invL; };   // ris_pixel's
        const uint32_t ntx = (rg.rw + kTileW - 1u) / kTileW;
        typedef float f4v __attribute__((ext_vector_type(4)));
        const uint32_t n4 = kStepPx * rf / 4u;
        // the wave's LDS: the step's rows
        float* const l_base = reinterpret_cast<float*>(g_lds) + (size_t)wave * kStepPx * rf * (ROMIS_PT_LDS2 ? 2u : 1u);
        f4v v[kRowF4];
        auto fetch = [&](uint32_t step) {
            const f4v* src = reinterpret_cast<const f4v*>(tab + pt_index(pt_row_of_thread(tile, (wave << 6) + step * kStepPx), rf, 0u));
#pragma unroll
            for (uint32_t u = 0; u < kRowF4; u++)
                if (64u * u + lane < n4) v[u] = __builtin_nontemporal_load(src + 64u * u + lane);
        };
        if (ROMIS_PT_PREFETCH) fetch(0u);
#pragma unroll 1
        for (uint32_t step = 0; step < kSteps; step++) {
            if (!ROMIS_PT_PREFETCH) fetch(step);
            float* const l_rows = l_base + (ROMIS_PT_LDS2 ? (step & 1u) * kStepPx * rf : 0u);
            f4v* const dst = reinterpret_cast<f4v*>(l_rows);
#pragma unroll
            for (uint32_t u = 0; u < kRowF4; u++)
                if (64u * u + lane < n4) dst[64u * u + lane] = v[u];
            if (ROMIS_PT_PREFETCH && step + 1u < kSteps) fetch(step + 1u);
            // the step's pixel of this lane: thread tq of the block (tile_pixel_of's mapping, map2d = 1) and its RNG state
            const uint32_t tq = (wave << 6) + step * kStepPx + q;
            const uint32_t xq = rg.rx0 + (tile % ntx) * kTileW + tq % kTileW, yq = rg.ry0 + (tile / ntx) * kTileH + tq / kTileW;
            const uint32_t psq = pix_state(key, yq * rg.W + xq);
            const bool lq = s_loop[tq] != 0u;
            pt_wave_sync();
            float w[kChunk], ws[kChunk];
#pragma unroll
            for (uint32_t k = 0; k < kChunk; k++)   // (an index past the chunk still reads inside the row)
                w[k] = weight(l_rows[q * rf + uniform_index(draw(psq, 4u * (c0 + k)), L)]);
            float run = ROMIS_FLT_MIN;
#pragma unroll
            for (uint32_t r = 0; r < kG; r++) {
                const float left = pt_from_left(run);
                run = j == 0u ? ROMIS_FLT_MIN : left;   // sub_init's wsum, or the total of the candidates before this chunk
#pragma unroll
                for (uint32_t k = 0; k < kChunk; k++) {
                    run = c0 + k < c1 ? run + w[k] : run;
                    ws[k] = run;
                }
            }
            uint32_t best = 0u;
#pragma unroll
            for (uint32_t k = 0; k < kChunk; k++) {
                const bool acc = accept_u(rand01(draw(psq, 4u * (c0 + k) + 3u)), w[k], ws[k]);
                if (acc && c0 + k < c1) best = c0 + k + 1u;
            }
            best = pt_group_max(lq ? best : 0u);
            if (lq && j == kG - 1u) {   // the pixel's last lane holds the whole sum
                s_wsum[tq] = run;
                s_best[tq] = best;
                if (best) s_pd[tq] = l_rows[q * rf + uniform_index(draw(psq, 4u * (best - 1u)), L)];
            }
            if (!ROMIS_PT_LDS2) pt_wave_sync();   // the rows are overwritten by the next step
        }
    }
    if (!live) return;
    // ris_pixel's tail (NT = 1, kLtPoint, no temporal reuse, no initial visibility rays)
    Sub r;
    sub_init(r);
    r.M = M;
    r.wsum = s_wsum[t];
    const uint32_t b = s_best[t];
    uint32_t hidx = L;
    float pj;
    if (b) {
        hidx = uniform_index(draw(pix_state(key, y * rg.W + x), 4u * (b - 1u)), L);
        r.pos = xyz(s.light_c2[hidx]);
        r.col = xyz(s.light_c2[L + hidx]);
        pj = s_pd[t];
        r.chosen = s.light_scale != 0.0f ? pj * s.light_scale : pj / (1.0f / (float)L);
    } else {
        pj = target_pdf(s, f, make_px(s, nt, pm, origin, p), r.pos, r.col, tb);
    }
    r.W = contribution_weight(pj, r.M, r.wsum);
    if (TEMP) {
        // ris_pixel's temporalReuse (NT = 1, kLtPoint), step for step: the predecessor from its frame handle or its
        // reservoir planes, its M clamped to clampM * M_current + 1, then the current reservoir (its target pdf pj) and
        // the predecessor combined biased (Combiner<1>::consume_pd, consume, finish_biased)
        const Px px = make_px(s, nt, pm, origin, p);
        Sub prev;
        uint32_t phidx = L;
        if (tin.hw) {
            const uint32_t hv = tin.hm[p];
            sub_init(prev);
            phidx = hv >> 24;
            prev.W = tin.hw[p];
            prev.M = hv & 0x00FFFFFFu;
            if (phidx < L) { prev.pos = xyz(s.light_c2[phidx]); prev.col = xyz(s.light_c2[L + phidx]); }
        } else {
            sub_load(prev, tin.pa, tin.pb, ridx(rg, 0u, p));
        }
        const unsigned long long C = (unsigned long long)f.clamp_m * (unsigned long long)r.M + 1ull;
        if ((unsigned long long)prev.M > C && prev.M != 0u) prev.M = (uint32_t)C;
        const uint32_t pst = pix_state(tin.key, y * rg.W + x);
        Sub out;
        sub_init(out);
        sub_take(out, r.pos, r.col, (pj * r.W) * (float)r.M, rand01(draw(pst, 0u)), pj);
        const float pp = target_pdf(s, f, px, prev.pos, prev.col);
        sub_take(out, prev.pos, prev.col, (pp * prev.W) * (float)prev.M, rand01(draw(pst, 1u)), pp);
        out.M = r.M + prev.M;
        const float po = out.has_pd ? out.pd : target_pdf(s, f, px, out.pos, out.col);
        out.W = contribution_weight(po, out.M, out.wsum);
        // the held sample's light index: the predecessor's when the output holds its sample, bit for bit
        if (hw) {
            const bool same = __float_as_uint(out.pos.x) == __float_as_uint(prev.pos.x) &&
                              __float_as_uint(out.pos.y) == __float_as_uint(prev.pos.y) &&
                              __float_as_uint(out.pos.z) == __float_as_uint(prev.pos.z) &&
                              __float_as_uint(out.col.x) == __float_as_uint(prev.col.x) &&
                              __float_as_uint(out.col.y) == __float_as_uint(prev.col.y) &&
                              __float_as_uint(out.col.z) == __float_as_uint(prev.col.z);
            if (same) hidx = phidx;
        }
        r = out;
        pj = po;
    }
    if (rp) rp[p] = pj;
    if (!(hw && res_dead) || rdbg) sub_store(r, ra, rb, rdbg, ridx(rg, 0u, p), p);
    if (hw) { hw[p] = r.W; hm[p] = r.M | (hidx << 24); }
}


// pt_ris_body<false> for two RNG keys in one launch (DESIGN.md §6 "RIS batch"): the rows of a step go to LDS once; phases
// A-D and the tail run once per key, key 1's (key1, rp1, hw1, hm1) exactly as a launch of its own would -- every draw, add
// and accept is that launch's.  The keys share the row bytes, s_loop and the pixel's nt / pm, nothing else.  It serves the
// look-ahead's route alone: the reservoir planes are dead, there is no debug plane, and every output plane is there
// (launch_gbuf_ris_phat_batch refuses anything else).  A copy of the body, not a parameter of it: with the parameter the
// one-key kernels' registers were allocated differently, and their instruction streams are held fixed
// (scripts/device_code_diff.py).  A change to phases A-D or the tail of either body goes into both.
__device__ __forceinline__ void pt_ris_batch_body(const SceneDev& s, const Region& rg, const FeaturesDev& f, uint32_t key, v3 origin,
                                                  const float4* __restrict__ n_t, const float4* __restrict__ p_mat,
                                                  float* __restrict__ rp, const uint8_t* __restrict__ tmiss, uint32_t skip_res,
                                                  float* __restrict__ hw, uint32_t* __restrict__ hm,
                                                  const float* __restrict__ tab, uint32_t key1, float* __restrict__ rp1,
                                                  float* __restrict__ hw1, uint32_t* __restrict__ hm1) {
    constexpr uint32_t NB = 2u;   // the keys
    const uint32_t tile = blockIdx.x;
    if (tile >= work_items(rg)) return;   // block-uniform
    const bool any = pt_tile_live(tmiss, tile);
    if (!any && (skip_res & 1u)) return;
    // accepted candidate + 1 (0: none) in a byte (M <= 32): four blocks a CU keep their LDS
    typedef uint8_t best_t;
    __shared__ best_t s_best[NB][kPtTilePx];
    __shared__ float s_wsum[NB][kPtTilePx], s_pd[NB][kPtTilePx];
    __shared__ uint8_t s_loop[kPtTilePx];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t L = s.num_lights, M = f.M, rf = pt_row_floats(L);
    uint32_t x, y;
    size_t p;
    const bool live = work_pixel(rg, tile, x, y, p);
    float4 nt = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pm = nt;
    if (live) {
        nt = n_t[gidx(rg, p)];
        pm = p_mat[p];
    }
    const bool loop = live && any && pt_runs_loop(s, pm);
#pragma unroll
    for (uint32_t kb = 0; kb < NB; kb++) {
        s_best[kb][t] = 0u;
        s_wsum[kb][t] = ROMIS_FLT_MIN;
        s_pd[kb][t] = 0.0f;
    }
    s_loop[t] = loop ? 1u : 0u;
    const GlTabs tb = gl_stage_tables<false>();
    __syncthreads();
    if (any) {
        const uint32_t q = lane / kG, j = lane % kG;
        const uint32_t chunk = (M + kG - 1u) / kG;
        const uint32_t c0 = min(j * chunk, M), c1 = min(c0 + chunk, M);
        const float invL = 1.0f / (float)L;
        auto weight = [&](float pd) { return s.light_scale != 0.0f ? pd * s.light_scale : pd / invL; };   // ris_pixel's
        const uint32_t ntx = (rg.rw + kTileW - 1u) / kTileW;
        typedef float f4v __attribute__((ext_vector_type(4)));
        const uint32_t n4 = kStepPx * rf / 4u;
        // the wave's LDS: the step's rows
        float* const l_base = reinterpret_cast<float*>(g_lds) + (size_t)wave * kStepPx * rf * (ROMIS_PT_LDS2 ? 2u : 1u);
        f4v v[kRowF4];
        auto fetch = [&](uint32_t step) {
            const f4v* src = reinterpret_cast<const f4v*>(tab + pt_index(pt_row_of_thread(tile, (wave << 6) + step * kStepPx), rf, 0u));
#pragma unroll
            for (uint32_t u = 0; u < kRowF4; u++)
                if (64u * u + lane < n4) v[u] = __builtin_nontemporal_load(src + 64u * u + lane);
        };
        if (ROMIS_PT_PREFETCH) fetch(0u);
#pragma unroll 1
        for (uint32_t step = 0; step < kSteps; step++) {
            if (!ROMIS_PT_PREFETCH) fetch(step);
            float* const l_rows = l_base + (ROMIS_PT_LDS2 ? (step & 1u) * kStepPx * rf : 0u);
            f4v* const dst = reinterpret_cast<f4v*>(l_rows);
#pragma unroll
            for (uint32_t u = 0; u < kRowF4; u++)
                if (64u * u + lane < n4) dst[64u * u + lane] = v[u];
            if (ROMIS_PT_PREFETCH && step + 1u < kSteps) fetch(step + 1u);
            // the step's pixel of this lane: thread tq of the block (tile_pixel_of's mapping, map2d = 1) and its RNG state
            const uint32_t tq = (wave << 6) + step * kStepPx + q;
            const uint32_t xq = rg.rx0 + (tile % ntx) * kTileW + tq % kTileW, yq = rg.ry0 + (tile / ntx) * kTileH + tq / kTileW;
            uint32_t psq[NB];
#pragma unroll
            for (uint32_t kb = 0; kb < NB; kb++) psq[kb] = pix_state(kb ? key1 : key, yq * rg.W + xq);
            const bool lq = s_loop[tq] != 0u;
            pt_wave_sync();
#pragma unroll
            for (uint32_t kb = 0; kb < NB; kb++) {   // phases A-D under key kb, over the same rows
                float w[kChunk], ws[kChunk];
#pragma unroll
                for (uint32_t k = 0; k < kChunk; k++)   // (an index past the chunk still reads inside the row)
                    w[k] = weight(l_rows[q * rf + uniform_index(draw(psq[kb], 4u * (c0 + k)), L)]);
                float run = ROMIS_FLT_MIN;
#pragma unroll
                for (uint32_t r = 0; r < kG; r++) {
                    const float left = pt_from_left(run);
                    run = j == 0u ? ROMIS_FLT_MIN : left;   // sub_init's wsum, or the total of the candidates before this chunk
#pragma unroll
                    for (uint32_t k = 0; k < kChunk; k++) {
                        run = c0 + k < c1 ? run + w[k] : run;
                        ws[k] = run;
                    }
                }
                uint32_t best = 0u;
#pragma unroll
                for (uint32_t k = 0; k < kChunk; k++) {
                    const bool acc = accept_u(rand01(draw(psq[kb], 4u * (c0 + k) + 3u)), w[k], ws[k]);
                    if (acc && c0 + k < c1) best = c0 + k + 1u;
                }
                best = pt_group_max(lq ? best : 0u);
                if (lq && j == kG - 1u) {   // the pixel's last lane holds the whole sum
                    s_wsum[kb][tq] = run;
                    s_best[kb][tq] = (best_t)best;
                    if (best) s_pd[kb][tq] = l_rows[q * rf + uniform_index(draw(psq[kb], 4u * (best - 1u)), L)];
                }
            }
            if (!ROMIS_PT_LDS2) pt_wave_sync();   // the rows are overwritten by the next step
        }
    }
    if (!live) return;
    // ris_pixel's tail (NT = 1, kLtPoint, no temporal reuse, no initial visibility rays)
#pragma unroll
    for (uint32_t kb = 0; kb < NB; kb++) {
        float* const rpk = kb ? rp1 : rp;   // key kb's planes
        float* const hwk = kb ? hw1 : hw;
        uint32_t* const hmk = kb ? hm1 : hm;
        Sub r;
        sub_init(r);
        r.M = M;
        r.wsum = s_wsum[kb][t];
        const uint32_t b = s_best[kb][t];
        uint32_t hidx = L;
        float pj;
        if (b) {
            hidx = uniform_index(draw(pix_state(kb ? key1 : key, y * rg.W + x), 4u * (b - 1u)), L);
            r.pos = xyz(s.light_c2[hidx]);
            r.col = xyz(s.light_c2[L + hidx]);
            pj = s_pd[kb][t];
            r.chosen = s.light_scale != 0.0f ? pj * s.light_scale : pj / (1.0f / (float)L);
        } else {
            pj = target_pdf(s, f, make_px(s, nt, pm, origin, p), r.pos, r.col, tb);
        }
        r.W = contribution_weight(pj, r.M, r.wsum);
        rpk[p] = pj;
        hwk[p] = r.W;
        hmk[p] = r.M | (hidx << 24);
    }
}

}  // namespace
}  // namespace romis

extern "C" __global__ __launch_bounds__(256) void k_gbuf_ris_n1_lds_pt_phat(
    SceneDev s, Region rg, FeaturesDev f, uint32_t key, float ox, float oy, float oz, const float4* n_t, const float4* p_mat,
    float4* ra, float4* rb, float2* rdbg, float* rp, const uint8_t* tmiss, uint32_t skip_res, float* hw, uint32_t* hm,
    uint32_t res_dead, const float* tab) {
    pt_ris_body<false>(s, rg, f, key, mk(ox, oy, oz), n_t, p_mat, ra, rb, rdbg, rp, tmiss, skip_res, hw, hm, res_dead, tab);
}
// ... with temporal reuse in the same kernel, as k_gbuf_ris_n1_lds_pt_temporal: no tile flags, every tile live
extern "C" __global__ __launch_bounds__(256) void k_gbuf_ris_n1_lds_pt_phat_temporal(
    SceneDev s, Region rg, FeaturesDev f, uint32_t key, float ox, float oy, float oz, const float4* n_t, const float4* p_mat,
    float4* ra, float4* rb, float2* rdbg, float* rp, TemporalIn tin, float* hw, uint32_t* hm, uint32_t res_dead,
    const float* tab) {
    pt_ris_body<true>(s, rg, f, key, mk(ox, oy, oz), n_t, p_mat, ra, rb, rdbg, rp, nullptr, 0u, hw, hm, res_dead, tab, tin);
}
// k_gbuf_ris_n1_lds_pt_phat for two RNG keys in one pass over the table (DESIGN.md §6 "RIS batch"): key k's pdf cache to
// rp_k, its handles to (hw_k, hm_k).  The reservoir planes are dead and there is no debug plane.
extern "C" __global__ __launch_bounds__(256) void k_gbuf_ris_n1_lds_pt_phat_batch2(
    SceneDev s, Region rg, FeaturesDev f, uint32_t key0, uint32_t key1, float ox, float oy, float oz, const float4* n_t,
    const float4* p_mat, float* rp0, float* rp1, const uint8_t* tmiss, uint32_t skip_res, float* hw0, uint32_t* hm0, float* hw1,
    uint32_t* hm1, const float* tab) {
    pt_ris_batch_body(s, rg, f, key0, mk(ox, oy, oz), n_t, p_mat, rp0, tmiss, skip_res, hw0, hm0, tab, key1, rp1, hw1, hm1);
}

namespace romis {

hipError_t launch_phat_table(const PhatTableDev& d, hipStream_t stream) {
    const uint32_t L = d.s.num_lights;
    if (!L || L > kPtMaxLights || !d.tab || !d.n_t || !d.p_mat || d.rg.map2d != 1u || d.rg.rw != d.rg.vw || d.rg.rh != d.rg.vh)
        return hipErrorInvalidValue;
    const uint32_t tiles = pt_tiles(d.rg.vw, d.rg.vh);
    if (!tiles) return hipSuccess;
    hipLaunchKernelGGL(k_phat_table, dim3(tiles), dim3(kPtTilePx), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_debug_phat(const PhatTableDev& d, uint32_t light, float* out, hipStream_t stream) {
    const Region& rg = d.rg;
    if (light >= d.s.num_lights) return hipErrorInvalidValue;
    if (!rg.rw || !rg.rh) return hipSuccess;
    hipLaunchKernelGGL(k_debug_phat, dim3((rg.rw + kTileW - 1u) / kTileW, (rg.rh + kTileH - 1u) / kTileH), dim3(256), 0, stream, d,
                       light, out);
    return hipGetLastError();
}

// launch_primary_ris's k_gbuf_ris launch for a route with `phat` (route_primary_ris): the same arguments and the table
hipError_t launch_gbuf_ris_phat(const Route& r, const SceneDev& s, const Region& rg0, const FeaturesDev& f, const LaunchBufs& b,
                                hipStream_t stream) {
    const bool temporal = r.kernel == Kernel::kGbufRisTemporal;
    if ((r.kernel != Kernel::kGbufRis && !temporal) || !r.phat || !b.phat || r.n != 1u || r.lt != kLtPoint || r.map2d != 1u || f.initial_vis)
        return hipErrorInvalidValue;
    const Region rg = r.region(rg0);
    const float* o = b.origin;
    // the route admits pt_fast shapes alone; a build with ROMIS_PT_G != 4 takes its own steps' rows
    if (!pt_fast(s.num_lights, f.M) || r.lds != pt_lds_bytes(s.num_lights)) return hipErrorInvalidValue;
    const size_t lds = (size_t)4u * kStepPx * pt_row_floats(s.num_lights) * 4u * (ROMIS_PT_LDS2 ? 2u : 1u);
    if ((kG == 2u || ROMIS_PT_LDS2) && lds + 4096u > kLdsBudget) {   // (A/B forms: more LDS than a kernel gets by default)
        static bool raised = false;
        if (!raised) {
            for (const void* k : {reinterpret_cast<const void*>(k_gbuf_ris_n1_lds_pt_phat),
                                  reinterpret_cast<const void*>(k_gbuf_ris_n1_lds_pt_phat_temporal)}) {
                const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
                if (e != hipSuccess) return e;
            }
            raised = true;
        }
    } else if (lds + 4096u > kLdsBudget) {
        return hipErrorInvalidValue;
    }
    if (temporal) {
        ROMIS_LAUNCH(k_gbuf_ris_n1_lds_pt_phat_temporal, dim3(r.grid), dim3(r.block), lds, stream, s, rg, f, b.key, o[0], o[1], o[2],
                     (const float4*)b.n_t, (const float4*)b.p_mat, b.oa, b.ob, r.dbg ? b.dbg : nullptr,
                     r.rp_out ? b.rp_out : nullptr, b.tin, r.how ? b.hout.w : nullptr, r.hom ? b.hout.m : nullptr, r.res_dead,
                     b.phat);
        return hipGetLastError();
    }
    ROMIS_LAUNCH(k_gbuf_ris_n1_lds_pt_phat, dim3(r.grid), dim3(r.block), lds, stream, s, rg, f, b.key, o[0], o[1], o[2], (const float4*)b.n_t,
                 (const float4*)b.p_mat, b.oa, b.ob, r.dbg ? b.dbg : nullptr, r.rp_out ? b.rp_out : nullptr,
                 r.flags ? (const uint8_t*)b.flags : nullptr, r.skip, r.how ? b.hout.w : nullptr, r.hom ? b.hout.m : nullptr,
                 r.res_dead, b.phat);
    return hipGetLastError();
}

// A frame's routed launch_gbuf_ris_phat launch for two RNG keys at once: key k's handles to out[k].h, its pdf cache to
// out[k].rp; b's own key, hout and rp_out are not used.  The route is one whose reservoir planes are dead and that
// writes both handle planes and the pdf cache, without temporal reuse or the debug plane (the look-ahead's frames).
hipError_t launch_gbuf_ris_phat_batch(const Route& r, const SceneDev& s, const Region& rg0, const FeaturesDev& f, const LaunchBufs& b,
                                      const RisBatchOut (&out)[2], hipStream_t stream) {
    if (r.kernel != Kernel::kGbufRis || !r.phat || !b.phat || r.n != 1u || r.lt != kLtPoint || r.map2d != 1u || f.initial_vis)
        return hipErrorInvalidValue;
    if (!r.res_dead || r.dbg || !r.how || !r.hom || !r.rp_out) return hipErrorInvalidValue;
    for (const RisBatchOut& o : out)
        if (!o.h.w || !o.h.m || !o.rp) return hipErrorInvalidValue;
    if (out[0].h.w == out[1].h.w || out[0].h.m == out[1].h.m || out[0].rp == out[1].rp) return hipErrorInvalidValue;
    const Region rg = r.region(rg0);
    const float* o = b.origin;
    if (!pt_fast(s.num_lights, f.M) || r.lds != pt_lds_bytes(s.num_lights)) return hipErrorInvalidValue;
    if (kG != kPtLanesPerPx || ROMIS_PT_LDS2) return hipErrorInvalidValue;   // (the A/B forms have no batch kernel)
    const size_t lds = pt_lds_bytes(s.num_lights);
    if (lds + 8192u > kLdsBudget) return hipErrorInvalidValue;   // (static LDS: 5,376 B)
    ROMIS_LAUNCH(k_gbuf_ris_n1_lds_pt_phat_batch2, dim3(r.grid), dim3(r.block), lds, stream, s, rg, f, out[0].key, out[1].key, o[0], o[1],
                 o[2], (const float4*)b.n_t, (const float4*)b.p_mat, out[0].rp, out[1].rp, r.flags ? (const uint8_t*)b.flags : nullptr,
                 r.skip, out[0].h.w, out[0].h.m, out[1].h.w, out[1].h.m, b.phat);
    return hipGetLastError();
}

}  // namespace romis
