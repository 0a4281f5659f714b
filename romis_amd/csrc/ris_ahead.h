// ris_ahead.h -- the key of a RIS look-ahead result (restir.cpp Frame::ris_stage, DESIGN.md §6 "RIS look-ahead").
// On a still view without temporal reuse, frame f + 1's RIS (k_gbuf_ris_n1_lds_pt_phat) reads nothing frame f writes, so
// restir_render launches it on a second stream beside frame f's last pass, into a second set of handle and pdf-cache
// planes.  The key names everything that launch's output is a function of; the next restir_render call takes the
// result only when the key of the frame it is about to render is equal, field for field.  Host only, no HIP include: a
// CPU test compiles it (tests/cpp/ris_ahead_key.cpp).
#pragma once

#include <cstdint>
#include <cstring>

namespace romis {

struct RisAheadKey {
    // the RNG key's inputs: restir_rng_key(seed, frame, RESTIR_STAGE_RIS, 0)
    uint32_t seed = 0, frame = 0;
    // what the launch read: the kept G-buffer (restir_ctx::gbuf_epoch names one), the light table and materials
    // (scene_gen), the geometry the G-buffer was traced over (geom_gen), one build of the p-hat table (phat_builds)
    uint64_t gbuf_epoch = 0, scene_gen = 0, geom_gen = 0, phat_build = 0;
    // the GbufView: CameraDev as bits (quat, origin, half_w, half_h), the image size, the restir_tile's ten words
    uint32_t cam[9] = {};
    uint32_t width = 0, height = 0;
    uint32_t tile[10] = {};
    uint32_t tex_on = 0;
    // FeaturesDev, whole: ris_pixel takes M, N, shading, initial_vis and texture; the frame's plan (handles, tile flags,
    // what RIS may skip) takes the passes' K, R, unbiased and spatial_vis, so a result is not kept across any of them
    uint32_t features[22] = {};
    uint32_t passes = 0;
    // the launch as routed: Route::grid, ::lds, and its buffer decisions (ris_ahead_route_bits)
    uint32_t route_grid = 0, route_lds = 0, route_bits = 0;
    // counts the restir_set_tuning calls of knobs that clear the kept G-buffer
    uint64_t tuning_gen = 0;
};

constexpr uint32_t kRisAheadKeyFields = 17;   // members above; the test has one case per member
static_assert(sizeof(RisAheadKey) == 4 * (2 + 9 + 2 + 10 + 1 + 22 + 1 + 3) + 8 * 5,
              "RisAheadKey changed: compare the new member in ris_ahead_key_equal, count it in kRisAheadKeyFields and "
              "give it a case in tests/cpp/ris_ahead_key.cpp");

inline bool ris_ahead_key_equal(const RisAheadKey& a, const RisAheadKey& b) {
    return a.seed == b.seed && a.frame == b.frame && a.gbuf_epoch == b.gbuf_epoch && a.scene_gen == b.scene_gen &&
           a.geom_gen == b.geom_gen && a.phat_build == b.phat_build && !std::memcmp(a.cam, b.cam, sizeof(a.cam)) &&
           a.width == b.width && a.height == b.height && !std::memcmp(a.tile, b.tile, sizeof(a.tile)) &&
           a.tex_on == b.tex_on && !std::memcmp(a.features, b.features, sizeof(a.features)) && a.passes == b.passes &&
           a.route_grid == b.route_grid && a.route_lds == b.route_lds && a.route_bits == b.route_bits &&
           a.tuning_gen == b.tuning_gen;
}

// The key of the frame after `k` on the same view: what a look-ahead launched beside frame k.frame is keyed by
inline RisAheadKey ris_ahead_next(RisAheadKey k) {
    k.frame += 1u;
    return k;
}

// Which of two plane sets a frame's grid 0 reads its handles and pdf cache from, and the one the look-ahead beside it
// writes: the other
inline int ris_ahead_other_set(int set) { return set ^ 1; }

// ---- RIS batch (DESIGN.md §6 "RIS batch"): one look-ahead launch may serve two frames, so results wait in a small ring.
// Plane set 0 is the frame's own (hnd[0], rp[0]); sets 1 .. kRisSets - 1 are the look-ahead's.  A result is pending from
// its launch until a frame takes it or everything pending is dropped; its set is busy that long, and the set a frame
// reads is busy for that frame.  tests/cpp/ris_batch_ring.cpp walks every reachable state of both cadences.

constexpr int kRisSets = 4;        // cadence (a) uses 3 of them, (b) all 4 (ris_batch_sets)
constexpr int kRisRingSlots = 3;   // cadence (b) launches two results with one still pending

// The key of the n-th frame after `k` on the same view (n = 1: ris_ahead_next)
inline RisAheadKey ris_ahead_nth(RisAheadKey k, uint32_t n) {
    k.frame += n;
    return k;
}

struct RisRingSlot {
    bool valid = false;
    int set = 0;           // the plane set the result lies in
    uint64_t launch = 0;   // the look-ahead launch that wrote it (RisRing::launches at that time): a batch's two share one
    RisAheadKey key;
};
struct RisRing {
    RisRingSlot slot[kRisRingSlots];
    uint64_t launches = 0;
};

inline int ris_ring_pending(const RisRing& r) {
    int n = 0;
    for (const RisRingSlot& s : r.slot) n += s.valid ? 1 : 0;
    return n;
}
// The sets no launch may write while a frame reads `read_set`: that one and every pending result's (bit s: set s)
inline uint32_t ris_ring_busy(const RisRing& r, int read_set) {
    uint32_t m = 1u << read_set;
    for (const RisRingSlot& s : r.slot)
        if (s.valid) m |= 1u << s.set;
    return m;
}
// The pending result keyed `k` (-1: none)
inline int ris_ring_find(const RisRing& r, const RisAheadKey& k) {
    for (int i = 0; i < kRisRingSlots; i++)
        if (r.slot[i].valid && ris_ahead_key_equal(r.slot[i].key, k)) return i;
    return -1;
}
// The n lowest of the first `sets` plane sets outside `busy`, ascending; false: fewer than n are free
inline bool ris_ring_pick(uint32_t busy, int n, int sets, int* out) {
    int got = 0;
    for (int s = 0; s < sets && got < n; s++)
        if (!((busy >> s) & 1u)) out[got++] = s;
    return got == n;
}
// One launch's n results (keys[i] in sets[i]) become pending; slots[i]: where.  false: the ring has no room (nothing changed)
inline bool ris_ring_push(RisRing& r, int n, const RisAheadKey* keys, const int* sets, int* slots) {
    if (ris_ring_pending(r) + n > kRisRingSlots) return false;
    r.launches++;
    int at = 0;
    for (int i = 0; i < n; i++) {
        while (r.slot[at].valid) at++;
        r.slot[at].valid = true;
        r.slot[at].set = sets[i];
        r.slot[at].launch = r.launches;
        r.slot[at].key = keys[i];
        slots[i] = at;
    }
    return true;
}
inline void ris_ring_take(RisRing& r, int i) { r.slot[i].valid = false; }
// Every pending result dropped: the number of launches with a result nobody took (restir_ahead_discards counts launches,
// so a batch whose first result was taken and one whose results both wait count one each)
inline uint32_t ris_ring_drop(RisRing& r) {
    uint32_t n = 0;
    for (int i = 0; i < kRisRingSlots; i++) {
        if (!r.slot[i].valid) continue;
        bool seen = false;
        for (int j = 0; j < i; j++) seen = seen || (r.slot[j].valid && r.slot[j].launch == r.slot[i].launch);
        n += seen ? 0u : 1u;
    }
    for (RisRingSlot& s : r.slot) s.valid = false;
    return n;
}

// Cadence.  How many results the look-ahead beside a frame launches, with `pending` results waiting once the frame took
// its own: below the batch streak one when none waits (the single look-ahead); from it on (`batching`) two -- form 0
// when none waits, form 1 when at most one does, so that a batch runs beside two frames' last passes.
inline int ris_batch_launch(uint32_t batch, uint32_t form, bool batching, int pending) {
    if (batch == 2u && batching) return pending <= (form ? 1 : 0) ? 2 : 0;
    return pending == 0 ? 1 : 0;
}
// Plane sets a cadence needs, set 0 included: the one being read, the pending ones, the two being written
inline int ris_batch_sets(uint32_t batch, uint32_t form) { return batch == 2u ? (form ? 4 : 3) : 2; }

}  // namespace romis
