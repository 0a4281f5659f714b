// ris_batch_ring.cpp -- csrc/ris_ahead.h's result ring and batch cadences on the CPU (tests/test_ris_batch_ring.py).
// A model of restir_render's use of the header: each frame takes the result keyed as itself (or runs its own RIS into
// set 0), the look-ahead beside it launches ris_batch_launch's count of results into ris_ring_pick's sets, and at any
// frame boundary everything pending may be dropped.  The walk covers every state reachable under each (batch, form) by
// breadth-first search over (ring contents, the set the last frame read); at every launch it checks that no set handed
// to the writer is pending or being read.  Prints one line per fact; the Python test asserts them.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "ris_ahead.h"

using namespace romis;

namespace {

RisAheadKey base_key() {
    RisAheadKey k;
    k.seed = 7; k.frame = 100; k.gbuf_epoch = 3; k.scene_gen = 4; k.geom_gen = 5; k.phat_build = 6;
    for (int i = 0; i < 9; i++) k.cam[i] = 10u + (uint32_t)i;
    k.width = 70; k.height = 37;
    for (int i = 0; i < 10; i++) k.tile[i] = 20u + (uint32_t)i;
    k.tex_on = 1;
    for (int i = 0; i < 22; i++) k.features[i] = 40u + (uint32_t)i;
    k.passes = 1; k.route_grid = 15; k.route_lds = 8192; k.route_bits = 0x1234; k.tuning_gen = 9;
    return k;
}

struct State {
    RisRing ring;
    uint32_t frame;    // the next frame's index
    uint32_t streak;   // the next frame's streak
};

// the state's shape: per slot (valid, set, frames ahead of the next frame, launch age rank), and whether it batches
std::string shape(const State& s, uint32_t batch_after) {
    std::string out = s.streak >= batch_after ? "B" : std::to_string(s.streak);
    for (const RisRingSlot& sl : s.ring.slot) {
        if (!sl.valid) { out += "|-"; continue; }
        int older = 0;
        for (const RisRingSlot& o : s.ring.slot) older += (o.valid && o.launch < sl.launch) ? 1 : 0;
        out += "|" + std::to_string(sl.set) + "," + std::to_string(sl.key.frame - s.frame) + "," + std::to_string(older);
    }
    return out;
}

struct Walk {
    int states = 0, launches = 0, bad_sets = 0, bad_takes = 0, bad_keys = 0, max_pending = 0, max_set = 0, bad_discards = 0;
};

// One frame of the still view from state s: take or own RIS, then the look-ahead.  Returns the state after it.
State frame(State s, uint32_t batch, uint32_t form, uint32_t ahead_after, uint32_t batch_after, Walk& w) {
    RisAheadKey key = base_key();
    key.frame = s.frame;
    int read_set = 0;
    if (s.streak >= ahead_after) {
        const int slot = ris_ring_find(s.ring, key);
        if (slot >= 0) {
            read_set = s.ring.slot[slot].set;
            ris_ring_take(s.ring, slot);
        } else if (ris_ring_pending(s.ring)) {
            w.bad_takes++;   // a still view's next frame always finds its result when any waits
        }
        const int pending = ris_ring_pending(s.ring);
        for (int i = 1; i <= pending; i++)
            if (ris_ring_find(s.ring, ris_ahead_nth(key, (uint32_t)i)) < 0) w.bad_keys++;
        const bool batching = s.streak >= (batch_after > ahead_after ? batch_after : ahead_after);
        const int n = ris_batch_launch(batch, form, batching, pending);
        if (n) {
            int sets[2] = {-1, -1}, slots[2] = {-1, -1};
            const uint32_t busy = ris_ring_busy(s.ring, read_set);
            if (!ris_ring_pick(busy, n, ris_batch_sets(batch, form), sets)) w.bad_sets++;
            RisAheadKey keys[2];
            for (int i = 0; i < n; i++) {
                if (sets[i] < 0 || sets[i] >= kRisSets || ((busy >> sets[i]) & 1u) || (i == 1 && sets[1] == sets[0])) w.bad_sets++;
                if (sets[i] > w.max_set) w.max_set = sets[i];
                keys[i] = ris_ahead_nth(key, (uint32_t)(pending + 1 + i));
            }
            if (!ris_ring_push(s.ring, n, keys, sets, slots)) w.bad_sets++;
            w.launches++;
        }
        if (ris_ring_pending(s.ring) > w.max_pending) w.max_pending = ris_ring_pending(s.ring);
    }
    s.frame++;
    s.streak++;
    return s;
}

Walk walk(uint32_t batch, uint32_t form, uint32_t ahead_after, uint32_t batch_after) {
    Walk w;
    std::set<std::string> seen;
    std::vector<State> todo;
    State s0{};
    s0.frame = 100;
    s0.streak = 1;
    todo.push_back(s0);
    while (!todo.empty()) {
        State s = todo.back();
        todo.pop_back();
        if (!seen.insert(shape(s, (batch_after > ahead_after ? batch_after : ahead_after) + 2u)).second) continue;
        w.states++;
        // the view goes on ...
        todo.push_back(frame(s, batch, form, ahead_after, batch_after, w));
        // ... or something changes here: every pending result is dropped, one discard per launch among them
        State d = s;
        std::set<uint64_t> ls;
        for (const RisRingSlot& sl : d.ring.slot)
            if (sl.valid) ls.insert(sl.launch);
        if (ris_ring_drop(d.ring) != ls.size() || ris_ring_pending(d.ring) != 0) w.bad_discards++;
        d.streak = 1;
        todo.push_back(d);
    }
    return w;
}

}  // namespace

int main() {
    // the n-th key differs from k in `frame` alone
    const RisAheadKey k = base_key();
    for (uint32_t n = 0; n <= 3; n++) {
        RisAheadKey m = ris_ahead_nth(k, n);
        const bool frame_ok = m.frame == k.frame + n;
        m.frame = k.frame;
        std::printf("nth %u %d %d %d\n", n, frame_ok ? 1 : 0, ris_ahead_key_equal(m, k) ? 1 : 0,
                    ris_ahead_key_equal(ris_ahead_nth(k, n), k) ? 1 : 0);
    }
    std::printf("nth_is_next %d\n", ris_ahead_key_equal(ris_ahead_nth(k, 1), ris_ahead_next(k)) ? 1 : 0);
    RisAheadKey last = k;
    last.frame = 0xFFFFFFFFu;
    std::printf("nth_wraps %u\n", ris_ahead_nth(last, 2).frame);

    // pick: lowest free sets, ascending; refuses when too few are free
    int out[2] = {-1, -1};
    bool ok = ris_ring_pick(0x1u, 2, 4, out);
    std::printf("pick %d %d %d\n", ok ? 1 : 0, out[0], out[1]);
    ok = ris_ring_pick(0x6u, 2, 4, out);
    std::printf("pick_b %d %d %d\n", ok ? 1 : 0, out[0], out[1]);
    std::printf("pick_full %d\n", ris_ring_pick(0x7u, 2, 4, out) ? 1 : 0);
    std::printf("pick_three_sets %d\n", ris_ring_pick(0x3u, 2, 3, out) ? 1 : 0);

    // discards per launch: a batch with both results pending, with one taken, two launches, nothing
    {
        RisRing r;
        int sets[2] = {1, 2}, slots[2];
        RisAheadKey keys[2] = {ris_ahead_nth(k, 1), ris_ahead_nth(k, 2)};
        ris_ring_push(r, 2, keys, sets, slots);
        RisRing both = r;
        std::printf("drop_both %u\n", ris_ring_drop(both));
        ris_ring_take(r, ris_ring_find(r, keys[0]));
        RisRing second = r;
        std::printf("drop_second %u\n", ris_ring_drop(second));
        int sets2[2] = {0, 3};
        RisAheadKey keys2[2] = {ris_ahead_nth(k, 3), ris_ahead_nth(k, 4)};
        std::printf("push_second_launch %d\n", ris_ring_push(r, 2, keys2, sets2, slots) ? 1 : 0);
        std::printf("busy %u\n", ris_ring_busy(r, 1));
        std::printf("push_full %d %d\n", ris_ring_push(r, 1, keys2, sets2, slots) ? 1 : 0, ris_ring_pending(r));
        std::printf("drop_two_launches %u\n", ris_ring_drop(r));
        std::printf("drop_nothing %u %d\n", ris_ring_drop(r), ris_ring_pending(r));
        std::printf("find_after_drop %d\n", ris_ring_find(r, keys[1]));
    }

    // every reachable state of each cadence: "walk <batch> <form> <states> <launches> <bad sets> <bad takes> <bad keys>
    // <bad discards> <max pending> <max set>"
    for (uint32_t batch = 1; batch <= 2; batch++)
        for (uint32_t form = 0; form <= 1; form++)
            for (uint32_t after : {3u, 8u}) {
                const Walk w = walk(batch, form, 3u, after);
                std::printf("walk %u %u %u %d %d %d %d %d %d %d %d\n", batch, form, after, w.states, w.launches, w.bad_sets,
                            w.bad_takes, w.bad_keys, w.bad_discards, w.max_pending, w.max_set);
            }
    // batch_after below ahead_after: batches start with the look-ahead, not before
    {
        const Walk w = walk(2u, 1u, 4u, 1u);
        std::printf("walk_low_after %d %d %d %d\n", w.bad_sets, w.bad_takes, w.bad_keys, w.max_pending);
    }
    std::printf("sets %d %d %d %d\n", ris_batch_sets(1, 0), ris_batch_sets(1, 1), ris_batch_sets(2, 0), ris_batch_sets(2, 1));
    return 0;
}
