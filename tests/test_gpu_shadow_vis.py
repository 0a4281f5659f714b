"""final.vis (the default): once a still view's shadow lists stand, the frame whose streak of reusing frames reaches
final.vis_after (4) runs k_shadow_vis, which asks every (pixel, point light) ray of the lists once and keeps the answer as
one bit (csrc/shadow_vis.h); from that frame on the fused last pass (k_spatial1hg_t2_final_vis) reads its rays' answers.
A stored bit is the return value of the very call the lists kernel makes, so every frame must equal, bit for bit, the
frame of a context that never uses the lists (final.lists = 0) -- no tolerances anywhere in this file.

Renderer.shadow_vis_frames() counts the frames that read the bits (shadow_list_frames() keeps counting them too),
shadow_vis_builds() the builds, and debug_shadow_vis(light) returns one light's stored bits (0xFF where none is held).

Frame numbers below: frame 0 traces, frame k >= 1 is the k-th reusing frame (the streak); lists from frame 2, bits from
frame 4.  Sizes as tests/test_gpu_shadow_lists.py: 96 x 48 (3 x 3 whole tiles) and the ragged 70 x 37.
"""
import numpy as np
import pytest

from romis_amd import _abi, restir, scene
from test_gpu_shadow_lists import NIGHTCLUB, SIZES, Pair, camera, features, lights_around, make_scene, pair, point_light  # noqa: F401
from test_gpu_parity import get_scene

pytestmark = pytest.mark.gpu

LISTS = [0, 0, 1, 2, 3, 4, 5]   # shadow_list_frames after frames 0 .. 6: today's sequence
BITS = [0, 0, 0, 0, 1, 2, 3]    # shadow_vis_frames


def run_frames(p, cam, w, h, f, what, n=7, first=0, **kw):
    """Frames first .. n - 1 of a still view on both contexts, the counters checked after each"""
    for frame in range(first, n):
        p.frame(cam, w, h, f, what, **kw)
        assert p.new.shadow_list_frames() == LISTS[frame], f"{what}: frame {frame}"
        assert p.new.shadow_vis_frames() == BITS[frame], f"{what}: frame {frame}"
    assert p.new.shadow_vis_builds() == (1 if n > 4 else 0)


def bits_equal_the_walk(r, lights, w, h, what):
    """debug_shadow_vis against the BVH-walk plane of debug_shadow_lists wherever a bit is held; returns (held, occluded,
    pixels without bits)"""
    held_n = occluded = 0
    none = None
    for light in lights:
        walk, _ = r.debug_shadow_lists(light, w, h)
        bits = r.debug_shadow_vis(light, w, h)
        held = bits != 0xFF
        assert np.isin(bits, (0, 1, 0xFF)).all()
        assert not (walk[held] == 0xFF).any(), f"{what} light {light}: bits held for background pixels"
        assert np.array_equal(bits[held], walk[held]), f"{what} light {light}: {(bits[held] != walk[held]).sum()} bits differ"
        assert none is None or np.array_equal(none, ~held), f"{what} light {light}: another set of pixels holds bits"
        none = ~held
        held_n += int(held.sum())
        occluded += int((bits == 0).sum())
    return held_n, occluded, none


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHTCLUB, "cube_points"])
def test_still_frames_equal_and_counted(pair, name, w, h):
    """Frames 0-6 of a still camera: bit-identical to final.lists = 0; the bits counter reads 0 until frame 4, the lists
    counter runs as it did before there were bits."""
    p = pair(make_scene(name))
    run_frames(p, camera(name, w, h), w, h, features(1), f"{name} {w}x{h}")
    assert p.new.gbuf_reuses() == 6


@pytest.mark.parametrize("name,w,h", [(NIGHTCLUB, 96, 48), (NIGHTCLUB, 70, 37), ("cube_points", 70, 37)])
def test_every_stored_bit_equals_the_walk(pair, name, w, h):
    """Every light's plane: at 96 x 48, 128 x 4,608 bits.  Both answers occur, so the comparison is not vacuous."""
    sc = make_scene(name)
    p = pair(sc)
    run_frames(p, camera(name, w, h), w, h, features(1), name, n=5)
    held, occluded, _ = bits_equal_the_walk(p.new, range(len(sc.lights)), w, h, name)
    assert held > 0 and 0 < occluded < held
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_vis: INVALID: .*light"):
        p.new.debug_shadow_vis(len(sc.lights), w, h)   # the zero sample has no bits
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_vis: INVALID: .*rectangle"):
        p.new.debug_shadow_vis(0, w + 1, h)


def test_debug_entry_needs_bits(pair):
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), "lists only", n=4)   # lists, no bits yet
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_vis: STATE: .*no visibility bits"):
        p.new.debug_shadow_vis(0, w, h)


@pytest.mark.parametrize("cap", [1, 3])
def test_short_records_walk_for_the_whole_wave(pair, cap):
    """final.lists_cap 1 and 3: most records say "walk the BVH", which the builder does for all of a wave's pixels"""
    w, h = 96, 48
    p = pair(make_scene(NIGHTCLUB), cap=cap)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), f"cap {cap}")
    held, occluded, _ = bits_equal_the_walk(p.new, (0, 31, 32, 64, 127), w, h, f"cap {cap}")
    assert 0 < occluded < held


@pytest.mark.parametrize("w,h", SIZES)
def test_tile_with_an_origin(pair, w, h):
    """The right-hand tile of a 2 x 1 split: the plane covers a rect that starts at x0 > 0 inside a ghost-zoned view"""
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    tile = restir.tile_plan(w, h, 2, 1, 1, f.spatial_resample_radius)
    assert tile.x0 > 0
    run_frames(p, cam, w, h, f, f"tile {w}x{h}", tile=tile)
    held, _, _ = bits_equal_the_walk(p.new, (0, 77, 127), tile.width, tile.height, "tile")
    assert held > 0


@pytest.mark.parametrize("n", [1, 33, 200])
def test_light_counts(pair, n):
    """1, 33 and 200 point lights around the nightclub's geometry: a partial only word, a second word with one bit, and
    seven words with a partial last one"""
    w, h = 70, 37
    base = get_scene(NIGHTCLUB)
    sc = scene.Scene(base.meshes, lights_around(base, n - 1, 11 + n, radius=0.3), f"nightclub_{n}pt")
    assert len(sc.lights) == n
    p = pair(sc)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), f"{n} lights")
    held, _, _ = bits_equal_the_walk(p.new, sorted({0, min(31, n - 1), min(32, n - 1), n // 2, n - 1}), w, h, f"{n} lights")
    assert held > 0


def test_kept_grid_with_temporal_reuse(pair):
    """C3's shape: two passes, temporal reuse, the grid kept and threaded into the next frame"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(2, temporal_reuse=1)
    prev = (None, None)
    for frame in range(7):
        prev = p.frame(cam, w, h, f, "temporal", want_grid=True, prev=prev)
        assert p.new.shadow_list_frames() == LISTS[frame] and p.new.shadow_vis_frames() == BITS[frame], f"frame {frame}"


def test_far_camera_background_tiles_hold_no_bits(pair):
    w, h = 96, 48
    p = pair(make_scene(NIGHTCLUB))
    far = scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)   # background tiles too
    run_frames(p, far, w, h, features(1), "far camera")
    held, _, none = bits_equal_the_walk(p.new, (0, 9, 127), w, h, "far camera")
    assert held > 0 and none.any()
    walk, _ = p.new.debug_shadow_lists(9, w, h)
    assert (walk == 0xFF).any() and none[walk == 0xFF].all()


# --------------------------------------------------------------------------------------------------------
# what drops the bits: each stops the bits frames and the right later frame builds them again
def after(p, cam, w, h, f, what, counts):
    """Frames after an event; counts: shadow_vis_frames expected after each"""
    for k, want in enumerate(counts):
        p.frame(cam, w, h, f, what)
        assert p.new.shadow_vis_frames() == want, f"{what}: frame {k} after"


def started(pair, w=70, h=37):
    sc = make_scene(NIGHTCLUB)
    p = pair(sc)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    run_frames(p, cam, w, h, f, "before", n=6)
    assert p.new.shadow_vis_frames() == 2 and p.new.shadow_vis_builds() == 1
    return sc, p, cam, f


def test_lights_set_between_frames(pair):
    """restir_set_lights keeps the G-buffer and restarts the streak: reusing frames 1-3 without bits, the fourth builds"""
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    moved = [point_light([l.p0[0] + 0.25, l.p0[1], l.p0[2] - 0.5], list(l.c0)) for l in sc.lights]
    p.each(lambda r: r.set_lights(moved))
    after(p, cam, w, h, f, "moved lights", [2, 2, 2, 3, 4])
    assert p.new.shadow_vis_builds() == 2
    bits_equal_the_walk(p.new, (0, 100), w, h, "moved lights")


def test_meshes_updated_between_frames(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    big = max(range(len(sc.meshes)), key=lambda i: len(sc.meshes[i].positions))
    pos = np.asarray(sc.meshes[big].positions, np.float32) + np.float32([0.125, 0.0, -0.0625])
    p.each(lambda r: r.update_meshes({big: (pos, None)}))
    after(p, cam, w, h, f, "moved mesh", [2, 2, 2, 2, 3, 4])   # a tracing frame first
    assert p.new.shadow_vis_builds() == 2
    bits_equal_the_walk(p.new, (5,), w, h, "moved mesh")


def test_camera_changed_between_frames(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    far = scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)
    after(p, far, w, h, f, "far camera", [2, 2, 2, 2, 3, 4])
    assert p.new.shadow_vis_builds() == 2
    bits_equal_the_walk(p.new, (9,), w, h, "far camera")


def test_scene_set_again(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    p.each(lambda r: r.set_scene(sc))
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_vis: STATE"):
        p.new.debug_shadow_vis(0, w, h)
    after(p, cam, w, h, f, "scene again", [2, 2, 2, 2, 3, 4])
    assert p.new.shadow_vis_builds() == 2


def test_final_vis_off_and_on_again(pair):
    """final.vis = 0 frees the plane (and, as any launch-shape knob, makes the next frame trace): lists frames go on,
    bits frames stop; switched on again the bits come back with the fourth reusing frame"""
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    p.new.set_tuning("final.vis", 0)
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_vis: STATE"):
        p.new.debug_shadow_vis(0, w, h)
    lists = p.new.shadow_list_frames()
    after(p, cam, w, h, f, "vis off", [2, 2, 2, 2, 2, 2])
    assert p.new.shadow_list_frames() == lists + 4 and p.new.shadow_vis_builds() == 1
    p.new.set_tuning("final.vis", 1)
    after(p, cam, w, h, f, "vis on again", [2, 2, 2, 2, 3, 4])
    assert p.new.shadow_vis_builds() == 2


# --------------------------------------------------------------------------------------------------------
# knobs that cannot change a stored byte keep the G-buffer, the lists and the bits
@pytest.mark.parametrize("key,value", [("timing.mask", -1), ("timing.every", 3), ("timing.fence", 1), ("final.lists_after", 1),
                                       ("final.vis_after", 3)])
def test_knob_keeps_the_caches(pair, key, value):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    r = p.new
    before = (r.gbuf_reuses(), r.shadow_list_frames(), r.shadow_vis_frames())
    r.set_tuning(key, value)
    p.frame(cam, w, h, f, key)   # against a context that never touched the knob
    assert (r.gbuf_reuses(), r.shadow_list_frames(), r.shadow_vis_frames()) == tuple(x + 1 for x in before), key
    assert r.shadow_vis_builds() == 1, f"{key}: the bits were built again"
    bits_equal_the_walk(r, (3,), w, h, key)
    # the control: a knob that may change what a frame stores still forces a tracing frame
    r.set_tuning("miss.tiles", 1)
    p.frame(cam, w, h, f, "miss.tiles")
    assert (r.gbuf_reuses(), r.shadow_list_frames(), r.shadow_vis_frames()) == tuple(x + 1 for x in before)


def test_vis_after_below_lists_after_is_refused(pair):
    p = pair(make_scene(NIGHTCLUB))
    with pytest.raises(_abi.RestirError, match=r"final.vis_after: >= final.lists_after"):
        p.new.set_tuning("final.vis_after", 1)
