"""frames.ahead (the default): on a still view whose RIS reads the p-hat table, without temporal reuse, a frame launches
the next frame's RIS on the context's second stream beside its own last pass, and the next frame takes that result when
its key (csrc/ris_ahead.h) is the stored one.  The look-ahead is the same launch under the next frame's RNG key into
other planes, so every frame must equal, bit for bit, the frame of a context with frames.ahead = 0 -- no tolerances
anywhere in this file.  (tests/test_gpu_phat_table.py ties the table's frames to ris.phat = 0, and those to the oracle.)

Frame numbers: frame 0 traces, frame k >= 1 is the k-th reusing frame (the streak).  Both contexts run ris.phat_after =
frames.ahead_after = AFTER = 3: frame 3 builds the table, runs its own RIS and launches frame 4's; frame 4 is the first
that takes a look-ahead result, so after frame k Renderer.ahead_frames() reads max(0, k - AFTER).  ahead_discards()
counts the results no frame took.  Sizes, as the p-hat tests chose them: 96 x 48 (whole 32 x 8 tiles), 70 x 37 (ragged)
and 33 x 9 (one pixel past a tile each way).
"""
import dataclasses

import numpy as np
import pytest

from romis_amd import _abi, restir, scene
from test_gpu_parity import SEED, assert_bits
from test_gpu_shadow_lists import NIGHTCLUB, camera, make_scene, point_light

pytestmark = pytest.mark.gpu

AFTER = 3
SIZES = [(96, 48), (70, 37), (33, 9)]


def features(passes=1, M=32, **kw):
    kw.setdefault("temporal_reuse", 0)
    return _abi.default_features(num_samples_in_reservoir=1, spatial_resampling_passes=passes, spatial_reuse=1,
                                 initial_light_samples=M, **kw)


class Pair:
    """Two contexts over one scene: `new` with the look-ahead from the AFTER-th reusing frame, `old` with frames.ahead = 0;
    frame() renders the same frame on both and asserts equal bits of the image and, where taken, the returned grid."""

    def __init__(self, sc, **knobs):
        self.new, self.old = restir.Renderer(0), restir.Renderer(0)
        self.old.set_tuning("frames.ahead", 0)
        for r in (self.new, self.old):
            r.set_tuning("ris.phat_after", AFTER)
            r.set_tuning("frames.ahead_after", AFTER)
        for k, v in knobs.items():   # a frames.* knob chooses the look-ahead's form: `new` alone
            for r in (self.new,) if k.startswith("frames") else (self.new, self.old):
                r.set_tuning(k.replace("__", "."), v)
        for r in (self.new, self.old):
            r.set_scene(sc)
            r.set_seed(SEED, 0)
        self.n = 0

    def each(self, fn):
        fn(self.new)
        fn(self.old)

    def frame(self, cam, w, h, f, what, tile=None, prev=(None, None), want_grid=True, want_rgb=True):
        a, ga = self.new.render_restir(prev[0], cam, w, h, f, tile=tile, want_grid=want_grid, want_rgb=want_rgb)
        b, gb = self.old.render_restir(prev[1], cam, w, h, f, tile=tile, want_grid=want_grid, want_rgb=want_rgb)
        if not want_rgb:
            tw, th = (tile.width, tile.height) if tile is not None else (w, h)
            a, b = self.new.download_rgb(tw, th), self.old.download_rgb(tw, th)
        assert_bits(a, b, f"{what}: frame {self.n} rgb, look-ahead against frames.ahead=0")
        if want_grid:
            for k, (x, y) in enumerate(zip(ga.download(), gb.download())):
                x, y = np.asarray(x).view(np.float32), np.asarray(y).view(np.float32)
                if tile is not None:   # a tile's ghost ring holds intermediate values: the owned columns (full-height tiles)
                    assert tile.gy0 == tile.y0 and tile.gheight == tile.height
                    x0 = tile.x0 - tile.gx0
                    x, y = x[:, :, x0:x0 + tile.width], y[:, :, x0:x0 + tile.width]
                assert_bits(x, y, f"{what}: frame {self.n} grid plane {k}")
        self.n += 1
        assert self.old.ahead_frames() == 0 and self.old.ahead_discards() == 0
        return ga, gb

    def close(self):
        self.new.close()
        self.old.close()


@pytest.fixture()
def pair():
    from romis_amd import build
    build.build()
    made = []

    def make(sc, **knobs):
        made.append(Pair(sc, **knobs))
        return made[-1]
    yield make
    for p in made:
        p.close()


def run_frames(p, cam, w, h, f, what, n=8, engaged=True, served=True, **kw):
    """Frames 0 .. n - 1 of a still view on both contexts, the counters checked after each"""
    for frame in range(n):
        p.frame(cam, w, h, f, what, **kw)
        assert p.new.ahead_frames() == (max(0, frame - AFTER) if engaged else 0), f"{what}: frame {frame}"
        assert p.new.ahead_discards() == 0, f"{what}: frame {frame}"
        for r in (p.new, p.old):   # as the p-hat tests expect, on both
            assert r.phat_frames() == (max(0, frame - AFTER + 1) if served else 0), f"{what}: frame {frame}"
            assert r.phat_builds() == (1 if frame >= AFTER and served else 0), f"{what}: frame {frame}"


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHTCLUB, "cube_points"])
def test_still_frames_equal_and_counted(pair, name, w, h):
    p = pair(make_scene(name))
    run_frames(p, camera(name, w, h), w, h, features(1), f"{name} {w}x{h}")
    assert p.new.gbuf_reuses() == 7 and p.old.gbuf_reuses() == 7


@pytest.mark.parametrize("knobs", [dict(frames__ahead=2), dict(frames__ahead_prio=1), dict(frames__ahead=2, frames__ahead_prio=1)])
def test_the_other_forms(pair, knobs):
    """RIS enqueued before the last pass (frames.ahead = 2), the second stream at the lowest priority"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB), **knobs)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), str(knobs))


def test_two_passes(pair):
    """Two biased passes: the first reads the look-ahead's handles and pdf cache for every pixel and neighbour"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(2), "two passes")


def test_the_default_engages_after_the_fourth_reusing_frame():
    from romis_amd import build
    build.build()
    w, h = 70, 37
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    r = restir.Renderer(0)
    try:
        r.set_scene(make_scene(NIGHTCLUB))
        r.set_seed(SEED, 0)
        for frame in range(7):
            r.render_restir(None, cam, w, h, f, want_grid=False)
            assert r.ahead_frames() == max(0, frame - 4), f"frame {frame}"
        assert r.ahead_discards() == 0
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------
# what invalidates a result: the next frame equals frames.ahead = 0's, one discard, and the look-ahead comes back
def started(pair, w=70, h=37, M=32):
    sc = make_scene(NIGHTCLUB)
    p = pair(sc)
    cam, f = camera(NIGHTCLUB, w, h), features(1, M=M)
    run_frames(p, cam, w, h, f, "before", n=AFTER + 3)
    assert p.new.ahead_frames() == 2
    return sc, p, cam, f


def after(p, cam, w, h, f, what, discards=1, frames=8):
    """The first frame after the change drops the pending result; within `frames` frames the look-ahead serves again"""
    before = p.new.ahead_frames()
    p.frame(cam, w, h, f, what)
    assert p.new.ahead_discards() == discards, what
    assert p.new.ahead_frames() == before, f"{what}: a stale result was taken"
    for _ in range(frames - 1):
        p.frame(cam, w, h, f, what)
    assert p.new.ahead_discards() == discards, what
    assert p.new.ahead_frames() >= before + 2, f"{what}: the look-ahead did not re-engage"


def test_camera_moved(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    far = scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)
    after(p, far, w, h, f, "far camera")


def test_another_seed(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    p.each(lambda r: r.set_seed(SEED + 1, 6))
    after(p, cam, w, h, f, "another seed")


def test_same_seed_another_frame_index(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    p.each(lambda r: r.set_seed(SEED, 40))
    after(p, cam, w, h, f, "frame index 40")


def test_changed_M(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    after(p, cam, w, h, features(1, M=16), "M = 16")


def test_light_moved(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    moved = [point_light([l.p0[0] + 0.25, l.p0[1], l.p0[2] - 0.5], list(l.c0)) for l in sc.lights]
    p.each(lambda r: r.set_lights(moved))
    after(p, cam, w, h, f, "moved lights")


def test_mesh_moved(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    big = max(range(len(sc.meshes)), key=lambda i: len(sc.meshes[i].positions))
    pos = np.asarray(sc.meshes[big].positions, np.float32) + np.float32([0.125, 0.0, -0.0625])
    p.each(lambda r: r.update_meshes({big: (pos, None)}))
    after(p, cam, w, h, f, "moved mesh", frames=9)


def test_material_changed(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    meshes = [dataclasses.replace(m, kd=np.asarray(m.kd, np.float32) * np.float32(0.5)) for m in sc.meshes]
    other = scene.Scene(meshes, sc.lights, "nightclub_half_kd")
    p.each(lambda r: r.set_scene(other))
    after(p, cam, w, h, f, "materials", frames=9)


def test_launch_shape_knob(pair):
    """A knob that is not one of the cache-keeping ones: the next frame traces, the pending result is dropped"""
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    p.new.set_tuning("ris.late", 0)   # against a context that never touched the knob
    after(p, cam, w, h, f, "ris.late", frames=9)


@pytest.mark.parametrize("key,value", [("timing.mask", -1), ("timing.every", 3), ("frames.ahead_after", 2)])
def test_knob_keeps_the_result(pair, key, value):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    before = p.new.ahead_frames()
    p.new.set_tuning(key, value)
    p.frame(cam, w, h, f, key)
    assert p.new.ahead_frames() == before + 1 and p.new.ahead_discards() == 0, key


# --------------------------------------------------------------------------------------------------------
def test_grid_wanted_on_alternate_frames(pair):
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for frame in range(10):
        p.frame(cam, w, h, f, "alternating grid", want_grid=frame % 2 == 0)
        assert p.new.ahead_frames() == max(0, frame - AFTER) and p.new.ahead_discards() == 0, f"frame {frame}"


def test_images_left_on_the_device(pair):
    """want_rgb = False: nothing waits for the frame; download_rgb reads the last pass's image behind it"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for frame in range(9):
        p.frame(cam, w, h, f, "device image", want_grid=False, want_rgb=False)
    assert p.new.ahead_frames() == 8 - AFTER and p.new.ahead_discards() == 0


@pytest.mark.parametrize("w,h", SIZES[:2])
def test_ghost_ring_tile(pair, w, h):
    """The right-hand tile of a 2 x 1 split: a ghost-zoned view that starts at x0 > 0 and reuses its G-buffer"""
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    tile = restir.tile_plan(w, h, 2, 1, 1, f.spatial_resample_radius)
    assert tile.x0 > 0 and tile.gx0 > 0
    run_frames(p, cam, w, h, f, f"tile {w}x{h}", tile=tile)


def test_temporal_frames_never_look_ahead(pair):
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(2, temporal_reuse=1)
    prev = (None, None)
    for frame in range(8):
        prev = p.frame(cam, w, h, f, "temporal", prev=prev)
    assert p.new.ahead_frames() == 0 and p.new.ahead_discards() == 0
    assert p.new.phat_frames() == 8 - AFTER


def test_M_33_never_looks_ahead(pair):
    """Past the table kernel's candidates: no table, no look-ahead"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1, M=33), "M = 33", engaged=False, served=False)


def test_without_the_table_no_look_ahead(pair):
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB), ris__phat=0)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), "ris.phat = 0", engaged=False, served=False)


def test_close_and_set_scene_with_a_look_ahead_in_flight(pair):
    """close() and set_scene() right behind a frame whose look-ahead may still be running wait for it; the contexts
    that follow render the frames of frames.ahead = 0"""
    w, h = 96, 48
    sc = make_scene(NIGHTCLUB)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    p = pair(sc)
    run_frames(p, cam, w, h, f, "first", n=AFTER + 2)
    p.new.render_restir(None, cam, w, h, f, want_grid=False, want_rgb=False)   # nothing waits for this frame
    p.new.close()
    p.new = restir.Renderer(0)
    for k in ("ris.phat_after", "frames.ahead_after"):
        p.new.set_tuning(k, AFTER)
    p.new.set_scene(sc)
    p.new.set_seed(SEED, 0)
    p.old.set_seed(SEED, 0)
    for _ in range(AFTER + 2):
        p.frame(cam, w, h, f, "after close")
    assert p.new.ahead_frames() == 1
    p.new.render_restir(None, cam, w, h, f, want_grid=False, want_rgb=False)
    p.old.render_restir(None, cam, w, h, f, want_grid=False, want_rgb=False)
    p.each(lambda r: r.set_scene(make_scene("cube_points")))
    assert p.new.ahead_discards() == 1
    cube = camera("cube_points", w, h)
    for _ in range(AFTER + 3):
        p.frame(cube, w, h, f, "after set_scene")
    assert p.new.ahead_frames() == 4 and p.new.ahead_discards() == 1   # two before the new scene, two after


def test_timings_count_every_ris_launch(pair):
    """Every launch timed: eight frames are eight RIS launches and the ninth frame's look-ahead, which synchronize()
    waits for; each frame has one last pass"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    p.new.set_tuning("timing.mask", -1)
    p.new.set_tuning("timing.every", 1)
    p.new.enable_timing(True)
    for frame in range(8):
        p.frame(cam, w, h, f, "timed", want_grid=False)
    p.new.synchronize()
    kt = p.new.timings()
    assert kt["primary_ris"][1] == 9 and kt["spatial"][1] == 8
    assert kt["primary_ris"][0] > 0.0
    assert p.new.ahead_frames() == 7 - AFTER
