"""ris.phat (the default): once a still view's G-buffer is reused for ris.phat_after frames with the lights unchanged,
k_phat_table stores RIS's target pdf of every (pixel, point light) (csrc/phat_table.h), and from that frame on RIS
(k_gbuf_ris_n1_lds_pt_phat) reads its candidates' p-hats from the table instead of evaluating them.  A stored entry is
the return value of the very call the table-free kernel makes, and the running sum is added in the reference's order, so
every frame must equal, bit for bit, the frame of a context with ris.phat = 0 -- no tolerances anywhere in this file.
(Existing tests tie ris.phat = 0 to the oracle.)

Renderer.phat_frames() counts the frames whose RIS read the table, phat_builds() the builds, and debug_phat(light)
returns one light's stored plane (-1 where none is held).

Frame numbers below: frame 0 traces, frame k >= 1 is the k-th reusing frame (the streak); the tests set ris.phat_after
= AFTER = 3, so frames 0-2 run without the table, frame 3 builds it and reads it.  Sizes: 96 x 48 (3 x 6 whole 32 x 8
tiles), 70 x 37 (ragged against the tiles and the 16-pixel steps) and 33 x 9.  Every frame compares the image and the
returned grid (the reservoir planes the last pass wrote from RIS's handles and pdf cache; the cache has no accessor of
its own: test_two_passes_read_the_pdf_cache and the temporal frames run a pass that reads every entry of it).  The kernel
serves M <= 32 and L <= 128; M = 33, 64 and L = 200 check that the route keeps the table-free kernel and builds nothing.
"""
import dataclasses

import numpy as np
import pytest

from romis_amd import _abi, restir, scene
from test_gpu_parity import SEED, assert_bits, get_scene
from test_gpu_shadow_lists import NIGHTCLUB, camera, lights_around, make_scene, point_light

pytestmark = pytest.mark.gpu

AFTER = 3
DEFAULT_AFTER = 4
SIZES = [(96, 48), (70, 37), (33, 9)]


def features(passes=1, M=32, **kw):
    kw.setdefault("temporal_reuse", 0)
    return _abi.default_features(num_samples_in_reservoir=1, spatial_resampling_passes=passes, spatial_reuse=1,
                                 initial_light_samples=M, **kw)


class Pair:
    """Two contexts over one scene: `new` with ris.phat_after = AFTER (None: the default), `old` with ris.phat = 0; frame()
    renders the same frame on both and asserts equal bits."""

    def __init__(self, sc, after=AFTER, **knobs):
        self.new, self.old = restir.Renderer(0), restir.Renderer(0)
        self.old.set_tuning("ris.phat", 0)
        if after is not None:
            self.new.set_tuning("ris.phat_after", after)
        for k, v in knobs.items():
            self.new.set_tuning(k.replace("__", "."), v)
        for r in (self.new, self.old):
            r.set_scene(sc)
            r.set_seed(SEED, 0)
        self.n = 0

    def each(self, fn):
        fn(self.new)
        fn(self.old)

    def frame(self, cam, w, h, f, what, tile=None, prev=(None, None)):
        a, ga = self.new.render_restir(prev[0], cam, w, h, f, tile=tile, want_grid=True)
        b, gb = self.old.render_restir(prev[1], cam, w, h, f, tile=tile, want_grid=True)
        assert_bits(a, b, f"{what}: frame {self.n} rgb, table against ris.phat=0")
        for k, (x, y) in enumerate(zip(ga.download(), gb.download())):
            x, y = np.asarray(x).view(np.float32), np.asarray(y).view(np.float32)
            if tile is not None:   # a tile's ghost ring holds intermediate values: the owned columns (full-height tiles)
                assert tile.gy0 == tile.y0 and tile.gheight == tile.height
                x0 = tile.x0 - tile.gx0
                x, y = x[:, :, x0:x0 + tile.width], y[:, :, x0:x0 + tile.width]
            assert_bits(x, y, f"{what}: frame {self.n} grid plane {k}")
        self.n += 1
        assert self.old.phat_frames() == 0 and self.old.phat_builds() == 0
        return ga, gb

    def close(self):
        self.new.close()
        self.old.close()


@pytest.fixture()
def pair():
    from romis_amd import build
    build.build()
    made = []

    def make(sc, after=AFTER, **knobs):
        made.append(Pair(sc, after, **knobs))
        return made[-1]
    yield make
    for p in made:
        p.close()


def run_frames(p, cam, w, h, f, what, n=AFTER + 3, after=AFTER, served=True, **kw):
    """Frames 0 .. n - 1 of a still view on both contexts, the counters checked after each.  served = False: a shape the
    table's kernel does not take (M > 32 or more than 128 lights) -- no table is built, the frames are the table-free
    kernel's on both contexts"""
    for frame in range(n):
        p.frame(cam, w, h, f, what, **kw)
        assert p.new.phat_frames() == (max(0, frame - after + 1) if served else 0), f"{what}: frame {frame}"
        assert p.new.phat_builds() == (1 if frame >= after and served else 0), f"{what}: frame {frame}"


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHTCLUB, "cube_points"])
def test_still_frames_equal_and_counted(pair, name, w, h):
    """Frames before, at and after ris.phat_after: bit-identical to ris.phat = 0; the counter starts with frame AFTER"""
    p = pair(make_scene(name))
    run_frames(p, camera(name, w, h), w, h, features(1), f"{name} {w}x{h}")
    assert p.new.gbuf_reuses() == AFTER + 2


def test_two_passes_read_the_pdf_cache(pair):
    """Two biased passes: the first reads RIS's pdf cache for every own pixel and neighbour and writes its own for the
    second, so a cache entry that differed from the table-free kernel's would show in the grid"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(2), "two passes")


def test_the_default_builds_with_the_fourth_reusing_frame(pair):
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB), after=None)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), "default", n=DEFAULT_AFTER + 2, after=DEFAULT_AFTER)


@pytest.mark.parametrize("M", [1, 5, 32, 33, 64])
def test_candidate_counts(pair, M):
    """M smaller than the four lanes of a pixel (1), ragged last chunks (5: chunks of 2, 2, 1, 0), whole chunks (32); 33 and
    64 are past the kernel's eight candidates a lane: the route keeps the table-free kernel and builds nothing"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1, M=M), f"M = {M}", served=M <= 32)


def mixed_materials(base):
    """Every other mesh of the scene specular (ks > 0, powf evaluated), the others ks = 0: both kinds in most tiles"""
    meshes = []
    for i, m in enumerate(base.meshes):
        ks = np.float32([0.7, 0.6, 0.5]) if i % 2 == 0 else np.float32([0.0, 0.0, 0.0])
        meshes.append(dataclasses.replace(m, ks=ks, shininess=np.float32(17.0 if i % 2 == 0 else m.shininess)))
    return meshes


@pytest.mark.parametrize("n", [1, 33, 128, 200])
def test_light_counts(pair, n):
    """1, 33, 128 and 200 point lights around the nightclub's geometry (row padding, a non-power-of-two uniform_index; 200
    is past the kernel's 128: no table), over materials with and without a specular term in one tile"""
    w, h = 70, 37
    base = get_scene(NIGHTCLUB)
    sc = scene.Scene(mixed_materials(base), lights_around(base, n - 1, 11 + n, radius=0.3), f"nightclub_mixed_{n}pt")
    assert len(sc.lights) == n
    p = pair(sc)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), f"{n} lights", served=n <= 128)
    if n <= 128:
        assert (p.new.debug_phat(n - 1, w, h) >= 0).any()


FLT_MIN = np.float32(1.17549435e-38)


@pytest.mark.parametrize("name,w,h", [(NIGHTCLUB, 70, 37), ("cube_points", 70, 37)])
def test_every_stored_entry_equals_the_table_free_p_hat(pair, name, w, h):
    """Some lights' planes against the table-free path's own p-hat: a scene holding only that light, M = 1, through the
    stage API (k_primary, k_ris).  Its one candidate draws that light with weight w = p-hat x 1, so the reservoir's wsum is
    FLT_MIN + p-hat at every pixel, and its chosen weight is the p-hat wherever the candidate was accepted."""
    sc = make_scene(name)
    p = pair(sc)
    cam = camera(name, w, h)
    run_frames(p, cam, w, h, features(1), name, n=AFTER + 1)
    L = len(sc.lights)
    lights = sorted({0, L // 3, L - 1})
    none = None
    held_n = took_n = 0
    ref = restir.Renderer(0)
    try:
        for i in lights:
            plane = p.new.debug_phat(i, w, h)
            held = plane >= 0
            assert none is None or np.array_equal(none, ~held), "another set of pixels holds entries"
            none = ~held
            assert (plane[~held] == -1).all() and held.any()
            ref.set_scene(scene.Scene(sc.meshes, [sc.lights[i]], f"{name}_only_{i}"))
            ref.stage_configure(w, h, 1)
            ref.stage_primary(cam)
            ref.stage_ris(cam, features(0, M=1), 12345, debug=True)
            dbg = ref.download(_abi.BUF_RES_DBG).reshape(h, w, 2)
            wsum, chosen = dbg[..., 0], dbg[..., 1]
            assert_bits((FLT_MIN + plane)[held], wsum[held], f"{name} light {i}: FLT_MIN + stored p-hat against wsum")
            took = held & (chosen > 0)
            held_n += int(held.sum())
            took_n += int(took.sum())
            assert_bits(plane[took], chosen[took], f"{name} light {i}: stored p-hat against the accepted weight")
            assert (chosen[held & ~took] == 0).all() and (plane[held & ~took] < 1e-30).all()
    finally:
        ref.close()
    assert took_n > 0, "the comparison is not vacuous"   # (a light behind a surface has p-hat 0 there)
    with pytest.raises(_abi.RestirError, match=r"restir_debug_phat: INVALID: .*light"):
        p.new.debug_phat(L, w, h)
    with pytest.raises(_abi.RestirError, match=r"restir_debug_phat: INVALID: .*pixels"):
        p.new.debug_phat(0, w + 1, h)


def test_debug_entry_needs_a_table(pair):
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), "no table yet", n=AFTER)
    with pytest.raises(_abi.RestirError, match=r"restir_debug_phat: STATE: .*no p-hat table"):
        p.new.debug_phat(0, w, h)


@pytest.mark.parametrize("w,h", SIZES[:2])
def test_tile_with_an_origin(pair, w, h):
    """The right-hand tile of a 2 x 1 split: a ghost-zoned view that starts at x0 > 0"""
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    tile = restir.tile_plan(w, h, 2, 1, 1, f.spatial_resample_radius)
    assert tile.x0 > 0 and tile.gx0 > 0
    run_frames(p, cam, w, h, f, f"tile {w}x{h}", tile=tile)
    assert (p.new.debug_phat(5, tile.gwidth, tile.gheight) >= 0).any()


def test_far_camera_background_tiles_hold_no_entries(pair):
    w, h = 96, 48
    p = pair(make_scene(NIGHTCLUB))
    far = scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)   # background tiles too
    run_frames(p, far, w, h, features(1), "far camera")
    plane = p.new.debug_phat(9, w, h)
    assert (plane >= 0).any() and (plane == -1).any()
    # a 32 x 8 tile without a held pixel exists: its rows are neither written nor read
    tiles = (plane >= 0).reshape(h // 8, 8, w // 32, 32).any(axis=(1, 3))
    assert (~tiles).any()


def test_camera_that_sees_only_background(pair):
    """Every tile is background: the build and the frames touch no row, and the frames are equal"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    away = scene.make_camera(5.0, 10.0, (400.0, 300.0, -200.0), (10.3, 30.0, 0.0), w, h)
    for frame in range(AFTER + 2):
        p.frame(away, w, h, features(1), "background only")
    bg, computed = p.new.background_pixels()
    assert bg == computed == w * h, "the camera was meant to miss the scene"


@pytest.mark.parametrize("w,h", SIZES[:2])
def test_temporal_frames_thread_the_grid(pair, w, h):
    """C3's shape: two passes, temporal reuse, the grid threaded through eight frames.  Frame 0 has no predecessor and
    traces; frames 1 .. 7 reuse the G-buffer under k_gbuf_ris_n1_lds_pt_temporal, from frame AFTER on under
    k_gbuf_ris_n1_lds_pt_phat_temporal, which reads the table on every one of them"""
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(2, temporal_reuse=1)
    prev = (None, None)
    for frame in range(8):
        prev = p.frame(cam, w, h, f, f"temporal {w}x{h}", prev=prev)
        assert p.new.phat_frames() == max(0, frame - AFTER + 1), f"frame {frame}"
        assert p.new.phat_builds() == (1 if frame >= AFTER else 0), f"frame {frame}"
    assert p.new.gbuf_reuses() == 7
    assert (p.new.debug_phat(3, w, h) >= 0).any()


# --------------------------------------------------------------------------------------------------------
# what drops the table: each stops the table's frames and the right later frame builds it again
def after(p, cam, w, h, f, what, counts):
    """Frames after an event; counts: phat_frames expected after each"""
    for k, want in enumerate(counts):
        p.frame(cam, w, h, f, what)
        assert p.new.phat_frames() == want, f"{what}: frame {k} after"


def started(pair, w=70, h=37):
    sc = make_scene(NIGHTCLUB)
    p = pair(sc)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    run_frames(p, cam, w, h, f, "before", n=AFTER + 2)
    assert p.new.phat_frames() == 2 and p.new.phat_builds() == 1
    return sc, p, cam, f


def test_lights_set_between_frames(pair):
    """restir_set_lights keeps the G-buffer and restarts the streak: reusing frames 1-2 without the table, the third builds"""
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    moved = [point_light([l.p0[0] + 0.25, l.p0[1], l.p0[2] - 0.5], list(l.c0)) for l in sc.lights]
    p.each(lambda r: r.set_lights(moved))
    after(p, cam, w, h, f, "moved lights", [2, 2, 3, 4])
    assert p.new.phat_builds() == 2


def test_meshes_updated_between_frames(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    big = max(range(len(sc.meshes)), key=lambda i: len(sc.meshes[i].positions))
    pos = np.asarray(sc.meshes[big].positions, np.float32) + np.float32([0.125, 0.0, -0.0625])
    p.each(lambda r: r.update_meshes({big: (pos, None)}))
    after(p, cam, w, h, f, "moved mesh", [2, 2, 2, 3, 4])   # a tracing frame first
    assert p.new.phat_builds() == 2


def test_camera_changed_between_frames(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    far = scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)
    after(p, far, w, h, f, "far camera", [2, 2, 2, 3, 4])
    assert p.new.phat_builds() == 2


def test_scene_set_again(pair):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    p.each(lambda r: r.set_scene(sc))
    with pytest.raises(_abi.RestirError, match=r"restir_debug_phat: STATE"):
        p.new.debug_phat(0, w, h)
    after(p, cam, w, h, f, "scene again", [2, 2, 2, 3, 4])
    assert p.new.phat_builds() == 2


def test_ris_phat_off_and_on_again(pair):
    """ris.phat = 0 frees the table (and, as any launch-shape knob, makes the next frame trace); switched on again the
    table comes back with the third reusing frame"""
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    p.new.set_tuning("ris.phat", 0)
    with pytest.raises(_abi.RestirError, match=r"restir_debug_phat: STATE"):
        p.new.debug_phat(0, w, h)
    after(p, cam, w, h, f, "phat off", [2, 2, 2, 2, 2])
    assert p.new.phat_builds() == 1
    p.new.set_tuning("ris.phat", 1)
    after(p, cam, w, h, f, "phat on again", [2, 2, 2, 3, 4])
    assert p.new.phat_builds() == 2


@pytest.mark.parametrize("key,value", [("timing.mask", -1), ("timing.every", 3), ("timing.fence", 1), ("ris.phat_after", 2)])
def test_knob_keeps_the_table(pair, key, value):
    w, h = 70, 37
    sc, p, cam, f = started(pair)
    r = p.new
    before = (r.gbuf_reuses(), r.phat_frames())
    r.set_tuning(key, value)
    p.frame(cam, w, h, f, key)   # against a context that never touched the knob
    assert (r.gbuf_reuses(), r.phat_frames()) == tuple(x + 1 for x in before), key
    assert r.phat_builds() == 1, f"{key}: the table was built again"


def test_a_table_over_the_size_cap_is_not_built(pair):
    """ris.phat_max_mb = 1: 70 x 37 with 128 lights needs 1.9 MB -- no build, no error, equal frames"""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB), ris__phat_max_mb=1)
    for frame in range(AFTER + 3):
        p.frame(camera(NIGHTCLUB, w, h), w, h, features(1), "capped")
    assert p.new.phat_frames() == 0 and p.new.phat_builds() == 0
    assert p.new.gbuf_reuses() == AFTER + 2
