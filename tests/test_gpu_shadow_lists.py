"""final.lists (the default): from the second consecutive frame that reuses the kept G-buffer with the lights unchanged,
the fused last pass (k_spatial1hg_t2_final_lists) traces each shadow ray over the candidate triangles of (its 32 x 16
tile, its light) -- records k_shadow_lists builds once per still view and light set (csrc/shadow_lists.h) -- instead of
staging the BVH, binning the rays and walking it.  A ray is still traced with the same triangle test, so every frame must
equal, bit for bit, the frame of a context that never uses the lists (final.lists = 0).

Renderer.shadow_list_frames() counts the frames that took the lists; Renderer.debug_shadow_lists(light) traces, for every
pixel of the kept G-buffer, the ray to one light by the BVH walk and over the pixel's list.

Sizes: 96 x 48 (3 x 3 tiles of 32 x 16) and the ragged 70 x 37 (3 x 3, the last column 6 wide, the last row 5 high);
the right-hand tile of a 2 x 1 split gives the pass's rect a non-zero origin.
"""
import numpy as np
import pytest

from romis_amd import _abi, restir, scene
from test_gpu_parity import SEED, assert_bits, get_scene

pytestmark = pytest.mark.gpu

NIGHTCLUB = "nightclub_128pt"
SIZES = [(96, 48), (70, 37)]


def point_light(p, c):
    l = _abi.Light(type=_abi.LIGHT_POINT)
    l.p0[:], l.c0[:] = [float(x) for x in p], [float(x) for x in c]
    return l


def lights_around(sc, n, seed, radius=1.2):
    """n point lights on a shell around the scene's bounds, and one at their centre (inside a closed mesh)"""
    pts = np.concatenate([np.asarray(m.positions, np.float32) for m in sc.meshes])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    c, r = (lo + hi) / 2, float((hi - lo).max())
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    pos = np.concatenate([c + radius * r * d / np.linalg.norm(d, axis=1, keepdims=True), c[None]])
    return [point_light(p, rng.uniform(0.5, 4.0, 3)) for p in pos]


_made = {}


def make_scene(name):
    if name not in _made:
        if name == "cube_points":
            base = scene.load_prebuilt("Cube")
            _made[name] = scene.Scene(base.meshes, lights_around(base, 15, 3), name)
        elif name == "nightclub_sheet":   # 166 + 128 triangles: no one-byte indices, the BVH kernel stays
            base = get_scene(NIGHTCLUB)
            n = 8   # a sheet of 8 x 8 quads in front of the camera's target
            g = np.stack(np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
            pos = np.concatenate([2.0 + g[:, :1] / n, np.full((len(g), 1), 1.0, np.float32), -2.0 + g[:, 1:] / n], axis=1)
            q = np.asarray([[i * (n + 1) + j for j in range(n)] for i in range(n)]).reshape(-1)
            tri = np.concatenate([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)]).astype(np.uint32)
            m0 = base.meshes[0]
            sheet = scene.MeshData(pos.astype(np.float32), np.tile(np.float32([0, 1, 0]), (len(pos), 1)), tri, m0.kd, m0.ks,
                                   m0.shininess, m0.transparency, name="sheet")
            _made[name] = scene.Scene(list(base.meshes) + [sheet], base.lights, name)
        else:
            _made[name] = get_scene(name)
    return _made[name]


def camera(name, w, h):
    return scene.camera_for(NIGHTCLUB if name == NIGHTCLUB else "Cube", w, h)


def features(passes=1, **kw):
    kw.setdefault("temporal_reuse", 0)
    return _abi.default_features(num_samples_in_reservoir=1, spatial_resampling_passes=passes, spatial_reuse=1, **kw)


class Pair:
    """Two contexts over one scene: `new` with the default knobs, `old` with final.lists = 0; frame() renders the same
    frame on both and asserts equal bits."""

    def __init__(self, sc, cap=None):
        self.new, self.old = restir.Renderer(0), restir.Renderer(0)
        self.old.set_tuning("final.lists", 0)
        if cap is not None:
            self.new.set_tuning("final.lists_cap", cap)
        for r in (self.new, self.old):
            r.set_scene(sc)
            r.set_seed(SEED, 0)
        self.n = 0

    def each(self, fn):
        fn(self.new)
        fn(self.old)

    def frame(self, cam, w, h, f, what, tile=None, want_grid=False, prev=(None, None)):
        a, ga = self.new.render_restir(prev[0], cam, w, h, f, tile=tile, want_grid=want_grid)
        b, gb = self.old.render_restir(prev[1], cam, w, h, f, tile=tile, want_grid=want_grid)
        assert_bits(a, b, f"{what}: frame {self.n} rgb, lists against final.lists=0")
        if want_grid:
            for k, (x, y) in enumerate(zip(ga.download(), gb.download())):
                assert_bits(np.asarray(x).view(np.float32), np.asarray(y).view(np.float32), f"{what}: frame {self.n} grid plane {k}")
        self.n += 1
        assert self.old.shadow_list_frames() == 0
        return ga, gb

    def close(self):
        self.new.close()
        self.old.close()


@pytest.fixture()
def pair():
    from romis_amd import build
    build.build()
    made = []

    def make(sc, cap=None):
        made.append(Pair(sc, cap))
        return made[-1]
    yield make
    for p in made:
        p.close()


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHTCLUB, "cube_points"])
def test_still_frames_equal_and_counted(pair, name, w, h):
    """Frames 0-3 of a still camera: bit-identical to final.lists = 0, the counter reads 0, 0, 1, 2."""
    p = pair(make_scene(name))
    cam, f = camera(name, w, h), features(1)
    for frame, want in enumerate([0, 0, 1, 2]):
        p.frame(cam, w, h, f, f"{name} {w}x{h}")
        assert p.new.shadow_list_frames() == want, f"frame {frame}"
        assert p.new.gbuf_reuses() == frame


@pytest.mark.parametrize("w,h", SIZES)
def test_tile_with_an_origin(pair, w, h):
    """The right-hand tile of a 2 x 1 split: the pass's rect starts at x0 > 0 inside a ghost-zoned view."""
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    tile = restir.tile_plan(w, h, 2, 1, 1, f.spatial_resample_radius)
    assert tile.x0 > 0
    for frame, want in enumerate([0, 0, 1, 2]):
        p.frame(cam, w, h, f, f"tile {w}x{h}", tile=tile)
        assert p.new.shadow_list_frames() == want, f"frame {frame}"
    for light in (0, 77, 128):
        a, b = p.new.debug_shadow_lists(light, tile.width, tile.height)
        assert np.array_equal(a, b), f"light {light}: {(a != b).sum()} rays differ"


@pytest.mark.parametrize("name,w,h", [(NIGHTCLUB, 96, 48), (NIGHTCLUB, 70, 37), ("cube_points", 70, 37)])
def test_every_ray_over_its_list_equals_the_walk(pair, name, w, h):
    """The debug entry's two planes for every light (and the zero sample): at 96 x 48, 129 x 4,608 rays."""
    sc = make_scene(name)
    p = pair(sc)
    cam, f = camera(name, w, h), features(1)
    for _ in range(3):
        p.frame(cam, w, h, f, name)
    assert p.new.shadow_list_frames() == 1
    occluded = traced = 0
    for light in range(len(sc.lights) + 1):
        a, b = p.new.debug_shadow_lists(light, w, h)
        assert np.array_equal(a, b), f"light {light}: {(a != b).sum()} of {a.size} rays differ"
        traced += int((a != 0xFF).sum())
        occluded += int((a == 0).sum())
    assert traced > 0 and 0 < occluded < traced   # both answers occur: the comparison is not vacuous


def test_debug_entry_refuses_what_it_cannot_answer(pair):
    """Before a frame has built lists the entry reports RESTIR_ERR_STATE; once there are lists, planes of another size
    than the lists' rectangle, or a light past the zero sample, RESTIR_ERR_INVALID -- it writes nothing then."""
    p = pair(make_scene(NIGHTCLUB))
    w, h = 70, 37
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    p.frame(cam, w, h, f, "one frame")   # the G-buffer is kept, no lists yet
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_lists: STATE: .*no shadow lists"):
        p.new.debug_shadow_lists(0, w, h)
    p.frame(cam, w, h, f, "two")
    p.frame(cam, w, h, f, "three")
    assert p.new.shadow_list_frames() == 1
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_lists: INVALID: .*70 x 37"):
        p.new.debug_shadow_lists(0, w + 1, h)
    with pytest.raises(_abi.RestirError, match=r"restir_debug_shadow_lists: INVALID: .*light 130"):
        p.new.debug_shadow_lists(130, w, h)
    a, b = p.new.debug_shadow_lists(128, w, h)
    assert np.array_equal(a, b)


def test_lists_after_knob_delays_the_build(pair):
    """final.lists_after = 4: the lists come with the fourth consecutive reusing frame instead of the second."""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    p.new.set_tuning("final.lists_after", 4)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for frame, want in enumerate([0, 0, 0, 0, 1, 2]):
        p.frame(cam, w, h, f, "lists_after 4")
        assert p.new.shadow_list_frames() == want, f"frame {frame}"


@pytest.mark.parametrize("cap", [1, 3])
def test_short_records_walk_per_ray(pair, cap):
    """final.lists_cap (a test knob): records of at most `cap` indices, every longer list says "walk the BVH"; blocks
    then mix rays over lists with rays that walk."""
    w, h = 96, 48
    p = pair(make_scene(NIGHTCLUB), cap=cap)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for frame, want in enumerate([0, 0, 1, 2]):
        p.frame(cam, w, h, f, f"cap {cap}")
        assert p.new.shadow_list_frames() == want
    for light in (0, 31, 64, 127, 128):
        a, b = p.new.debug_shadow_lists(light, w, h)
        assert np.array_equal(a, b), f"cap {cap} light {light}: {(a != b).sum()} rays differ"


def test_more_than_256_triangles_keeps_the_bvh_kernel(pair):
    w, h = 70, 37
    sc = make_scene("nightclub_sheet")
    assert 256 < sc.num_triangles < 400   # (the BVH still fits the LDS budget: the fused kernels run)
    p = pair(sc)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for _ in range(4):
        p.frame(cam, w, h, f, "sheet")
    assert p.new.gbuf_reuses() == 3 and p.new.shadow_list_frames() == 0


# --------------------------------------------------------------------------------------------------------
# what drops the lists
def test_lights_set_between_frames(pair):
    """restir_set_lights keeps the G-buffer and drops the lists: the next frame reuses the G-buffer without lists (the
    first frame of the new lights), the one after builds them again."""
    w, h = 70, 37
    sc = make_scene(NIGHTCLUB)
    p = pair(sc)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for _ in range(3):
        p.frame(cam, w, h, f, "before")
    assert p.new.shadow_list_frames() == 1
    moved = [point_light([l.p0[0] + 0.25, l.p0[1], l.p0[2] - 0.5], list(l.c0)) for l in sc.lights]
    p.each(lambda r: r.set_lights(moved))
    for want in (1, 2, 3):
        p.frame(cam, w, h, f, "moved lights")
        assert p.new.shadow_list_frames() == want
    for light in (0, 100):
        a, b = p.new.debug_shadow_lists(light, w, h)
        assert np.array_equal(a, b)
    # lights that move every frame never build lists
    before = p.new.shadow_list_frames()
    for k in range(3):
        p.each(lambda r: r.set_lights(sc.lights if k % 2 else moved))
        p.frame(cam, w, h, f, "lights every frame")
    assert p.new.shadow_list_frames() == before


def test_meshes_updated_between_frames(pair):
    w, h = 70, 37
    sc = make_scene(NIGHTCLUB)
    p = pair(sc)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for _ in range(3):
        p.frame(cam, w, h, f, "before")
    assert p.new.shadow_list_frames() == 1
    big = max(range(len(sc.meshes)), key=lambda i: len(sc.meshes[i].positions))
    pos = np.asarray(sc.meshes[big].positions, np.float32) + np.float32([0.125, 0.0, -0.0625])
    p.each(lambda r: r.update_meshes({big: (pos, None)}))
    # a tracing frame, the first reusing frame, then the lists again
    for want in (1, 1, 2, 3):
        p.frame(cam, w, h, f, "moved mesh")
        assert p.new.shadow_list_frames() == want
    a, b = p.new.debug_shadow_lists(5, w, h)
    assert np.array_equal(a, b)


def test_camera_changed_between_frames(pair):
    w, h = 96, 48
    p = pair(make_scene(NIGHTCLUB))
    f = features(1)
    cam = camera(NIGHTCLUB, w, h)
    far = scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)   # background tiles too
    for _ in range(3):
        p.frame(cam, w, h, f, "before")
    assert p.new.shadow_list_frames() == 1
    for want in (1, 1, 2, 3):
        p.frame(far, w, h, f, "far camera")
        assert p.new.shadow_list_frames() == want
    a, b = p.new.debug_shadow_lists(9, w, h)
    assert np.array_equal(a, b) and (a == 0xFF).any()   # the far view has background tiles


def test_kept_grid_with_temporal_reuse(pair):
    """C3's shape: temporal reuse with the grid kept; the fused last pass then also stores the returned grid."""
    w, h = 70, 37
    p = pair(make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(2, temporal_reuse=1)
    prev = (None, None)
    for frame in range(4):
        prev = p.frame(cam, w, h, f, "temporal", want_grid=True, prev=prev)
    assert p.new.shadow_list_frames() == 2
