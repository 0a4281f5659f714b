"""gbuf.reuse (the default): a context keeps the G-buffer and the tile flags of the last view restir_render traced, and
a frame of the same view -- scene upload, camera, image size, tile -- runs the k_gbuf_ris family over them instead of
tracing its primary rays again.  The kept records are the values the frame's own primary rays would produce, so every
frame must equal the oracle's frame of its (seed, frame index) bit for bit, RGB and the returned grid; where the oracle
helper does not cover a path (a ghost-zoned tile) the frame of a fresh context that always traces (gbuf.reuse = 0)
stands in.  Renderer.gbuf_reuses() counts the frames that took the reuse kernels (both kinds are timed under
RESTIR_K_PRIMARY_RIS, so the launch counters cannot tell them apart).

Everything else that writes those buffers, or changes what a frame would leave in them, must make the next frame trace:
each such event happens here between two frames of one context.

Sizes 70 x 37 and 96 x 40: 3 x 5 tiles of 32 x 8, ragged in both axes at 70 x 37 and in y at 96 x 40.  Of the 15 tiles
(CPU oracle primary rays) the far nightclub camera leaves 10 all background, the default one 1 (9 / 12 mixed), the
Cornell TOML camera 9 / 12, the framed Cornell camera none.
"""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

from romis_amd import _abi, scene
from test_gpu_fused_final import same_grid, same_rgb
from test_gpu_parity import SEED, assert_bits, assert_grid, get_scene

pytestmark = pytest.mark.gpu

NIGHTCLUB, CORNELL, TEX = "nightclub_128pt", "cornell_1024", "CubeTextured"
SIZES = [(70, 37), (96, 40)]


def camera(view, w, h):
    if view == "nightclub_far":   # pulled back: two thirds of the tiles see only background
        return scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)
    if view == "cornell_framed":  # inside the box: no background tile
        return scene.cornell_framed_camera(w, h)
    return scene.camera_for(NIGHTCLUB if view.startswith("nightclub") else CORNELL, w, h)


VIEWS = {"nightclub_far": NIGHTCLUB, "nightclub_in": NIGHTCLUB, "cornell_toml": CORNELL, "cornell_framed": CORNELL}


@pytest.fixture()
def gpu():
    """A context of its own per test: what it keeps from one frame to the next is the subject."""
    from romis_amd import build, restir
    build.build()
    r = restir.Renderer(0)
    yield r
    r.close()


def features(passes=1, N=1, **kw):
    kw.setdefault("temporal_reuse", 0)
    return _abi.default_features(num_samples_in_reservoir=N, spatial_resampling_passes=passes,
                                 spatial_reuse=1 if passes else 0, **kw)


def fresh_frame(s, cam, w, h, f, frame, tile=None):
    """Frame `frame` of a new context that never reuses: (rgb, grid planes)."""
    from romis_amd import restir
    r = restir.Renderer(0)
    try:
        r.set_tuning("gbuf.reuse", 0)
        r.set_scene(s)
        r.set_seed(SEED, frame)
        rgb, grid = r.render_restir(None, cam, w, h, f, tile=tile)
        planes = [np.asarray(a) for a in grid.download()]
        assert r.gbuf_reuses() == 0
    finally:
        r.close()
    return rgb, planes


def check_frame(gpu, oracle, osc, cam, w, h, f, frame, what, prev=(None, None), want_grid=True):
    """Render the context's next frame (index `frame`) and compare it with the oracle's; returns (grid, oracle grid)."""
    rgb, grid = gpu.render_restir(prev[0], cam, w, h, f, want_grid=want_grid)
    want, res, _ = oracle.render_frame(osc, cam, f, w, h, SEED, frame, prev=prev[1])
    assert_bits(rgb, want, f"{what} frame {frame} rgb")
    if want_grid:
        assert_grid(grid, res, f"{what} frame {frame}")
    return grid, res


# --------------------------------------------------------------------------------------------------------
# a static view
@pytest.mark.parametrize("passes", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("view", ["nightclub_far", "nightclub_in", "cornell_toml"])
def test_static_view_frames_match_oracle(gpu, oracle, view, w, h, N, passes):
    """Four frames of one camera: frames 1-3 take the reuse kernel (without and with a returned grid), each equals the
    oracle's."""
    s = get_scene(VIEWS[view])
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam = camera(view, w, h)
    f = features(passes, N)
    gpu.set_seed(SEED, 0)
    for frame in range(4):
        check_frame(gpu, oracle, osc, cam, w, h, f, frame, f"{view} {w}x{h} N={N} passes={passes}",
                    want_grid=frame != 2)
        assert gpu.gbuf_reuses() == frame, f"frame {frame}: {gpu.gbuf_reuses()} reusing frames so far"
    bg, px = gpu.background_pixels()   # the flags a reusing frame read are the tracing frame's
    assert px == w * h and (bg > 0 or view == "nightclub_in")


def test_static_view_background_pixels_unchanged(gpu):
    """restir_background_pixels after a reusing frame counts what it counted after the tracing frame."""
    w, h = 96, 40
    gpu.set_scene(get_scene(NIGHTCLUB))
    cam, f = camera("nightclub_far", w, h), features(1)
    gpu.render_restir(None, cam, w, h, f, want_grid=False)
    first = gpu.background_pixels()
    gpu.render_restir(None, cam, w, h, f, want_grid=False)
    assert gpu.gbuf_reuses() == 1
    assert gpu.background_pixels() == first and 0 < first[0] < first[1] == w * h


@pytest.mark.parametrize("w,h", SIZES)
def test_static_view_unbiased_and_framed(gpu, oracle, w, h):
    """The framed Cornell camera (no background tile) through a single unbiased pass with visibility reuse, whose
    tracing frame skips nothing here, then the TOML camera, whose tracing frame also skips background tiles' G-buffer
    records (skip bit 1) and whose reusing frames skip them again."""
    s = get_scene(CORNELL)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    f = features(1, unbiased_combination=1, spatial_reuse_visibility_check=1)
    gpu.set_seed(SEED, 0)
    frame = 0
    for view in ("cornell_framed", "cornell_toml"):
        before = gpu.gbuf_reuses()
        for k in range(3):
            check_frame(gpu, oracle, osc, camera(view, w, h), w, h, f, frame, f"{view} unbiased {w}x{h}")
            frame += 1
            assert gpu.gbuf_reuses() == before + k


# --------------------------------------------------------------------------------------------------------
# temporal reuse: the grid threaded through four frames
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("w,h", SIZES)
def test_temporal_frames_match_oracle(gpu, oracle, w, h, N):
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam = camera("nightclub_far", w, h)
    f = features(2, N, temporal_reuse=1)
    gpu.set_seed(SEED, 0)
    prev = (None, None)
    for frame in range(4):
        prev = check_frame(gpu, oracle, osc, cam, w, h, f, frame, f"temporal {w}x{h} N={N}", prev=prev)
        assert gpu.gbuf_reuses() == frame, f"frame {frame}: {gpu.gbuf_reuses()} reusing frames so far"


# --------------------------------------------------------------------------------------------------------
# invalidation: frame 0 of a view, an event, then frame 1
W0, H0 = 70, 37


def derived(cam):
    fr = _abi.CameraFrame()
    _abi.load_library().restir_camera_derive(C.byref(cam), C.byref(fr))
    return bytes(fr)


@pytest.mark.parametrize("field", ["distance", "look_at", "fovy"])
def test_camera_moved_by_one_ulp(gpu, oracle, field):
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam, f = camera("nightclub_far", W0, H0), features(1)
    gpu.set_seed(SEED, 0)
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 0, "before")
    cam2 = _abi.Camera.from_buffer_copy(cam)
    if field == "look_at":
        cam2.look_at[1] = float(np.nextafter(np.float32(cam.look_at[1]), np.float32(np.inf)))
    else:
        setattr(cam2, field, float(np.nextafter(np.float32(getattr(cam, field)), np.float32(np.inf))))
    check_frame(gpu, oracle, osc, cam2, W0, H0, f, 1, f"{field} + 1 ulp")
    if derived(cam2) != derived(cam):   # (a derived camera equal in every bit is the same view)
        assert gpu.gbuf_reuses() == 0
    check_frame(gpu, oracle, osc, cam2, W0, H0, f, 2, f"{field} + 1 ulp, again")
    assert gpu.gbuf_reuses() >= 1


def test_scene_changed_in_one_triangle(gpu, oracle):
    s = get_scene(NIGHTCLUB)
    s2 = scene.Scene([copy.deepcopy(m) for m in s.meshes], s.lights, s.name)
    big = max(range(len(s2.meshes)), key=lambda i: len(s2.meshes[i].triangles))
    tri = s2.meshes[big].triangles[0]
    s2.meshes[big].positions[tri[0]] += np.float32(0.25)   # one vertex of one triangle
    cam, f = camera("nightclub_in", W0, H0), features(1)
    gpu.set_scene(s)
    gpu.set_seed(SEED, 0)
    check_frame(gpu, oracle, oracle.OracleScene(s), cam, W0, H0, f, 0, "before")
    gpu.set_scene(s2)
    check_frame(gpu, oracle, oracle.OracleScene(s2), cam, W0, H0, f, 1, "changed scene")
    assert gpu.gbuf_reuses() == 0
    gpu.set_scene(s2)   # the same scene uploaded again is another upload
    check_frame(gpu, oracle, oracle.OracleScene(s2), cam, W0, H0, f, 2, "uploaded again")
    assert gpu.gbuf_reuses() == 0


def test_image_size_changed(gpu, oracle):
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    f = features(1)
    gpu.set_seed(SEED, 0)
    frame = 0
    for w, h in [(70, 37), (96, 40), (70, 37), (70, 38)]:
        check_frame(gpu, oracle, osc, camera("nightclub_far", w, h), w, h, f, frame, f"{w}x{h}")
        frame += 1
    assert gpu.gbuf_reuses() == 0


@pytest.mark.parametrize("passes", [1, 2])
def test_tile_region_changed(gpu, oracle, passes):
    """A ghost-zoned tile (rank 1 of 2 x 1), then the whole image, then the tile twice: only the last frame reuses."""
    from romis_amd import restir
    w, h = 96, 40
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    cam, f = camera("nightclub_far", w, h), features(passes)
    tile = restir.tile_plan(w, h, 2, 1, 1, passes * f.spatial_resample_radius)
    gpu.set_seed(SEED, 0)
    for frame, t in enumerate([tile, None, tile, tile]):
        rgb, grid = gpu.render_restir(None, cam, w, h, f, tile=t)
        want, planes = fresh_frame(s, cam, w, h, f, frame, tile=t)
        same_rgb(rgb, want, f"frame {frame} rgb")
        same_grid([np.asarray(a) for a in grid.download()], planes, f"frame {frame}", t)
        assert gpu.gbuf_reuses() == (1 if frame == 3 else 0)
    want, _, _ = oracle.render_frame(oracle.OracleScene(s), cam, f, w, h, SEED, 1)
    rgb1, _ = fresh_frame(s, cam, w, h, f, 1)
    assert_bits(rgb1, want, "the fresh context's whole frame against the oracle")


def test_texture_mapping_toggled(gpu, oracle):
    s = get_scene(TEX)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam = scene.camera_for(TEX, W0, H0)
    gpu.set_seed(SEED, 0)
    for frame, tex in enumerate([1, 0, 0, 1]):
        check_frame(gpu, oracle, osc, cam, W0, H0, features(1, enable_texture_mapping=tex), frame, f"texture={tex}")
        assert gpu.gbuf_reuses() == (1 if frame >= 2 else 0)


def test_stage_primary_between_frames(gpu, oracle):
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam, f = camera("nightclub_far", W0, H0), features(1)
    gpu.set_seed(SEED, 0)
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 0, "before")
    gpu.stage_configure(W0, H0, 1)
    gpu.stage_primary(camera("nightclub_in", W0, H0))   # another view into the same planes
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 1, "after stage_primary")
    assert gpu.gbuf_reuses() == 0


def test_halo_frame_between_frames(gpu, oracle):
    from romis_amd import restir
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam, f = camera("nightclub_far", W0, H0), features(1)
    gpu.set_seed(SEED, 0)
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 0, "before")
    tile = restir.tile_plan(W0, H0, 1, 1, 0, f.spatial_resample_radius)
    gpu.halo_begin(None, camera("nightclub_in", W0, H0), W0, H0, f, (1, 1), 0)   # frame index 1, another view
    gpu.halo_spatial()
    gpu.halo_end(tile, want_rgb=False, want_grid=False)
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 2, "after a halo frame")
    assert gpu.gbuf_reuses() == 0


def test_records_layout_never_reuses(gpu, oracle):
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam, f = camera("nightclub_far", W0, H0), features(1)
    gpu.set_tuning("layout.records", 1)
    gpu.set_seed(SEED, 0)
    for frame in range(3):
        check_frame(gpu, oracle, osc, cam, W0, H0, f, frame, "records")
    assert gpu.gbuf_reuses() == 0
    gpu.set_tuning("layout.records", 0)   # back on the planes: one tracing frame, then reuse
    for frame in range(3, 6):
        check_frame(gpu, oracle, osc, cam, W0, H0, f, frame, "planes again")
    assert gpu.gbuf_reuses() == 2


@pytest.mark.parametrize("first", ["biased", "unbiased"])
def test_skip_word_changes(gpu, oracle, first):
    """A biased frame (background tiles' reservoirs skipped) and a single-pass unbiased frame (their G-buffer records
    too) of one view, in both orders, without a returned grid as the benchmark renders: the unbiased frame may read the
    biased one's G-buffer, the biased frame must not read the unbiased one's."""
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam = camera("nightclub_far", W0, H0)
    fb, fu = features(1), features(1, unbiased_combination=1)
    order = [fb, fu, fu, fb] if first == "biased" else [fu, fb, fb, fu]
    gpu.set_seed(SEED, 0)
    counts = []
    for frame, f in enumerate(order):
        check_frame(gpu, oracle, osc, cam, W0, H0, f, frame, f"{first} first", want_grid=False)
        counts.append(gpu.gbuf_reuses())
    assert counts[1] == (1 if first == "biased" else 0), counts   # unbiased after biased reuses, biased after unbiased traces


@pytest.mark.parametrize("N", [1, 2])
def test_initial_visibility_keeps_the_bvh(gpu, oracle, N):
    """initial_samples_visibility_check: the reuse kernel stages the BVH for the candidates' shadow rays."""
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam = camera("nightclub_in", W0, H0)
    gpu.set_seed(SEED, 0)
    for frame, vis in enumerate([0, 1, 1, 0]):
        check_frame(gpu, oracle, osc, cam, W0, H0, features(1, N, initial_samples_visibility_check=vis), frame,
                    f"initial_vis={vis} N={N}")
        assert gpu.gbuf_reuses() == frame


# --------------------------------------------------------------------------------------------------------
# the knob, and two contexts on two threads
def test_knob_off_every_frame_traces(gpu, oracle):
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam, f = camera("nightclub_far", W0, H0), features(1)
    gpu.set_tuning("gbuf.reuse", 0)
    gpu.set_seed(SEED, 0)
    for frame in range(3):
        check_frame(gpu, oracle, osc, cam, W0, H0, f, frame, "gbuf.reuse=0")
    assert gpu.gbuf_reuses() == 0


def test_any_knob_makes_the_next_frame_trace(gpu, oracle):
    s = get_scene(NIGHTCLUB)
    gpu.set_scene(s)
    osc = oracle.OracleScene(s)
    cam, f = camera("nightclub_far", W0, H0), features(1)
    gpu.set_seed(SEED, 0)
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 0, "before")
    gpu.set_tuning("miss.tiles", 0)   # the next frame writes no flags
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 1, "miss.tiles=0")
    assert gpu.gbuf_reuses() == 0
    gpu.set_tuning("miss.tiles", 1)
    check_frame(gpu, oracle, osc, cam, W0, H0, f, 2, "miss.tiles=1")
    assert gpu.gbuf_reuses() == 0


def test_two_contexts_on_two_threads(oracle):
    """Two contexts, one per thread, render their own cameras in turn (tests/cpp/render_threads.cpp through Python
    threads): each context's frames equal its own oracle frames and reuse its own G-buffer."""
    from romis_amd import build, restir
    build.build()
    w, h, frames = 96, 40, 3
    s = get_scene(NIGHTCLUB)
    f = features(1)
    cams = [camera("nightclub_far", w, h), camera("nightclub_in", w, h)]
    got = [[None] * frames for _ in cams]
    reuses, errors = [None, None], []
    turn = [threading.Semaphore(1), threading.Semaphore(0)]

    def worker(i):
        try:
            r = restir.Renderer(0)
            try:
                r.set_scene(s)
                r.set_seed(SEED, 0)
                for frame in range(frames):
                    turn[i].acquire()          # strictly alternating frames
                    try:
                        got[i][frame], _ = r.render_restir(None, cams[i], w, h, f, want_grid=False)
                    finally:
                        turn[1 - i].release()
                reuses[i] = r.gbuf_reuses()
            finally:
                r.close()
        except Exception as e:   # noqa: BLE001 -- reported by the asserting thread
            errors.append(e)
            turn[1 - i].release()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    osc = oracle.OracleScene(s)
    for i, cam in enumerate(cams):
        for frame in range(frames):
            want, _, _ = oracle.render_frame(osc, cam, f, w, h, SEED, frame)
            assert_bits(got[i][frame], want, f"context {i} frame {frame}")
        assert reuses[i] == frames - 1
