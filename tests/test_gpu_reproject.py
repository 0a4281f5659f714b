"""Motion-compensated temporal reuse on the GPU: restir_frame_reproject (include/restir_c.h), every comparison bit for bit.

The expected side is tests/test_reproject_host.py's numpy float32 restatement over the oracle's two G-buffers (np_map) and
a numpy gather of the predecessor grid; the frames that consume a reprojected grid are the oracle's own
render_frame(prev = the gathered grid): the oracle is used as it stands.  Frames are 70 x 37 and 33 x 17 (ragged 32 x 8
tiles) and one 3 pixels wide.  The oracle's sequences are computed once and shared by the knob variants.

Identity: a miss pixel of the reprojected grid is empty by definition, so the frame rendered from it differs from the
frame rendered from the predecessor itself in one word, the M of those miss pixels (which counts the predecessor's
samples; nothing reads it -- a miss pixel has a zero normal and is no one's neighbour in a biased pass).  The image, every
hit pixel and every other word are equal, and where every pixel hits geometry (a Cornell view from inside the box) the
whole grid is.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from romis_amd import _abi, scene
from test_gpu_parity import SEED, assert_bits, assert_grid, get_scene
from test_gpu_scene_shapes import counted, feats
from test_reproject_host import NONE, REASONS, camera_frame, classes, np_map

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
W, H = 70, 37
W2, H2 = 33, 17
NIGHT, CORNELL, MONKEY = "nightclub_128pt", "cornell_parallelogram", "Monkey"
NIGHT_BOX = 9       # a box on the nightclub's floor (tests/test_gpu_dynamic_scene.py)
INVALID, STATE, UNSUPPORTED = 1, 4, 5


@pytest.fixture()
def gpu():
    from romis_amd import build, restir
    build.build()
    r = restir.Renderer(0)
    yield r
    r.close()


def the_scene(name):
    return scene.load_prebuilt(name) if name == MONKEY else get_scene(name)


def night_camera(w, h, yaw=30.0, dist=25.0):
    """The nightclub's default camera (scene.nightclub_camera) with another yaw / distance."""
    return scene.make_camera(30.0, dist, (2.57, 1.23, -1.35), (10.3, yaw, 0.0), w, h)


def framed_camera(w, h, yaw=0.0, dist=0.0):
    c = scene.CORNELL_FRAMED
    rot = c["rot_deg"]
    return scene.make_camera(c["fov_deg"], c["dist"] + dist, c["look_at"], (rot[0], rot[1] + yaw, rot[2]), w, h)


# scene -> (predecessor's camera, current camera, width, height, bvh.max_leaf)
PAIRS = {
    "night_yaw": (NIGHT, lambda: night_camera(W, H), lambda: night_camera(W, H, yaw=36.0), W, H, None),
    "night_dolly": (NIGHT, lambda: night_camera(W, H, dist=2.0), lambda: night_camera(W, H), W, H, None),
    "night_thin": (NIGHT, lambda: night_camera(3, H), lambda: night_camera(3, H, yaw=36.0), 3, H, None),
    "cornell": (CORNELL, lambda: framed_camera(W, H), lambda: framed_camera(W, H, yaw=8.0, dist=0.3), W, H, None),
    "monkey_leaf2": (MONKEY, lambda: framed_camera(W2, H2), lambda: framed_camera(W2, H2, yaw=-7.0, dist=-0.2), W2, H2, 2),
}

_oscenes, _maps = {}, {}


def oscene(oracle, name):
    if name not in _oscenes:
        _oscenes[name] = oracle.OracleScene(the_scene(name))
    return _oscenes[name]


def expected_map(oracle, osc, cam_prev, cam_cur, w, h):
    """The restatement's map from the oracle's G-buffers of the two cameras."""
    gb_cur, gb_prev = oracle.gbuffer(osc, cam_cur, w, h), oracle.gbuffer(osc, cam_prev, w, h)
    return np_map(camera_frame(_abi.load_library(), cam_prev), w, h, gb_cur, gb_prev, osc.miss_material)


def pair_map(oracle, pair):
    if pair not in _maps:
        name, cp, cc, w, h, _ = PAIRS[pair]
        m = expected_map(oracle, oscene(oracle, name), cp(), cc(), w, h)
        m.flags.writeable = False
        _maps[pair] = m
    return _maps[pair]


def planes(grid):
    """A device grid as the oracle's planes: (res_a, res_b) [N][pixels][4] float32, res_b's w = bits(M)."""
    pos, col, w, m = grid.download()
    N = w.shape[0]
    a = np.concatenate([pos.reshape(N, -1, 3), w.reshape(N, -1, 1)], axis=2)
    b = np.concatenate([col.reshape(N, -1, 3), m.reshape(N, -1, 1).view(f32)], axis=2)
    return np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)


def gathered(res, m):
    """The predecessor planes `res` moved by map m: plane[:, p] = plane[:, m[p]], all-zero words where m rejects."""
    m = np.asarray(m).reshape(-1)
    ok = m <= NONE - len(REASONS)
    src = np.where(ok, m, 0).astype(np.int64)
    out = []
    for r in res:
        g = np.ascontiguousarray(r).view(u32)[:, src].copy()
        g[:, ~ok] = 0
        out.append(np.ascontiguousarray(g.view(f32)))
    return tuple(out)


def same_words(got, want, what):
    for k, (g, w_) in enumerate(zip(got, want)):
        g, w_ = np.ascontiguousarray(g).view(u32), np.ascontiguousarray(w_).view(u32)
        assert g.shape == w_.shape, f"{what}: shapes {g.shape} / {w_.shape}"
        bad = np.argwhere(g != w_)
        assert bad.size == 0, f"{what} plane {'ab'[k]}: {len(bad)} of {g.size} words differ, first at (j, pixel, word) {bad[0].tolist()}"


def setup(gpu, name, leaf=None):
    if leaf is not None:
        gpu.set_tuning("bvh.max_leaf", leaf)
    gpu.set_scene(the_scene(name))
    gpu.set_seed(SEED, 0)


# ---- the map and the gathered grid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("pair", ["night_yaw", "cornell", "monkey_leaf2"])
def test_map_and_grid_equal_the_restatement(gpu, oracle, pair, N):
    name, cp, cc, w, h, leaf = PAIRS[pair]
    setup(gpu, name, leaf)
    if pair == "monkey_leaf2":
        assert gpu.scene_info().bvh_lds_bytes > 65536   # the global-BVH primary kernel
    want = pair_map(oracle, pair)
    cls = classes(want, w)
    assert cls["moved"] >= 16 and cls["valid"] < w * h, cls
    _, prev = gpu.render_restir(None, cp(), w, h, feats(N, 1, temporal=1))
    before = planes(prev)
    grid, got = gpu.reproject(prev, cp(), cc(), want_map=True)
    assert got.shape == (h, w)
    bad = np.flatnonzero(got.reshape(-1) != want)
    assert bad.size == 0, f"{pair}: {bad.size} map entries differ, first pixel {bad[0]}: {got.reshape(-1)[bad[0]]:#x} != {want[bad[0]]:#x}"
    assert grid.info() == prev.info()
    same_words(planes(grid), gathered(before, want), f"{pair} N={N} reprojected grid")
    same_words(planes(prev), before, f"{pair} N={N}: the predecessor after the call")
    # without the map the call only enqueues; the grid is the same
    same_words(planes(gpu.reproject(prev, cp(), cc())), gathered(before, want), f"{pair} N={N} without a map")


def test_three_pixel_wide_frame_and_the_dolly(gpu, oracle):
    setup(gpu, NIGHT)
    for pair in ("night_thin", "night_dolly"):
        _, cp, cc, w, h, _ = PAIRS[pair]
        want = pair_map(oracle, pair)
        _, prev = gpu.render_restir(None, cp(), w, h, feats(2, 2, temporal=1))
        grid, got = gpu.reproject(prev, cp(), cc(), want_map=True)
        assert np.array_equal(got.reshape(-1), want), pair
        same_words(planes(grid), gathered(planes(prev), want), pair)


def test_every_class_occurs(oracle):
    """Every reject reason and "valid at another pixel" on >= 16 pixels of a case the map test compares -- the counts of
    the two nightclub pairs are the float64 figures of the feature's specification, to within a few pixels."""
    yaw, dolly = classes(pair_map(oracle, "night_yaw"), W), classes(pair_map(oracle, "night_dolly"), W)
    for key, n in {"miss": 681, "off-screen": 106, "predecessor miss": 30, "depth": 104, "normal": 56, "valid": 1613,
                   "moved": 1499}.items():
        assert abs(yaw[key] - n) <= 8 and yaw[key] >= 16, (key, yaw)
    for key, n in {"behind": 866, "off-screen": 921}.items():
        assert abs(dolly[key] - n) <= 8 and dolly[key] >= 16, (key, dolly)
    for key in list(REASONS) + ["moved"]:
        assert max(yaw[key], dolly[key]) >= 16, key


# ---- identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,passes", [(1, 2), (2, 1)])
def test_identity_on_the_nightclub(gpu, oracle, N, passes):
    """cam_prev == cam_cur: the predecessor on hit pixels, empty on misses; the next frame from either has the same image,
    the same grid on every hit pixel, and on miss pixels differs in M alone (module docstring)."""
    setup(gpu, NIGHT)
    cam, f = night_camera(W, H), feats(N, passes, temporal=1)
    osc = oscene(oracle, NIGHT)
    hit = np.ascontiguousarray(oracle.gbuffer(osc, cam, W, H)[1][:, 3]).view(u32) != osc.miss_material
    assert 16 <= hit.sum() <= W * H - 16
    _, prev = gpu.render_restir(None, cam, W, H, f)
    grid, m = gpu.reproject(prev, cam, cam, want_map=True)
    m = m.reshape(-1)
    assert np.array_equal(m[hit], np.arange(W * H, dtype=u32)[hit]) and (m[~hit] == NONE).all()
    pa, ga = planes(prev), planes(grid)
    for p, g in zip(pa, ga):
        assert np.array_equal(g.view(u32)[:, hit], p.view(u32)[:, hit]) and not g.view(u32)[:, ~hit].any()
    rgb1, next1 = gpu.render_restir(prev, cam, W, H, f)
    gpu.set_seed(SEED, 1)
    rgb2, next2 = gpu.render_restir(grid, cam, W, H, f)
    assert_bits(rgb2, rgb1, "identity: the next frame's image")
    (a1, b1), (a2, b2) = planes(next1), planes(next2)
    same_words((a2,), (a1,), "identity: the next grid's res_a")
    assert np.array_equal(b2.view(u32)[:, hit], b1.view(u32)[:, hit])
    assert np.array_equal(b2.view(u32)[:, ~hit, :3], b1.view(u32)[:, ~hit, :3])
    # both are the oracle's frames of their predecessors
    want, res, _ = oracle.render_frame(osc, cam, f, W, H, SEED, 1, prev=gathered(pa, m))
    assert_bits(rgb2, want, "identity: the oracle's frame")
    assert_grid(next2, res, "identity")


def test_identity_where_every_pixel_hits(gpu, oracle):
    """The framed Cornell camera half a unit closer sees no background (the 32 x 32 light grid scene): the reprojected grid
    is the predecessor, and so is the next frame."""
    setup(gpu, "cornell_1024")
    cam, f = framed_camera(W, H, dist=-0.5), feats(1, 2, temporal=1)
    osc = oscene(oracle, "cornell_1024")
    assert (np.ascontiguousarray(oracle.gbuffer(osc, cam, W, H)[1][:, 3]).view(u32) != osc.miss_material).all()
    _, prev = gpu.render_restir(None, cam, W, H, f)
    grid = gpu.reproject(prev, cam, cam)
    same_words(planes(grid), planes(prev), "identity")
    rgb1, next1 = gpu.render_restir(prev, cam, W, H, f)
    gpu.set_seed(SEED, 1)
    rgb2, next2 = gpu.render_restir(grid, cam, W, H, f)
    assert_bits(rgb2, rgb1, "identity: the next frame's image")
    same_words(planes(next2), planes(next1), "identity: the next frame's grid")


# ---- sequences -------------------------------------------------------------------------------------------------------
FRAMES = 4
_sequences = {}


def sequence_cameras(w, h):
    """The camera yaws 2 degrees and dollies in by 0.8 between frames."""
    return [night_camera(w, h, yaw=30.0 + 2.0 * k, dist=25.0 - 0.8 * k) for k in range(FRAMES)]


def moved_scene(s, k):
    """The nightclub with its floor box moved k steps (frame k of the update case)."""
    p = [np.ascontiguousarray(m.positions, f32) for m in s.meshes]
    p[NIGHT_BOX] = (p[NIGHT_BOX] + np.array([0.0, 0.4, 0.3], f32) * f32(k)).astype(f32)
    meshes = [dataclasses.replace(m, positions=q) for m, q in zip(s.meshes, p)]
    return scene.Scene(meshes, s.lights, s.name), p[NIGHT_BOX]


def oracle_sequence(oracle, key, f, moving):
    """[(image, grid planes, the map that led to the frame, its classes)] of the reprojected sequence on the oracle: before
    frame k > 0 the last grid is gathered by the restatement's map over the oracle's G-buffers of cameras k - 1 and k
    (both over the scene as it stands at frame k) and handed to render_frame as the predecessor."""
    if key not in _sequences:
        s = the_scene(NIGHT)
        cams = sequence_cameras(W, H)
        out, res = [], None
        for k in range(FRAMES):
            osc = oracle.OracleScene(moved_scene(s, k)[0]) if moving else oscene(oracle, NIGHT)
            m, prev = None, None
            if k:
                m = expected_map(oracle, osc, cams[k - 1], cams[k], W, H)
                prev = gathered(res, m)
            rgb, res, _ = oracle.render_frame(osc, cams[k], f, W, H, SEED, k, prev=prev)
            out.append((rgb, res, m, classes(m, W) if k else None))
        _sequences[key] = out
    return _sequences[key]


def run_sequence(gpu, oracle, f, key, knobs, moving=False):
    """The sequence on the device under tuning `knobs`; returns RESTIR_K_FINAL's launches per frame."""
    s = the_scene(NIGHT)
    want = oracle_sequence(oracle, key, f, moving)
    setup(gpu, NIGHT)
    for k_, v in knobs.items():
        gpu.set_tuning(k_, v)
    cams = sequence_cameras(W, H)
    grid, finals = None, []
    for k in range(FRAMES):
        rgb_w, res_w, m_w, cls = want[k]
        if moving and k:
            gpu.update_meshes({NIGHT_BOX: (moved_scene(s, k)[1], None)})
        prev = None
        if k:
            assert cls["moved"] >= 16 and cls["valid"] >= 16, cls   # reprojection matters in this sequence
            prev, m = gpu.reproject(grid, cams[k - 1], cams[k], want_map=True)
            assert np.array_equal(m.reshape(-1), m_w), f"{key} {knobs} frame {k}: map"
        with counted(gpu) as n:
            rgb, grid = gpu.render_restir(prev, cams[k], W, H, f)
        assert_bits(rgb, rgb_w, f"{key} {knobs} frame {k} rgb")
        assert_grid(grid, res_w, f"{key} {knobs} frame {k}")
        finals.append(n["final"])
    return finals


KNOBS = [{"fuse.temporal": ft, "spatial.handles": sh} for ft in (1, 0) for sh in (1, 0)]


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("N", [1, 2])
def test_reprojected_sequence_matches_oracle(gpu, oracle, N, passes):
    f = feats(N, passes, temporal=1)
    finals = {}
    for knobs in KNOBS:
        finals[(knobs["fuse.temporal"], knobs["spatial.handles"])] = run_sequence(gpu, oracle, f, ("seq", N, passes), knobs)
    if (N, passes) == (1, 2):
        # the handles came through the reprojection: every frame's passes read handles and the last one shades (no
        # RESTIR_K_FINAL launch), as tests/test_gpu_dynamic_scene.py observes for same-pixel reuse; without the knob
        # final shading is a launch of its own
        assert finals[(1, 1)] == [0] * FRAMES, finals
        assert finals[(1, 0)] == [1] * FRAMES, finals


def test_reprojected_sequence_unbiased_with_visibility(gpu, oracle):
    f = feats(1, 1, unbiased=1, vis=1, temporal=1)
    run_sequence(gpu, oracle, f, ("seq_unbiased_vis",), {})


def test_reprojected_sequence_with_a_moving_box(gpu, oracle):
    """restir_update_meshes between frames: both G-buffers of a reprojection are traced over the geometry as it stands."""
    f = feats(1, 2, temporal=1)
    run_sequence(gpu, oracle, f, ("seq_moving",), {}, moving=True)


def test_small_frame_sequence(gpu, oracle):
    """33 x 17: two frames, N = 2."""
    setup(gpu, NIGHT)
    osc = oscene(oracle, NIGHT)
    f = feats(2, 2, temporal=1)
    c0, c1 = night_camera(W2, H2), night_camera(W2, H2, yaw=33.0, dist=23.0)
    rgb_w, res_w, _ = oracle.render_frame(osc, c0, f, W2, H2, SEED, 0)
    m_w = expected_map(oracle, osc, c0, c1, W2, H2)
    rgb_w1, res_w1, _ = oracle.render_frame(osc, c1, f, W2, H2, SEED, 1, prev=gathered(res_w, m_w))
    rgb, grid = gpu.render_restir(None, c0, W2, H2, f)
    assert_bits(rgb, rgb_w, "33x17 frame 0")
    prev, m = gpu.reproject(grid, c0, c1, want_map=True)
    assert np.array_equal(m.reshape(-1), m_w) and classes(m_w, W2)["moved"] >= 16
    rgb, grid = gpu.render_restir(prev, c1, W2, H2, f)
    assert_bits(rgb, rgb_w1, "33x17 frame 1")
    assert_grid(grid, res_w1, "33x17 frame 1")


# ---- errors and lifetime ---------------------------------------------------------------------------------------------
def call(gpu, prev, cp, cc, out):
    return gpu.lib.restir_frame_reproject(gpu.ctx, prev.handle if prev is not None else None, C.byref(cp), C.byref(cc),
                                          C.byref(out), None)


def test_refused_predecessors(gpu, oracle):
    from romis_amd import restir
    cam, cam2 = night_camera(W, H), night_camera(W, H, yaw=36.0)
    out = C.c_void_p()
    other = restir.Renderer(0)
    try:
        other.set_scene(the_scene(NIGHT))
        _, whole = other.render_restir(None, cam, W, H, feats(1, 1, temporal=1))
        assert call(gpu, whole, cam, cam2, out) == STATE and out.value is None   # no scene on this context yet
        setup(gpu, NIGHT)
        assert call(gpu, None, cam, cam2, out) == INVALID
        tile = restir.tile_plan(W, H, 2, 1, 1, 0)
        _, part = gpu.render_restir(None, cam, W, H, feats(1, 0, temporal=1), tile=tile)
        assert call(gpu, part, cam, cam2, out) == UNSUPPORTED and out.value is None
        assert b"screen tile" in gpu.lib.restir_last_error()
        gpu.set_tuning("layout.records", 1)
        _, rec = gpu.render_restir(None, cam, W, H, feats(1, 1, temporal=1))
        gpu.set_tuning("layout.records", 0)
        assert call(gpu, rec, cam, cam2, out) == UNSUPPORTED and out.value is None
        assert b"records layout" in gpu.lib.restir_last_error()
        # a predecessor from the second context works, and that context may go first
        before = planes(whole)
        grid = gpu.reproject(whole, cam, cam2)
        same_words(planes(grid), gathered(before, pair_map(oracle, "night_yaw")), "a predecessor of another context")
        same_words(planes(whole), before, "the predecessor after the call")
    finally:
        other.close()
    same_words(planes(grid), gathered(before, pair_map(oracle, "night_yaw")), "after the producing context closed")


def test_frames_release_cleanly(gpu, oracle):
    """Predecessors released before their reprojections and the reverse, the pool re-using their records: the frames that
    follow are still the oracle's."""
    setup(gpu, NIGHT)
    osc = oscene(oracle, NIGHT)
    f = feats(1, 2, temporal=1)
    c0, c1 = night_camera(W, H), night_camera(W, H, yaw=36.0)
    want0, res0, _ = oracle.render_frame(osc, c0, f, W, H, SEED, 0)
    m_w = pair_map(oracle, "night_yaw")
    want1, res1, _ = oracle.render_frame(osc, c1, f, W, H, SEED, 1, prev=gathered(res0, m_w))
    for order in ("prev_first", "grid_first", "both_kept"):
        gpu.set_seed(SEED, 0)
        _, prev = gpu.render_restir(None, c0, W, H, f)
        grid = gpu.reproject(prev, c0, c1)
        spare = gpu.reproject(prev, c0, c1)
        if order == "prev_first":
            del prev
        elif order == "grid_first":
            del spare
            spare = gpu.reproject(prev, c0, c1)
        rgb, nxt = gpu.render_restir(grid, c1, W, H, f)
        assert_bits(rgb, want1, f"{order} rgb")
        assert_grid(nxt, res1, order)
        same_words(planes(spare), gathered(res0, m_w), f"{order}: a second reprojection")
        del grid, spare, nxt
    gpu.synchronize()
