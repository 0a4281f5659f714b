"""The reprojected image history on the device (include/restir_c.h "a reprojected image history", csrc/history.h /
history.hip), every comparison bit for bit.

1  a still camera: after five advances the mean is restir_accum_download's of the same frames, n is 5 on every surface
   pixel (a miss pixel is reason 0 at every advance and so holds one sample, the constant background), the map is the
   identity on surface pixels and reason 0 on misses; nightclub, Cornell and Monkey at 70 x 37, 33 x 17 and 3 x 37.
   Monkey's smooth-shaded pixels whose stored normal has N.N < 0.906 fail restir_frame_reproject's normal test against
   themselves (reason 5, on the CPU restatement first) and hold one sample like the misses;
2  a moving camera: four advances to and fro along each pair of tests/test_history_host.py's PAIRS; after each the map is
   restir_history_map_host's over the oracle's G-buffers and the downloaded previous counts, the state is
   restir_history_fold's of the previous state, the map and the frame, and outside reasons 6 and 7 the map is
   restir_frame_reproject's for the same two cameras;
3  the cap, max_frames = 2;
4  an uploaded image with NaN and inf pixels, over valid and over no history;
5  restir_history_denoise equals restir_denoise_lum_host(mean, var = restir_history_variance_host(...)), colour and final
   variance plane, one to five levels at 70 x 37 and 130 x 70 after a camera move; with the tone fields the result is the
   tone map of the linear result;
6  no side effects on frames, grids and the still view's counters; one guide trace per view across advance,
   history_denoise and denoise_lum; restir_accum_* works alongside;
7  restir_set_scene and restir_update_meshes reset, restir_set_lights does not;
8  every error leaves image, history and counters alone;
9  it helps: the device's 8-frame yaw sequence has the bits of the oracle's, on which test_history_host.py establishes the
   inequalities, and they hold against render_exact on the device.
GPU against the CPU; images are at most 130 x 70."""
import ctypes as C

import numpy as np
import pytest

import exact_spec
import history_spec as hs
from romis_amd import _abi, restir, scene
from test_gpu_exact import NIGHT, SEED, assert_bits, bits, c2, c3, counters
from test_gpu_reproject import CORNELL, MONKEY, framed_camera, night_camera, the_scene
from test_history_host import LIN, PAIRS, assert_words, gbuf, oracle_sequence, oscene
from test_reproject_host import NONE, camera_frame, np_map

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
INVALID, STATE, UNSUPPORTED = 1, 4, 5
R7 = NONE - hs.NO_HISTORY


@pytest.fixture(scope="module")
def lib():
    from romis_amd import build
    build.build()
    return _abi.load_library()


@pytest.fixture()
def gpu(lib):
    r = restir.Renderer(0)
    yield r
    r.close()


def setup(r, name, leaf=None):
    if leaf is not None:
        r.set_tuning("bvh.max_leaf", leaf)
    r.set_scene(the_scene(name))
    r.set_seed(SEED, 0)


def frame(r, cam, w, h, f=None):
    """the next linear C2 frame as the context's image"""
    return r.render_restir(None, cam, w, h, f or c2(**LIN), want_grid=False)[0]


def miss_of(name):
    return len(the_scene(name).meshes)


def assert_state(got, want, what):
    for g, w_, part in zip(got, want, ("mean", "S", "n")):
        assert_words(g, w_, f"{what}: {part}")


def empty_state(w, h):
    return np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32), np.zeros((h, w), U32)


# ---- 1: a still camera ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cam,w,h", [(NIGHT, night_camera, 70, 37), (NIGHT, night_camera, 3, 37), (CORNELL, framed_camera, 33, 17),
                                          (MONKEY, framed_camera, 33, 17), (MONKEY, framed_camera, 70, 37)])
def test_still_camera_is_the_accumulator(gpu, oracle, name, cam, w, h):
    setup(gpu, name)
    cam = cam(w, h)
    miss = miss_of(name)
    gb = gbuf(oracle, name, cam, w, h)
    surface = hs.flip(hs.material(gb[1], miss) != miss, w, h)   # image rows
    # The still view's map: the identity on surface pixels, reason 0 on misses.  Step 5 compares the G-buffer's normals as
    # they are stored, unnormalised, so a pixel whose interpolated normal has N.N < 0.906 (Monkey's smooth shading) fails
    # restir_frame_reproject's own normal test against itself and starts over at every advance: reason 5, as that call's
    ident = np.arange(w * h, dtype=U32).reshape(h, w)
    want_map = hs.np_map(camera_frame(_abi.load_library(), cam), w, h, gb, (gb[0], hs.material(gb[1], miss), np.ones((h, w), U32)),
                         miss).reshape(h, w)
    short = hs.flip(want_map == NONE - 5, w, h)
    assert_words(want_map, np.where(hs.flip(surface & ~short, w, h), ident, np.where(hs.flip(short, w, h), U32(NONE - 5), U32(NONE))),
                 "identity, reason 0 or reason 5")
    assert not short.any() or name == MONKEY, "flat-shaded scenes keep every surface pixel"
    kept = surface & ~short
    assert kept.sum() * 4 >= w * h or w == 3
    gpu.history_begin()
    gpu.accum_begin(True)
    try:
        for k in range(5):
            last = frame(gpu, cam, w, h)
            gpu.accum_add()
            smap = gpu.history_advance(cam, w, h, want_map=True)
            if k == 0:
                assert (smap == R7).all()
            else:
                assert_words(smap, want_map, f"{name} {w}x{h}: the map of advance {k}")
        mean, S, n = gpu.history_state()
        amean, am2 = gpu.accum_state(w, h)
        assert_bits(mean[~short], amean[~short], f"{name} {w}x{h}: the mean of five")
        assert_bits(mean[short], last[short], f"{name} {w}x{h}: a pixel that starts over shows the last frame")
        assert (n[kept] == 5).all() and (n[~kept] == 1).all()
        assert np.allclose(S[kept], am2[kept] / F32(5.0), rtol=1e-4, atol=1e-30)
        assert gpu.history_frames() == (5, 0)
        gpu.history_resolve(None)
        assert_bits(gpu.download_rgb(w, h), mean, "the resolve")
    finally:
        gpu.accum_end()
        gpu.history_end()


# ---- 2: a moving camera -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_moving_camera_equals_the_host_functions(gpu, oracle, lib, pair):
    name, cp, cc, w, h, leaf = PAIRS[pair]
    setup(gpu, name, leaf)
    miss = miss_of(name)
    assert miss == oscene(oracle, name).miss_material
    cams = [cp(), cc(), cp(), cc()]
    gpu.history_begin(restir.history_params(max_frames=32))
    state, maps = empty_state(w, h), []
    for k, cam in enumerate(cams):
        x = frame(gpu, cam, w, h)
        smap = gpu.history_advance(cam, w, h, want_map=True)
        gb = gbuf(oracle, name, cam, w, h)
        if k == 0:
            want = restir.history_map_host(camera_frame(lib, cam), w, h, gb, None, miss)
        else:
            pgb = gbuf(oracle, name, cams[k - 1], w, h)
            want = restir.history_map_host(camera_frame(lib, cams[k - 1]), w, h, gb, (pgb[0], hs.material(pgb[1], miss), state[2]), miss)
            assert hs.classes(want)["moved"] * 4 >= w * h
        assert_words(smap, want, f"{pair}: the map of advance {k}")
        state = restir.history_fold(*state, smap, x, 32)
        assert_state(gpu.history_state(), state, f"{pair}: the state after advance {k}")
        maps.append(smap)
    assert state[2].max() >= 3 and gpu.history_frames() == (4, 0)
    # after each move, outside reasons 6 and 7, the map is restir_frame_reproject's for the same two cameras
    from test_gpu_scene_shapes import feats
    for k in (1, 2, 3):
        _, grid = gpu.render_restir(None, cams[k - 1], w, h, feats(1, 1, temporal=1))
        _, rmap = gpu.reproject(grid, cams[k - 1], cams[k], want_map=True)
        own = (maps[k] == NONE - hs.MATERIAL) | (maps[k] == R7)
        assert (~own).sum() * 2 >= w * h
        assert_words(maps[k][~own], rmap[~own], f"{pair}: advance {k} against restir_frame_reproject's map")
        assert_words(rmap, np_map(camera_frame(lib, cams[k - 1]), w, h, gbuf(oracle, name, cams[k], w, h),
                                  gbuf(oracle, name, cams[k - 1], w, h), miss), f"{pair}: restir_frame_reproject's map of move {k}")
    gpu.history_end()


# ---- 3: the cap -------------------------------------------------------------------------------------------------------------
def test_cap_of_two_frames(gpu, oracle, lib):
    w, h = 70, 37
    setup(gpu, NIGHT)
    cams = [night_camera(w, h, yaw=30.0 + 0.6 * k) for k in range(5)]
    gpu.history_begin(restir.history_params(max_frames=2))
    state = empty_state(w, h)
    for k, cam in enumerate(cams):
        x = frame(gpu, cam, w, h)
        smap = gpu.history_advance(cam, w, h, want_map=True)
        state = restir.history_fold(*state, smap, x, 2)
        assert_state(gpu.history_state(), state, f"advance {k}")
        assert_state(state, hs.fold(*prev, smap, x, 2) if k else state, f"advance {k}: the restatement")
        prev = state
    assert state[2].max() == 2 and (state[2] == 2).sum() > w * h // 2
    gpu.history_end()


# ---- 4: an image with NaN and inf pixels ------------------------------------------------------------------------------------
def test_non_finite_pixels(gpu, oracle, lib):
    w, h = 33, 17
    setup(gpu, NIGHT)
    cam = night_camera(w, h)
    miss = miss_of(NIGHT)
    surface = hs.flip(hs.material(gbuf(oracle, NIGHT, cam, w, h)[1], miss) != miss, w, h)
    on, off = np.argwhere(surface), np.argwhere(~surface)
    assert len(on) >= 6 and len(off) >= 3
    gpu.history_begin(restir.history_params(max_frames=32))
    gpu.stage_configure(w, h, 1)
    good = frame(gpu, cam, w, h)
    state = empty_state(w, h)

    def advance(img, what):
        nonlocal state
        gpu.stage_configure(w, h, 1)
        gpu.upload(_abi.BUF_RGB, img)
        smap = gpu.history_advance(cam, w, h, want_map=True)
        state = restir.history_fold(*state, smap, img, 32)
        assert_state(gpu.history_state(), state, what)
        assert_state(state, hs.fold(*before, smap, img, 32), f"{what}: the restatement")
        return smap

    # no history under the bad pixels: they show x's bits and stay empty
    bad = good.copy()
    specials = [np.nan, np.inf, -np.inf]
    for j, (r_, c_) in enumerate(list(on[:3]) + list(off[:3])):
        bad[r_, c_, j % 3] = specials[j % 3]
    before = state
    advance(bad, "NaN and inf over no history")
    for r_, c_ in list(on[:3]) + list(off[:3]):
        assert state[2][r_, c_] == 0 and np.array_equal(bits(state[0][r_, c_]), bits(bad[r_, c_])) and (bits(state[1][r_, c_]) == 0).all()
    before = state
    smap = advance(good, "a good frame")
    assert (hs.flip(smap, w, h)[tuple(on[:3].T)] == R7).all(), "an empty record is reason 7"
    assert (state[2][surface] >= 1).all()
    # valid history under bad pixels: it passes through
    bad = good.copy()
    for j, (r_, c_) in enumerate(on[3:6]):
        bad[r_, c_, j] = specials[j]
    before = state
    advance(bad, "NaN and inf over valid history")
    for r_, c_ in on[3:6]:
        assert state[2][r_, c_] == 2 and np.array_equal(bits(state[0][r_, c_]), bits(before[0][r_, c_]))
    gpu.history_end()


# ---- 5: the filter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(70, 37), (130, 70)])
def test_history_denoise_equals_the_host_functions(gpu, oracle, lib, w, h):
    setup(gpu, NIGHT)
    miss = miss_of(NIGHT)
    cams = [night_camera(w, h, yaw=30.0 + 1.0 * k) for k in range(5)]
    hp = restir.history_params(spatial_below=3)
    gpu.history_begin(hp)
    for cam in cams:
        frame(gpu, cam, w, h)
        gpu.history_advance(cam, w, h)
    mean, S, n = gpu.history_state()
    assert (n < 3).sum() >= 16 and (n >= 3).sum() >= w * h // 4, "both branches of the variance plane"
    n_t, p_mat = gbuf(oracle, NIGHT, cams[-1], w, h)
    for iterations in range(1, 6):
        p = restir.denoise_lum_params(iterations=iterations)
        var = restir.history_variance_host(mean, S, n, n_t, p_mat, miss, hp, p.geo)
        want, want_v = restir.denoise_lum_host(mean, n_t, p_mat, miss, p, var=var)
        got = gpu.history_denoise(p)   # (the last image: a frame at first, then the call's own result)
        assert_bits(got, want, f"{w}x{h}, {iterations} levels")
        assert_bits(gpu.denoise_lum_variance(), want_v, f"{w}x{h}, {iterations} levels: the variance plane")
        assert_bits(gpu.download_rgb(w, h), got, "download_rgb")
    assert_state(gpu.history_state(), (mean, S, n), "the history is only read")
    # the variance plane's other variant (the spatial estimate everywhere, the history's entries over it): the same bits
    gpu.set_tuning("history.var_fused", 0)
    for iterations in (1, 2, 5):
        p = restir.denoise_lum_params(iterations=iterations, normal_power_log2=3, sigma_plane=0.05)
        var = restir.history_variance_host(mean, S, n, n_t, p_mat, miss, hp, p.geo)
        want, want_v = restir.denoise_lum_host(mean, n_t, p_mat, miss, p, var=var)
        three = gpu.history_denoise(p)
        assert_bits(three, want, f"{w}x{h}, {iterations} levels, three launches")
        assert_bits(gpu.denoise_lum_variance(), want_v, f"{w}x{h}, {iterations} levels, three launches: the variance plane")
        gpu.set_tuning("history.var_fused", 1)
        assert_bits(gpu.history_denoise(p), three, f"{w}x{h}, {iterations} levels, one launch")
        assert_bits(gpu.denoise_lum_variance(), want_v, f"{w}x{h}, {iterations} levels, one launch: the variance plane")
        gpu.set_tuning("history.var_fused", 0)
    gpu.set_tuning("history.var_fused", 1)
    with pytest.raises(_abi.RestirError, match="INVALID"):
        gpu.set_tuning("history.var_fused", 2)
    tone = _abi.default_features(gamma=2.2, exposure=0.7)
    p = restir.denoise_lum_params()
    want = restir.denoise_lum_host(mean, n_t, p_mat, miss, p, var=restir.history_variance_host(mean, S, n, n_t, p_mat, miss, hp, p.geo))[0]
    assert_bits(gpu.history_denoise(p, tone=tone), exact_spec.tonemap(oracle, want, tone.exposure, tone.gamma), "tone mapped")
    assert gpu.history_denoise(p, tone=_abi.default_features(**LIN), download=False) is None
    assert_bits(gpu.download_rgb(w, h), want, "tone mapping off, enqueue only")
    # variance_source is checked and otherwise ignored; the result is no frame
    assert_bits(gpu.history_denoise(restir.denoise_lum_params(variance_source=_abi.RESTIR_DENOISE_VAR_ACCUM)), want, "variance_source")
    assert lib.restir_history_denoise(gpu.ctx, C.byref(restir.denoise_lum_params(variance_source=2)), None, None) == INVALID
    assert lib.restir_history_advance(gpu.ctx, C.byref(cams[-1]), w, h, None) == STATE
    gpu.history_resolve(None)
    assert_bits(gpu.download_rgb(w, h), mean, "the resolve")
    gpu.history_resolve(tone)
    assert_bits(gpu.download_rgb(w, h), exact_spec.tonemap(oracle, mean, tone.exposure, tone.gamma), "the resolve, tone mapped")
    gpu.history_end()


# ---- 6: no side effects -----------------------------------------------------------------------------------------------------
FRAMES = 7


def run(sc, cams, w, h, f, history):
    r = restir.Renderer(0)
    try:
        r.set_scene(sc)
        r.set_seed(SEED, 0)
        out = dict(images=[], grids=[], builds=[])
        if history:
            r.history_begin()
            r.accum_begin(True)
        prev = None
        for k in range(FRAMES):
            cam = cams[k]
            rgb, grid = r.render_restir(prev if f.temporal_reuse else None, cam, w, h, f, want_grid=True)
            out["images"].append(rgb)
            out["grids"].append([np.asarray(a).copy() for a in grid.download()])
            prev = grid
            if history:
                r.history_advance(cam, w, h, want_map=k % 2 == 0)
                r.accum_add()   # the history's "folded already" mark is its own
                if k % 3 == 1:
                    r.history_denoise(download=k % 2 == 0)
                    r.denoise_lum(cam, w, h, download=False)
                elif k % 3 == 2:
                    r.history_resolve(None)
                out["builds"].append(r.denoise_guide_builds())
        out["counters"] = counters(r)
        out["ahead"] = (r.ahead_frames(), r.ahead_discards())
        if history:
            out["accum_frames"] = r.accum_stats().frames
            out["history"] = r.history_frames()
        return out
    finally:
        r.close()


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("cfg", ["c2", "c3"])
def test_history_changes_no_frame_and_no_cache(cfg, moving):
    w, h = 70, 37
    sc = the_scene(NIGHT)
    cams = [night_camera(w, h, yaw=30.0 + (0.6 * k if moving else 0.0)) for k in range(FRAMES)]
    f = dict(c2=c2, c3=c3)[cfg](**LIN)
    plain, mixed = run(sc, cams, w, h, f, False), run(sc, cams, w, h, f, True)
    for k in range(FRAMES):
        assert_bits(mixed["images"][k], plain["images"][k], f"{cfg} frame {k} image")
        for j, (a, b) in enumerate(zip(mixed["grids"][k], plain["grids"][k])):
            assert_bits(a.view(F32), b.view(F32), f"{cfg} frame {k} grid plane {j}")
    assert mixed["counters"] == plain["counters"] and mixed["ahead"] == plain["ahead"], cfg
    if not moving:
        assert plain["counters"]["gbuf_reuses"] == FRAMES - 1 and plain["counters"]["phat_builds"] == 1   # the still view's routes ran
    # one guide trace per view across advance, history_denoise and denoise_lum
    assert mixed["builds"] == ([k + 1 for k in range(FRAMES)] if moving else [1] * FRAMES)
    assert mixed["accum_frames"] == FRAMES and mixed["history"] == (FRAMES, 0)


# ---- 7: resets --------------------------------------------------------------------------------------------------------------
def test_geometry_changes_reset_and_lights_do_not(gpu, lib):
    w, h = 33, 17
    sc = the_scene(NIGHT)
    setup(gpu, NIGHT)
    cam = night_camera(w, h)
    gpu.history_begin()

    def advance():
        frame(gpu, cam, w, h)
        return gpu.history_advance(cam, w, h, want_map=True)

    assert (advance() == R7).all() and not (advance() == R7).any()
    gpu.set_lights(sc.lights[:7])
    assert not (advance() == R7).any() and gpu.history_frames() == (3, 0)
    gpu.set_scene(sc)
    assert gpu.history_frames() == (3, 1)
    assert lib.restir_history_resolve(gpu.ctx, None) == STATE
    assert lib.restir_history_denoise(gpu.ctx, C.byref(restir.denoise_lum_params()), None, None) == STATE
    assert (advance() == R7).all()
    assert (gpu.history_state()[2] == 1).all()
    assert not (advance() == R7).any()
    m = sc.meshes[9]
    gpu.update_meshes({9: ((np.ascontiguousarray(m.positions, F32) + F32(0.01)).astype(F32), None)})
    assert gpu.history_frames() == (5, 2)
    assert (advance() == R7).all() and gpu.history_frames() == (6, 2)
    gpu.history_end()


# ---- 8: errors --------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(gpu, lib):
    w, h = 33, 17
    cam = night_camera(w, h)
    adv = lambda c_=cam, w_=w, h_=h: lib.restir_history_advance(gpu.ctx, C.byref(c_) if c_ is not None else None, w_, h_, None)
    gpu.history_begin()
    assert adv() == STATE and b"restir_set_scene" in lib.restir_last_error()   # no scene
    gpu.history_end()
    setup(gpu, NIGHT)
    assert adv() == STATE and b"restir_history_begin" in lib.restir_last_error()   # no open history
    gpu.history_begin(restir.history_params(max_frames=32))
    assert adv() == STATE and b"nothing rendered" in lib.restir_last_error()       # no image
    assert lib.restir_history_resolve(gpu.ctx, None) == STATE                      # before the first advance
    assert lib.restir_history_denoise(gpu.ctx, C.byref(restir.denoise_lum_params()), None, None) == STATE
    assert lib.restir_history_download(gpu.ctx, None, None, None, w * h) == STATE
    img = frame(gpu, cam, w, h)
    gpu.history_advance(cam, w, h)
    img = frame(gpu, cam, w, h)
    gpu.history_advance(cam, w, h)
    state, frames, cnt, builds = gpu.history_state(), gpu.history_frames(), counters(gpu), gpu.denoise_guide_builds()

    def unchanged(what, image):
        assert_state(gpu.history_state(), state, what)
        assert gpu.history_frames() == frames and counters(gpu) == cnt and gpu.denoise_guide_builds() == builds, what
        assert_bits(gpu.download_rgb(image.shape[1], image.shape[0]), image, f"{what}: the image")

    assert adv() == STATE and b"folded already" in lib.restir_last_error()
    unchanged("an image folded already", img)
    img = frame(gpu, cam, w, h)
    cnt = counters(gpu)
    assert adv(None) == INVALID and adv(w_=0) == INVALID and adv(h_=0) == INVALID
    bad = _abi.Camera.from_buffer_copy(cam)
    bad.distance = float("nan")
    assert adv(bad) == INVALID and b"not finite" in lib.restir_last_error()
    assert adv(w_=w + 1) == STATE and adv(night_camera(70, 37), 70, 37) == STATE   # a size other than the history's
    assert lib.restir_history_denoise(gpu.ctx, None, None, None) == INVALID
    assert lib.restir_history_denoise(gpu.ctx, C.byref(restir.denoise_lum_params(iterations=6)), None, None) == INVALID
    assert lib.restir_history_download(gpu.ctx, None, None, None, w * h - 1) == INVALID
    unchanged("argument errors", img)
    # a screen tile's image
    tile = restir.tile_plan(w, h, 2, 1, 0, 10)   # (the ghost zone one C2 pass needs)
    part = gpu.render_restir(None, cam, w, h, c2(**LIN), tile=tile, want_grid=False)[0]
    cnt = counters(gpu)
    assert adv() == UNSUPPORTED
    unchanged("a screen tile's image", part)
    # a resolved and a denoised image
    img = frame(gpu, cam, w, h)
    cnt = counters(gpu)
    gpu.history_resolve(None)
    assert adv() == STATE and b"resolve" in lib.restir_last_error()
    unchanged("a resolved image", state[0])
    frame(gpu, cam, w, h)
    den = gpu.denoise(cam, w, h)
    cnt, builds = counters(gpu), gpu.denoise_guide_builds()
    assert adv() == STATE
    unchanged("a denoised image", den)
    # range errors of begin leave the open history alone
    for p in (_abi.HistoryParams(0, 4, 0, 0), _abi.HistoryParams(32, 1, 0, 0), _abi.HistoryParams(32, 4, 1, 0),
              _abi.HistoryParams(32, 4, 0, 1), _abi.HistoryParams(_abi.RESTIR_ACCUM_MAX_FRAMES + 1, 4, 0, 0)):
        assert lib.restir_history_begin(gpu.ctx, C.byref(p)) == INVALID
    assert lib.restir_history_begin(gpu.ctx, None) == INVALID
    unchanged("begin's range errors", den)
    # the history goes on
    x = frame(gpu, cam, w, h)
    smap = gpu.history_advance(cam, w, h, want_map=True)
    assert_state(gpu.history_state(), restir.history_fold(*state, smap, x, 32), "the next advance")
    gpu.history_end()
    assert lib.restir_history_frames(gpu.ctx, C.byref(C.c_uint64()), C.byref(C.c_uint64())) == STATE


def test_halo_frame_is_refused(gpu, lib):
    w, h = 33, 17
    setup(gpu, NIGHT)
    cam = night_camera(w, h)
    gpu.history_begin()
    frame(gpu, cam, w, h)
    gpu.history_advance(cam, w, h)
    state = gpu.history_state()
    frame(gpu, cam, w, h)
    f = c2(**LIN)
    gpu.halo_record(True)
    gpu.halo_begin(None, cam, w, h, f, (2, 1), 0)
    assert lib.restir_history_advance(gpu.ctx, C.byref(cam), w, h, None) == STATE and b"halo" in lib.restir_last_error()
    assert lib.restir_history_resolve(gpu.ctx, None) == STATE
    assert lib.restir_history_denoise(gpu.ctx, C.byref(restir.denoise_lum_params()), None, None) == STATE
    assert_state(gpu.history_state(), state, "a halo frame")
    for _ in range(f.spatial_resampling_passes):
        gpu.halo_pass()
    gpu.halo_end(restir.tile_plan(w, h, 2, 1, 0, f.spatial_resample_radius), False, False)
    gpu.halo_record(False)
    assert lib.restir_history_advance(gpu.ctx, C.byref(cam), w, h, None) == UNSUPPORTED, "the halo frame's image is a tile's"
    assert_state(gpu.history_state(), state, "a halo frame's tile")
    gpu.history_end()


# ---- 9: it helps ------------------------------------------------------------------------------------------------------------
def test_history_helps(gpu, oracle, lib):
    s = oracle_sequence(oracle, lib)
    w, h = s["w"], s["h"]
    setup(gpu, NIGHT)
    gpu.history_begin()
    for k, cam in enumerate(s["cams"]):
        assert_bits(frame(gpu, cam, w, h), s["frames"][k], f"frame {k} against the oracle's")
        assert_words(gpu.history_advance(cam, w, h, want_map=True), s["maps"][k], f"the map of advance {k}")
    assert_state(gpu.history_state(), (s["mean"], s["S"], s["n"]), "the history against the restatement over the oracle's frames")
    cam = s["cams"][-1]
    err = lambda: gpu.error("image")
    exact = gpu.render_exact(cam, w, h, c2(**LIN))
    assert_bits(exact, s["exact"], "render_exact")
    gpu.reference_set()
    gpu.set_seed(SEED, 7)
    assert_bits(frame(gpu, cam, w, h), s["frames"][-1], "frame 7 again")
    raw = err()
    assert_bits(gpu.denoise_lum(cam, w, h), s["spatial_dn"], "denoise_lum (SPATIAL) of frame 7")
    spatial = err()
    gpu.history_resolve(None)
    mean = err()
    assert_bits(gpu.history_denoise(), s["hist_dn"], "history_denoise")
    hist = err()
    assert mean.mse < raw.mse
    assert hist.rel_mse < spatial.rel_mse
    gpu.history_end()
