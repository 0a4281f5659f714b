"""The image history's bilinear gather on the device (include/restir_c.h "The gather of restir_history_advance",
csrc/history.h history_gather_bilinear, history.hip k_history_advance<kHistGatherBilinear>), every comparison bit for bit
against restir_history_advance_host over the oracle's G-buffers.

1  a moving camera: four advances to and fro along each pair of tests/test_history_host.py's PAIRS and the 3 x 37 pair,
   max_frames 32: after each the map and the downloaded state are the host function's of the state downloaded before;
2  the cap, max_frames = 2;
3  an uploaded image with NaN and inf pixels, over valid and over no history;
4  mixed modes on one history, each advance the host function of its mode; the mode is reported and survives
   history_end / history_begin and a set_scene reset;
5  NEAREST set explicitly is restir_history_fold as before;
6  history_denoise after four bilinear advances equals the host functions at 1, 2 and 5 levels, both history.var_fused values;
7  no side effects on frames, grids, counters and the look-ahead with the bilinear history on one side;
8  gather_set(2) is INVALID and leaves mode, state, counters and image alone;
9  it helps: the device's 16-frame sequence has the oracle sequence's bits, on which test_history_bilinear_host.py establishes
   the inequalities, and they hold against render_exact on the device.
GPU against the CPU; images are at most 130 x 70."""
import ctypes as C

import numpy as np
import pytest

import history_bilinear_spec as hb
import history_spec as hs
from romis_amd import _abi, restir
from test_gpu_exact import NIGHT, SEED, assert_bits, c2, c3, counters
from test_gpu_history import FRAMES, assert_state, empty_state, frame, miss_of, setup
from test_gpu_reproject import night_camera, the_scene
from test_history_bilinear_host import HELPS_CAP, PAIRS_B, oracle_sequence
from test_history_host import LIN, assert_words, gbuf, oscene
from test_reproject_host import NONE, camera_frame

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
INVALID = 1
NEAREST, BILINEAR = restir.HISTORY_GATHER_NEAREST, restir.HISTORY_GATHER_BILINEAR
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


def host_advance(lib, oracle, name, cams, k, w, h, state, x, cap, mode):
    """restir_history_advance_host for advance k of the camera list: the oracle's G-buffers, the state before"""
    miss = miss_of(name)
    gb = gbuf(oracle, name, cams[k], w, h)
    if k == 0:
        return restir.history_advance_host(camera_frame(lib, cams[0]), gb, None, *state, x, miss, cap, mode)
    pgb = gbuf(oracle, name, cams[k - 1], w, h)
    return restir.history_advance_host(camera_frame(lib, cams[k - 1]), gb, (pgb[0], hs.material(pgb[1], miss)), *state, x, miss, cap, mode)


def check_advance(gpu, lib, oracle, name, cams, k, w, h, state, x, cap, mode, what):
    smap = gpu.history_advance(cams[k], w, h, want_map=True)
    want = host_advance(lib, oracle, name, cams, k, w, h, state, x, cap, mode)
    assert_words(smap, want[3], f"{what}: the map of advance {k}")
    assert_state(gpu.history_state(), want[:3], f"{what}: the state after advance {k}")
    return want[:3], smap


# ---- 1: a moving camera -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(PAIRS_B))
def test_moving_camera_equals_the_host_function(gpu, oracle, lib, pair):
    name, cp, cc, w, h, leaf = PAIRS_B[pair]
    setup(gpu, name, leaf)
    assert miss_of(name) == oscene(oracle, name).miss_material
    cams = [cp(), cc(), cp(), cc()]
    assert gpu.history_gather(BILINEAR) == BILINEAR
    gpu.history_begin(restir.history_params(max_frames=32))
    state, blended = empty_state(w, h), 0
    for k in range(4):
        x = frame(gpu, cams[k], w, h)
        before = state
        state, smap = check_advance(gpu, lib, oracle, name, cams, k, w, h, state, x, 32, BILINEAR, pair)
        if k:
            near = host_advance(lib, oracle, name, cams, k, w, h, before, x, 32, NEAREST)
            blended += int((np.ascontiguousarray(near[0]).view(U32) != np.ascontiguousarray(state[0]).view(U32)).any(axis=-1).sum())
            assert ((near[3] <= NONE - 8) <= (smap <= NONE - 8)).all(), "every pixel the nearest mode accepts is accepted"
    assert blended * 4 >= w * h or w == 3, "the gather blends"
    assert state[2].max() >= 3 and gpu.history_frames() == (4, 0)
    gpu.history_end()


# ---- 2: the cap -------------------------------------------------------------------------------------------------------------
def test_cap_of_two_frames(gpu, oracle, lib):
    w, h = 70, 37
    setup(gpu, NIGHT)
    cams = [night_camera(w, h, yaw=30.0 + 0.6 * k) for k in range(5)]
    gpu.history_gather(BILINEAR)
    gpu.history_begin(restir.history_params(max_frames=2))
    state = empty_state(w, h)
    for k in range(5):
        x = frame(gpu, cams[k], w, h)
        state, _ = check_advance(gpu, lib, oracle, NIGHT, cams, k, w, h, state, x, 2, BILINEAR, "cap 2")
    assert state[2].max() == 2 and (state[2] == 2).sum() > w * h // 2
    gpu.history_end()


# ---- 3: an image with NaN and inf pixels ------------------------------------------------------------------------------------
def test_non_finite_pixels(gpu, oracle, lib):
    w, h = 33, 17
    setup(gpu, NIGHT)
    cams = [night_camera(w, h, yaw=30.0 + 0.9 * k) for k in range(3)]
    miss = miss_of(NIGHT)
    gpu.history_gather(BILINEAR)
    gpu.history_begin(restir.history_params(max_frames=32))
    state = empty_state(w, h)
    specials = [np.nan, np.inf, -np.inf]
    for k, cam in enumerate(cams):
        good = frame(gpu, cam, w, h)
        surface = hs.flip(hs.material(gbuf(oracle, NIGHT, cam, w, h)[1], miss) != miss, w, h)
        on, off = np.argwhere(surface), np.argwhere(~surface)
        assert len(on) >= 6 and len(off) >= 3
        bad = good.copy()
        mid = len(on) // 2 + 3 * (k % 2)   # (the image's middle: pixels the small yaw keeps)
        chosen = list(on[mid:mid + 3]) + list(off[:3])
        for j, (r_, c_) in enumerate(chosen):
            bad[r_, c_, j % 3] = specials[j % 3]
        gpu.stage_configure(w, h, 1)
        gpu.upload(_abi.BUF_RGB, bad)
        before = state
        state, smap = check_advance(gpu, lib, oracle, NIGHT, cams, k, w, h, state, bad, 32, BILINEAR, "NaN and inf")
        spec = hb.advance(camera_frame(lib, cams[k - 1]) if k else None, w, h, gbuf(oracle, NIGHT, cam, w, h),
                          None if k == 0 else (gbuf(oracle, NIGHT, cams[k - 1], w, h)[0],
                                               hs.material(gbuf(oracle, NIGHT, cams[k - 1], w, h)[1], miss)), *before, bad, miss, 32)
        assert_state(state, spec[:3], f"advance {k}: the restatement")
        if k == 0:
            for r_, c_ in chosen:
                assert state[2][r_, c_] == 0, "no history under a bad pixel: it stays empty"
    accepted = hs.flip(smap, w, h) <= NONE - 8
    passed = accepted & ~np.isfinite(bad).all(axis=-1)
    assert passed.any(), "a bad pixel over valid history"
    gpu.history_end()


# ---- 4, 5: mixed modes, and NEAREST set explicitly ---------------------------------------------------------------------------
def test_mixed_modes_on_one_history(gpu, oracle, lib):
    name, cp, cc, w, h, leaf = PAIRS_B["night_yaw"]
    setup(gpu, name, leaf)
    cams = [cp(), cc(), cp(), cc()]
    assert gpu.history_gather() == NEAREST
    gpu.history_begin(restir.history_params(max_frames=32))
    state = empty_state(w, h)
    for k, mode in enumerate((NEAREST, BILINEAR, NEAREST, BILINEAR)):
        assert gpu.history_gather(mode) == mode == gpu.history_gather()
        x = frame(gpu, cams[k], w, h)
        before = state
        state, smap = check_advance(gpu, lib, oracle, name, cams, k, w, h, state, x, 32, mode, f"mode {mode}")
        if mode == NEAREST:
            assert_state(state, restir.history_fold(*before, smap, x, 32), f"advance {k}: NEAREST is restir_history_fold of its map")
    # the mode survives history_end / history_begin and a reset
    gpu.history_end()
    assert gpu.history_gather() == BILINEAR
    gpu.history_begin(restir.history_params(max_frames=32))
    assert gpu.history_gather() == BILINEAR
    state = empty_state(w, h)
    for k in range(2):
        x = frame(gpu, cams[k], w, h)
        state, _ = check_advance(gpu, lib, oracle, name, cams, k, w, h, state, x, 32, BILINEAR, "after begin")
    gpu.set_scene(the_scene(name))
    assert gpu.history_gather() == BILINEAR and gpu.history_frames() == (2, 1)
    x = frame(gpu, cams[0], w, h)
    assert (gpu.history_advance(cams[0], w, h, want_map=True) == R7).all()
    state = restir.history_advance_host(camera_frame(lib, cams[0]), gbuf(oracle, name, cams[0], w, h), None, *empty_state(w, h), x,
                                        miss_of(name), 32, BILINEAR)[:3]
    x = frame(gpu, cams[1], w, h)
    check_advance(gpu, lib, oracle, name, cams, 1, w, h, state, x, 32, BILINEAR, "after the reset")
    gpu.history_end()


# ---- 6: the filter ----------------------------------------------------------------------------------------------------------
def test_history_denoise_after_bilinear_advances(gpu, oracle, lib):
    w, h = 70, 37
    setup(gpu, NIGHT)
    miss = miss_of(NIGHT)
    cams = [night_camera(w, h, yaw=30.0 + 1.0 * k) for k in range(4)]
    hp = restir.history_params(spatial_below=3)
    gpu.history_gather(BILINEAR)
    gpu.history_begin(hp)
    for cam in cams:
        frame(gpu, cam, w, h)
        gpu.history_advance(cam, w, h)
    mean, S, n = gpu.history_state()
    assert (n < 3).sum() >= 16 and (n >= 3).sum() >= w * h // 4, "both branches of the variance plane"
    n_t, p_mat = gbuf(oracle, NIGHT, cams[-1], w, h)
    for fused in (1, 0):
        gpu.set_tuning("history.var_fused", fused)
        for iterations in (1, 2, 5):
            p = restir.denoise_lum_params(iterations=iterations)
            var = restir.history_variance_host(mean, S, n, n_t, p_mat, miss, hp, p.geo)
            want, want_v = restir.denoise_lum_host(mean, n_t, p_mat, miss, p, var=var)
            assert_bits(gpu.history_denoise(p), want, f"{iterations} levels, var_fused {fused}")
            assert_bits(gpu.denoise_lum_variance(), want_v, f"{iterations} levels, var_fused {fused}: the variance plane")
    gpu.set_tuning("history.var_fused", 1)
    assert_state(gpu.history_state(), (mean, S, n), "the history is only read")
    gpu.history_end()


# ---- 7: no side effects -----------------------------------------------------------------------------------------------------
def run(sc, cams, w, h, f, history):
    """test_gpu_history.run with the bilinear gather on the history's side"""
    r = restir.Renderer(0)
    try:
        r.set_scene(sc)
        r.set_seed(SEED, 0)
        out = dict(images=[], grids=[], builds=[])
        if history:
            r.history_begin()
            r.history_gather(BILINEAR)   # with an open history
        prev = None
        for k in range(FRAMES):
            cam = cams[k]
            rgb, grid = r.render_restir(prev if f.temporal_reuse else None, cam, w, h, f, want_grid=True)
            out["images"].append(rgb)
            out["grids"].append([np.asarray(a).copy() for a in grid.download()])
            prev = grid
            if history:
                r.history_advance(cam, w, h, want_map=k % 2 == 0)
                if k == 3:
                    r.history_gather(NEAREST), r.history_gather(BILINEAR)   # setting the mode touches nothing
                if k % 3 == 1:
                    r.history_denoise(download=k % 2 == 0)
                elif k % 3 == 2:
                    r.history_resolve(None)
                out["builds"].append(r.denoise_guide_builds())
        out["counters"] = counters(r)
        out["ahead"] = (r.ahead_frames(), r.ahead_discards())
        if history:
            out["history"] = r.history_frames()
        return out
    finally:
        r.close()


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("cfg", ["c2", "c3"])
def test_bilinear_history_changes_no_frame_and_no_cache(cfg, moving):
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
    assert mixed["builds"] == ([k + 1 for k in range(FRAMES)] if moving else [1] * FRAMES)   # one guide trace per view
    assert mixed["history"] == (FRAMES, 0)


# ---- 8: errors --------------------------------------------------------------------------------------------------------------
def test_a_bad_mode_changes_nothing(gpu, lib):
    w, h = 33, 17
    setup(gpu, NIGHT)
    cam = night_camera(w, h)
    gpu.history_gather(BILINEAR)
    gpu.history_begin()
    for _ in range(2):
        img = frame(gpu, cam, w, h)
        gpu.history_advance(cam, w, h)
    img = frame(gpu, cam, w, h)
    state, frames, cnt, builds = gpu.history_state(), gpu.history_frames(), counters(gpu), gpu.denoise_guide_builds()
    for bad in (2, 3, 0xFFFFFFFF):
        assert lib.restir_history_gather_set(gpu.ctx, bad) == INVALID and b"gather" in lib.restir_last_error()
    assert lib.restir_history_gather_get(gpu.ctx, None) == INVALID
    with pytest.raises(_abi.RestirError, match="INVALID"):
        gpu.history_gather(2)
    assert gpu.history_gather() == BILINEAR
    assert_state(gpu.history_state(), state, "a bad mode")
    assert gpu.history_frames() == frames and counters(gpu) == cnt and gpu.denoise_guide_builds() == builds
    assert_bits(gpu.download_rgb(w, h), img, "a bad mode: the image")
    gpu.history_end()


# ---- 9: it helps ------------------------------------------------------------------------------------------------------------
def test_bilinear_history_helps(gpu, oracle, lib):
    s = oracle_sequence(oracle, lib)
    w, h = s["w"], s["h"]
    errs = {}
    for mode in (NEAREST, BILINEAR):
        setup(gpu, NIGHT)
        gpu.history_gather(mode)
        gpu.history_begin(s["params"])
        assert s["params"].max_frames == HELPS_CAP
        for k, cam in enumerate(s["cams"]):
            assert_bits(frame(gpu, cam, w, h), s["frames"][k], f"frame {k} against the oracle's")
            assert_words(gpu.history_advance(cam, w, h, want_map=True), s["maps"][mode][k], f"mode {mode}: the map of advance {k}")
            assert_state(gpu.history_state(), s["states"][mode][k], f"mode {mode}: the state after advance {k}")
        assert_bits(gpu.render_exact(s["cams"][-1], w, h, c2(**LIN)), s["exact"], "render_exact")
        gpu.reference_set()
        gpu.history_resolve(None)
        mean = gpu.error("image")
        assert_bits(gpu.history_denoise(), s["dn"][mode], f"mode {mode}: history_denoise")
        errs[mode] = (mean, gpu.error("image"))
        gpu.history_end()
    (mn, dn), (mb, db) = errs[NEAREST], errs[BILINEAR]
    print(f"history mean MAE {mn.mae:.4f} -> {mb.mae:.4f}  history_denoise rel_mse {dn.rel_mse:.4f} -> {db.rel_mse:.4f}  "
          f"history_denoise MAE {dn.mae:.4f} -> {db.mae:.4f}")
    assert mb.mae < mn.mae
    assert db.rel_mse < dn.rel_mse
    assert db.mae < dn.mae
