"""Accumulating frames on the device (include/restir_c.h "accumulating frames", csrc/accum.h / accum.hip).

A  the device's fold equals the host's restir_accum_fold bit for bit after every add, at sizes whose float count leaves
   every remainder of the 16-byte groups, below one group and over several blocks, with and without the variance;
B  a resolve is the mean's bits, or the oracle's or_tonemap of them, and a present afterwards serves that image;
C  a still view keeps every cache while it accumulates: twelve frames with an add after each equal, bit for bit and
   counter for counter, the frames of a context that never accumulates, and the state is the host fold of the images;
D  restir_render_accumulate is that manual loop: state, resolved image, temporal chain and frame indices consumed;
E  the stats against numpy float64 within the worst-case summation bound, non-finite entries left out, and est_mse falls
   from 16 to 64 frames;
F  the adaptive stop ends at the frame count a manual run predicts, and max_frames caps it;
G  the calls that must fail with RESTIR_ERR_STATE do, and leave the state as it was.
GPU against host code and GPU against GPU; the oracle only tone maps.  Images are at most 70 x 37."""
import ctypes as C

import numpy as np
import pytest

from romis_amd import _abi, restir, scene

pytestmark = pytest.mark.gpu

STATE, INVALID = 4, 1
NAME = "nightclub_128pt"
SEED = _abi.RESTIR_DEFAULT_SEED
W, H = 64, 36
FRAMES = 12
SIZES = [(1, 1), (3, 2), (4, 1), (5, 3), (7, 5), (33, 17), (70, 37)]
F32 = np.float32
FP = C.POINTER(C.c_float)


def fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_bits(got, want, what):
    g, w_ = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w_.shape, f"{what}: shape {g.shape} != {w_.shape}"
    bad = np.flatnonzero(g != w_)
    assert bad.size == 0, f"{what}: {bad.size}/{g.size} words differ; first idx {bad[:4].tolist()}"


def assert_same(got, want, what):
    """Bit for bit, but a NaN for a NaN: its payload and sign are not part of the contract."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs in other places"
    assert np.array_equal(np.isinf(got), np.isinf(want)), f"{what}: infinities in other places"
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), f"{what}: {(bits(got)[~nan] != bits(want)[~nan]).sum()} words differ"


def c2(**kw):
    """bench.py's C2: N = 1, M = 32, k = 5, r = 10, one biased pass, no temporal reuse"""
    kw.setdefault("temporal_reuse", 0)
    kw.setdefault("spatial_resampling_passes", 1)
    return _abi.default_features(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5,
                                 spatial_resample_radius=10, spatial_reuse=1, **kw)


def c3(**kw):
    """... and C3: two passes and temporal reuse, every frame the next one's predecessor"""
    return c2(temporal_reuse=1, spatial_resampling_passes=2, **kw)


CONFIGS = {"c2": c2, "c3": c3}
TONE = dict(enable_tone_mapping=1, exposure=0.7, gamma=2.2)


@pytest.fixture(scope="module")
def lib():
    from romis_amd import build
    build.build()
    return _abi.load_library()


@pytest.fixture(scope="module")
def nightclub(lib):
    return scene.bench_scene(NAME), scene.camera_for(NAME, W, H)


def new_renderer(sc):
    r = restir.Renderer(0)
    r.set_scene(sc)
    r.set_seed(SEED, 0)
    return r


def counters(r):
    return dict(gbuf_reuses=r.gbuf_reuses(), shadow_list_frames=r.shadow_list_frames(), shadow_vis_frames=r.shadow_vis_frames(),
                shadow_vis_builds=r.shadow_vis_builds(), phat_frames=r.phat_frames(), phat_builds=r.phat_builds())


def host_fold(images, variance=True):
    """restir_accum_fold over the images in order, from the empty state"""
    mean, m2 = np.zeros(images[0].shape, F32), np.zeros(images[0].shape, F32)
    for n, x in enumerate(images, start=1):
        restir.accum_fold(mean, m2 if variance else None, x, n)
    return mean, m2


def oracle_tonemap(oracle, img, exposure, gamma):
    lib = oracle.lib()
    src = np.ascontiguousarray(img, F32).reshape(-1, 3)
    out = np.zeros_like(src)
    for i in range(len(src)):
        lib.or_tonemap(src[i].ctypes.data_as(FP), exposure, gamma, out[i].ctypes.data_as(FP))
    return out.reshape(np.shape(img))


# ---- A: device against host ---------------------------------------------------------------------------------------
def uploaded_images(w, h, nframes, nonfinite):
    """Images of moderate hashed values (so that sums stay finite), the special finite values at moving places and,
    with `nonfinite`, infinities and NaNs at a few"""
    n = w * h * 3
    out = []
    for k in range(nframes):
        u = fmix32(np.arange(n, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15 + 7919 * k))
        x = ((u >> np.uint32(8)).astype(F32) * F32(2.0 ** -21) - F32(2.0)).astype(F32)          # [-2, 6)
        special = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x3F7FFFFF, 0x3F800001]
        if nonfinite:   # ... and values whose differences overflow
            special += [0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFA55A5A]
        s = np.roll(np.array(special, np.uint32), k).view(F32)
        at = (np.arange(len(s)) * 5 + 3 * k) % n
        x[at] = s[:len(at)]
        out.append(x.reshape(h, w, 3))
    return out


@pytest.mark.parametrize("variance", [True, False])
@pytest.mark.parametrize("w,h", SIZES)
def test_device_fold_equals_the_host_fold(lib, w, h, variance):
    r = restir.Renderer(0)
    try:
        r.stage_configure(w, h, 1)
        for nonfinite in (False, True):
            images = uploaded_images(w, h, 7, nonfinite)
            r.accum_begin(variance)
            mean, m2 = np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32)
            for n, x in enumerate(images, start=1):
                r.upload(_abi.BUF_RGB, x)
                r.accum_add()
                restir.accum_fold(mean, m2 if variance else None, x, n)
                got_mean, got_m2 = r.accum_state(w, h)
                what = f"{w}x{h} variance={variance} nonfinite={nonfinite} after add {n}"
                if nonfinite:
                    assert_same(got_mean, mean, what + ": mean")
                    assert_same(got_m2, m2, what + ": m2")
                else:
                    assert_bits(got_mean, mean, what + ": mean")
                    assert_bits(got_m2, m2, what + ": m2")
            assert nonfinite or (np.isfinite(mean).all() and np.isfinite(m2).all())
            assert variance == bool(m2.any())
    finally:
        r.close()


# ---- B: resolve ----------------------------------------------------------------------------------------------------
def host_rgba8(lib, rgb):
    a = np.ascontiguousarray(rgb, F32)
    out = np.zeros(a.shape[:-1] + (4,), np.uint8)
    assert lib.restir_rgb_to_rgba8(a.ctypes.data, a.size // 3, out.ctypes.data) == 0
    return out


def host_bmp(lib, rgb):
    a = np.ascontiguousarray(rgb, F32)
    h, w = a.shape[:2]
    n = C.c_size_t()
    assert lib.restir_encode_bmp(a.ctypes.data, w, h, None, 0, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint8)
    assert lib.restir_encode_bmp(a.ctypes.data, w, h, buf.ctypes.data, n.value, C.byref(n)) == 0
    return buf


@pytest.mark.parametrize("w,h", [(5, 3), (70, 37)])
def test_resolve_is_the_mean_or_its_tone_map(lib, oracle, w, h, tmp_path):
    r = restir.Renderer(0)
    try:
        r.stage_configure(w, h, 1)
        images = uploaded_images(w, h, 5, False)
        r.accum_begin(True)
        for x in images:
            r.upload(_abi.BUF_RGB, x)
            r.accum_add()
        mean, _ = host_fold(images)
        assert (mean > 1.0).any() and (mean < 0.0).any() and np.isfinite(mean).all()
        r.accum_resolve(None)
        assert_bits(r.download_rgb(w, h), mean, "resolve without tone")
        assert_bits(r.accum_state(w, h)[0], mean, "the state after a resolve")
        for exposure, gamma in [(1.5, 1.0), (0.7, 2.2)]:
            f = _abi.default_features(enable_tone_mapping=1, exposure=exposure, gamma=gamma)
            r.accum_resolve(f)
            want = oracle_tonemap(oracle, mean, exposure, gamma)
            got = r.download_rgb(w, h)
            assert_same(got, want, f"resolve with exposure {exposure} gamma {gamma}")   # pow of a negative base: NaN
            assert np.isfinite(want).any()
            # a present afterwards serves the resolved image
            assert np.array_equal(r.download_rgba8(w, h), host_rgba8(lib, got))
            with r.present("bgra8_bottom_up") as im:
                assert (im.width, im.height) == (w, h)
                assert im.wait().tobytes() == host_bmp(lib, got)[122:].tobytes()
            path = tmp_path / f"resolved_{gamma}.bmp"
            r.write_bmp(path)
            assert path.read_bytes() == host_bmp(lib, got).tobytes()
        r.accum_resolve(_abi.default_features(enable_tone_mapping=0, exposure=0.7, gamma=2.2))
        assert_bits(r.download_rgb(w, h), mean, "resolve with enable_tone_mapping = 0")
    finally:
        r.close()


# ---- C, D: real frames of a still view -------------------------------------------------------------------------------
def manual_run(sc, cam, make, accumulate):
    """FRAMES frames of the still view without tone mapping, every image and grid read back; with `accumulate` an add
    after each, then the state, a resolve with TONE and one more frame"""
    f = make(enable_tone_mapping=0)
    r = new_renderer(sc)
    try:
        out = dict(images=[], grids=[])
        if accumulate:
            r.accum_begin(True)
        prev = None
        for _ in range(FRAMES):
            rgb, grid = r.render_restir(prev if f.temporal_reuse else None, cam, W, H, f, want_grid=True)
            if accumulate:
                r.accum_add()
            out["images"].append(rgb)
            out["grids"].append([np.asarray(a).copy() for a in grid.download()])
            prev = grid
        out["counters"] = counters(r)
        if accumulate:
            out["state"] = r.accum_state(W, H)
            out["stats"] = r.accum_stats()
            r.accum_resolve(make(**TONE))
            out["resolved"] = r.download_rgb(W, H)
        out["next"], _ = r.render_restir(prev if f.temporal_reuse else None, cam, W, H, f, want_grid=False)
        return out
    finally:
        r.close()


@pytest.fixture(scope="module", params=["c2", "c3"])
def still(request, nightclub):
    sc, cam = nightclub
    make = CONFIGS[request.param]
    return request.param, make, manual_run(sc, cam, make, True), manual_run(sc, cam, make, False)


def test_accumulating_changes_no_frame_and_no_cache(still):
    cfg, _, acc, plain = still
    for k in range(FRAMES):
        assert_bits(acc["images"][k], plain["images"][k], f"{cfg} frame {k} image")
        for j, (a, b) in enumerate(zip(acc["grids"][k], plain["grids"][k])):
            assert_bits(a.view(F32), b.view(F32), f"{cfg} frame {k} grid plane {j}")
    assert_bits(acc["next"], plain["next"], f"{cfg} frame {FRAMES}")
    assert not np.array_equal(bits(acc["images"][0]), bits(acc["images"][1]))   # independent frames
    assert acc["counters"] == plain["counters"], cfg
    # the routes a still nightclub view takes (tests/test_gpu_gbuf_reuse.py, _shadow_vis.py, _phat_table.py)
    assert acc["counters"]["gbuf_reuses"] == FRAMES - 1
    assert acc["counters"]["phat_frames"] > 0 and acc["counters"]["phat_builds"] == 1
    if cfg == "c2":
        assert acc["counters"]["shadow_list_frames"] > 0 and acc["counters"]["shadow_vis_frames"] > 0
        assert acc["counters"]["shadow_vis_builds"] == 1


def test_state_is_the_host_fold_of_the_frames(still):
    cfg, _, acc, _ = still
    mean, m2 = host_fold(acc["images"])
    assert_bits(acc["state"][0], mean, f"{cfg} mean")
    assert_bits(acc["state"][1], m2, f"{cfg} m2")
    assert (m2 > 0).any() and np.isfinite(m2).all()


def test_render_accumulate_is_the_manual_loop(still, nightclub, oracle):
    cfg, make, acc, _ = still
    sc, cam = nightclub
    r = new_renderer(sc)
    try:
        rgb, stats = r.render_accumulated(cam, W, H, make(**TONE), FRAMES)
        assert (stats.width, stats.height, stats.frames, stats.flags) == (W, H, FRAMES, _abi.RESTIR_ACCUM_VARIANCE)
        mean, m2 = r.accum_state(W, H)
        assert_bits(mean, acc["state"][0], f"{cfg} mean")
        assert_bits(m2, acc["state"][1], f"{cfg} m2")
        assert_bits(r.accum_state()[1], m2, f"{cfg} m2, the size taken from the stats")
        assert_bits(rgb, acc["resolved"], f"{cfg} resolved image")
        assert_bits(r.download_rgb(W, H), rgb, f"{cfg} the last image is the resolved one")
        assert_bits(rgb, oracle_tonemap(oracle, mean, TONE["exposure"], TONE["gamma"]), f"{cfg} tone map after the mean")
        assert (stats.est_mse, stats.mean_value, stats.nonfinite) == (acc["stats"].est_mse, acc["stats"].mean_value, 0)
        # the frame indices consumed: the next frame is the manual run's next frame (C3's has no predecessor in either)
        f = make(enable_tone_mapping=0)
        if not f.temporal_reuse:
            nxt, _ = r.render_restir(None, cam, W, H, f, want_grid=False)
            assert_bits(nxt, acc["next"], f"{cfg} frame {FRAMES}")
        else:
            r2 = new_renderer(sc)
            try:
                r2.set_seed(SEED, FRAMES)
                want, _ = r2.render_restir(None, cam, W, H, f, want_grid=False)
            finally:
                r2.close()
            nxt, _ = r.render_restir(None, cam, W, H, f, want_grid=False)
            assert_bits(nxt, want, f"{cfg} frame {FRAMES} without a predecessor")
        # the accumulation stays open
        r.accum_add()
        assert r.accum_stats().frames == FRAMES + 1
    finally:
        r.close()


def test_render_accumulate_request_errors(lib, nightclub):
    sc, cam = nightclub
    r = new_renderer(sc)
    try:
        f = c2()
        V = _abi.RESTIR_ACCUM_VARIANCE

        def call(**kw):
            req = _abi.AccumRequest(**kw)
            return lib.restir_render_accumulate(r.ctx, C.byref(cam), C.byref(f), W, H, None, C.byref(req), None, None)
        assert call(flags=V, max_frames=0) == INVALID
        assert call(flags=V, min_frames=3, max_frames=2) == INVALID
        assert call(flags=V, max_frames=4, target_mse=1e-3, check_every=0) == INVALID
        assert call(flags=0, max_frames=4, target_mse=1e-3, check_every=1) == INVALID   # a target needs the variance
        assert call(flags=2, max_frames=4) == INVALID
        assert lib.restir_render_accumulate(r.ctx, C.byref(cam), C.byref(f), W, H, None, None, None, None) == INVALID
        assert r.gbuf_reuses() == 0 and lib.restir_accum_add(r.ctx) == STATE   # nothing was rendered or begun
        assert call(flags=0, max_frames=1) == 0                                 # one frame, no variance: fine
        s = _abi.AccumStats()
        assert lib.restir_accum_stats_get(r.ctx, C.byref(s)) == STATE
    finally:
        r.close()


# ---- E: stats -------------------------------------------------------------------------------------------------------
def numpy_stats(mean, m2, n):
    """(est_mse, mean_value, nonfinite, tolerance of each): float64 over the state, the terms formed as the kernel forms
    them; the tolerance is the worst-case error bound of any summation order in double, count * 2^-52 * sum |term|, over
    the floats counted"""
    mean, m2 = mean.reshape(-1), m2.reshape(-1)
    ok = np.isfinite(mean) & np.isfinite(m2)
    terms = m2[ok].astype(np.float64) / (np.float64(n) * np.float64(n - 1))
    values = mean[ok].astype(np.float64)
    counted = int(ok.sum())
    bound = mean.size * 2.0 ** -52
    return (terms.sum() / counted, values.sum() / counted, int(mean.size - counted),
            bound * np.abs(terms).sum() / counted, bound * np.abs(values).sum() / counted)


def check_stats(s, mean, m2, n, what):
    est, val, bad, tol_e, tol_v = numpy_stats(mean, m2, n)
    print(f"{what}: est_mse {s.est_mse!r} want {est!r} tol {tol_e!r}; mean_value {s.mean_value!r} want {val!r} tol {tol_v!r}; "
          f"nonfinite {s.nonfinite} want {bad}")
    assert s.frames == n and s.nonfinite == bad, what
    assert abs(s.est_mse - est) <= tol_e, what
    assert abs(s.mean_value - val) <= tol_v, what


def test_stats_against_numpy(still):
    cfg, _, acc, _ = still
    check_stats(acc["stats"], acc["state"][0], acc["state"][1], FRAMES, f"{cfg} {W}x{H}")
    assert acc["stats"].est_mse > 0 and acc["stats"].mean_value > 0


@pytest.mark.parametrize("w,h", [(5, 3), (70, 37)])
def test_stats_leave_non_finite_entries_out(lib, w, h):
    r = restir.Renderer(0)
    try:
        r.stage_configure(w, h, 1)
        images = uploaded_images(w, h, 4, False)
        images[2][h // 2, w // 3, :] = np.nan          # one NaN pixel in one frame: its three floats stay NaN
        r.accum_begin(True)
        for x in images:
            r.upload(_abi.BUF_RGB, x)
            r.accum_add()
        mean, m2 = r.accum_state(w, h)
        s = r.accum_stats()
        assert s.nonfinite == 3 and (s.width, s.height) == (w, h)
        check_stats(s, mean, m2, 4, f"NaN pixel {w}x{h}")
        assert np.isfinite(s.est_mse) and np.isfinite(s.mean_value)
        again = r.accum_stats()                        # deterministic: the same bits every time
        assert (again.est_mse, again.mean_value, again.nonfinite) == (s.est_mse, s.mean_value, s.nonfinite)
    finally:
        r.close()


# ---- E (convergence), F: adaptive stop -----------------------------------------------------------------------------------
FIRST = 16   # the frame index the convergence runs start at


@pytest.fixture(scope="module")
def checkpoints(nightclub):
    """est_mse after 8, 16, ..., 64 frames of C2's still view, run by hand from frame index FIRST.

    The frames are heavy-tailed: a biased pass without visibility now and then hands a pixel a sample whose weight is
    thousands of times the image's mean (frame 23 of the default seed holds a value of 6,430 against a mean of 0.4), and
    est_mse is dominated by the few such values its frames hold.  It falls as 1 / n between them and jumps at each.  So
    which 64 frames are accumulated decides whether est_mse(64) < est_mse(16); the start was chosen on the CPU from the
    oracle's frames (bit-identical to the device's) folded by restir_accum_fold, est_mse after 8, 16, ..., 64 frames:
        from frame 0:   11.03  2.92 32.77 18.53 11.91  8.28  6.30  6.73   (frame 23 arrives after the 16th: it rises)
        from frame 16: 283.57 71.17 31.75 17.86 11.86 11.66  8.63  7.42   (frame 23 is among the first 8: it falls)"""
    sc, cam = nightclub
    f = c2(enable_tone_mapping=0)
    r = new_renderer(sc)
    try:
        r.set_seed(SEED, FIRST)
        r.accum_begin(True)
        est = {}
        for n in range(1, 65):
            r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)
            r.accum_add()
            if n % 8 == 0:
                est[n] = r.accum_stats().est_mse
        return est
    finally:
        r.close()


def test_est_mse_falls_with_more_frames(checkpoints):
    print({n: e for n, e in checkpoints.items()})
    assert checkpoints[64] < checkpoints[16]
    assert checkpoints[64] > 0


def test_adaptive_stop_ends_where_the_manual_run_predicts(checkpoints, nightclub):
    sc, cam = nightclub
    est = checkpoints
    # a target between two consecutive checkpoints, the later one the first to meet it
    pairs = [k for k in range(16, 64, 8) if est[k + 8] < min(est[n] for n in range(8, k + 8, 8))]
    assert pairs, f"no checkpoint undercuts all before it: {est}"
    k = pairs[0]
    target = 0.5 * (min(est[n] for n in range(8, k + 8, 8)) + est[k + 8])
    predicted = min(n for n in sorted(est) if est[n] <= target)
    assert predicted == k + 8
    r = new_renderer(sc)
    try:
        r.set_seed(SEED, FIRST)
        _, stats = r.render_accumulated(cam, W, H, c2(), 64, target_mse=target, min_frames=8, check_every=8, want_rgb=False)
        assert stats.frames == predicted
        assert stats.est_mse == est[predicted]            # same seed, same bits
        r.set_seed(SEED, FIRST)
        _, stats = r.render_accumulated(cam, W, H, c2(), predicted - 4, target_mse=target, min_frames=8, check_every=8,
                                        want_rgb=False)
        assert stats.frames == predicted - 4              # max_frames caps it
        r.set_seed(SEED, FIRST)
        _, stats = r.render_accumulated(cam, W, H, c2(), 64, target_mse=est[8], min_frames=8, check_every=8, want_rgb=False)
        assert stats.frames == 8                           # met at the first check
    finally:
        r.close()


# ---- G: state rules ---------------------------------------------------------------------------------------------------
def test_state_rules(lib, nightclub):
    sc, _ = nightclub
    w, h = 33, 17
    cam, cam2 = scene.camera_for(NAME, w, h), scene.camera_for(NAME, 70, 37)
    f = c2(enable_tone_mapping=0, spatial_resampling_passes=2)
    r = new_renderer(sc)

    def refused(call, what, state):
        """the call is RESTIR_ERR_STATE and the state (None: there is none to read) is as it was"""
        assert call() == STATE, what
        assert lib.restir_last_error(), what
        if state is None:
            assert lib.restir_accum_download(r.ctx, np.zeros(w * h * 3, F32).ctypes.data_as(FP), None, w * h * 3) == STATE, what
            return
        mean, m2 = r.accum_state(w, h)
        assert_bits(mean, state[0], what + ": mean")
        assert_bits(m2, state[1], what + ": m2")

    add = lambda: lib.restir_accum_add(r.ctx)
    stats = lambda: lib.restir_accum_stats_get(r.ctx, C.byref(_abi.AccumStats()))
    render = lambda c=cam, ww=w, hh=h: r.render_restir(None, c, ww, hh, f, want_rgb=False, want_grid=False)
    try:
        refused(add, "add before begin, nothing rendered", None)
        render()
        refused(add, "add before begin", None)
        refused(lambda: lib.restir_accum_resolve(r.ctx, None), "resolve before begin", None)
        r.accum_begin(True)
        refused(lambda: lib.restir_accum_resolve(r.ctx, None), "resolve with no frame", None)
        r.accum_add()                                   # the image rendered before the begin is a producer's
        state = r.accum_state(w, h)
        refused(add, "add twice after one render", state)
        refused(stats, "stats with one frame", state)
        r.accum_resolve(None)
        refused(add, "add after resolve", state)
        render(cam2, 70, 37)
        refused(add, "add after a render of another size", state)
        # a halo frame: between begin and end the image has its size but not its pixels
        tiles = (2, 1)
        t = restir.tile_plan(w, h, tiles[0], tiles[1], 0, f.spatial_resample_radius)
        r.halo_record(True)
        r.halo_begin(None, cam, w, h, f, tiles, 0)
        refused(add, "add between halo_begin and halo_end", state)
        assert b"halo" in lib.restir_last_error()
        for _ in range(f.spatial_resampling_passes):
            r.halo_pass()
        r.halo_end(t, False, False)
        r.halo_record(False)
        refused(add, "add of the halo tile's image: another size", state)
        render()
        r.accum_add()                                   # ... and the accumulation goes on
        assert r.accum_stats().frames == 2
        # without the variance there are no stats
        r.accum_begin(False)
        for _ in range(2):
            render()
            r.accum_add()
        state = r.accum_state(w, h)
        assert not state[1].any()
        refused(stats, "stats without the variance flag", state)
        assert lib.restir_accum_begin(r.ctx, 2) == INVALID   # unknown flags
        # a begin after all that works again, and an end closes
        r.accum_begin(True)
        render()
        r.accum_add()
        render()
        r.accum_add()
        assert r.accum_stats().frames == 2
        assert lib.restir_accum_download(r.ctx, np.zeros(4, F32).ctypes.data_as(FP), None, 4) == INVALID   # short buffer
        r.accum_end()
        render()
        refused(add, "add after end", None)
        r.accum_end()                                   # idempotent
    finally:
        r.close()
