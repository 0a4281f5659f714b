"""restir_denoise_lum on the device (include/restir_c.h "denoising with a variance-guided luminance term", csrc/denoise.h /
denoise.hip): the a-trous filter with a luminance term scaled by each pixel's measured noise.

1  RESTIR_DENOISE_VAR_SPATIAL equals restir_denoise_lum_host bit for bit, colour and the downloaded variance plane: the
   nightclub and Monkey at 33 x 17, 70 x 37 and 130 x 70, one to five levels; download_rgb agrees; with the tone fields the
   result is the tone map of the linear result;
2  RESTIR_DENOISE_VAR_ACCUM equals the host function fed restir_accum_download's mean and the plane computed from its m2 in
   numpy; the accumulation is untouched and goes on;
3  a lighting edge survives on the device where restir_denoise blurs it;
4  an uploaded image with NaN and inf pixels;
5  a 2 x 2 split denoised tile by tile equals the host function run per tile;
6  no side effects on frames, one guide trace per view across both calls, the result is served like a resolve;
7  every error leaves the image's bits alone;
8  it helps where restir_denoise hurts, confirmed on the CPU first.
GPU against the CPU; images are at most 130 x 70."""
import ctypes as C

import numpy as np
import pytest

import denoise_lum_spec as lspec
import exact_spec
from romis_amd import _abi, restir, scene
from test_gpu_denoise import CAMS, FP, FRAMES, LIN, MONKEY, SIZES, frame0, gbuffer, miss_of
from test_gpu_exact import NIGHT, SEED, assert_bits, bits, c2, c3, counters, oscene, spec_image, the_camera, the_scene

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 4
F32, U32 = np.float32, np.uint32
SPATIAL, ACCUM = _abi.RESTIR_DENOISE_VAR_SPATIAL, _abi.RESTIR_DENOISE_VAR_ACCUM
P = restir.denoise_lum_params


@pytest.fixture(scope="module")
def lib():
    from romis_amd import build
    build.build()
    return _abi.load_library()


@pytest.fixture(scope="module")
def gpu(lib):
    r = restir.Renderer(0)
    yield r
    r.close()


def accumulate(r, cam, w, h, n, first=0):
    """n linear C2 frames from frame index `first` on, each added to the open accumulation; the frames"""
    r.set_seed(SEED, first)
    frames = []
    for _ in range(n):
        frames.append(r.render_restir(None, cam, w, h, c2(**LIN), want_grid=False)[0])
        r.accum_add()
    return frames


# ---- 1: SPATIAL against the host ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHT, MONKEY])
def test_spatial_equals_the_host_function(gpu, oracle, name, w, h):
    gpu.set_scene(the_scene(name))
    cam = the_camera(name, CAMS[name], w, h)
    n_t, p_mat = gbuffer(oracle, name, w, h)
    for iterations in range(1, 6):
        raw = frame0(gpu, cam, w, h)
        p = P(iterations=iterations)
        got = gpu.denoise_lum(cam, w, h, params=p)
        want, want_v = restir.denoise_lum_host(raw, n_t, p_mat, miss_of(name), p)
        assert_bits(got, want, f"{name} {w}x{h}, {iterations} levels")
        assert_bits(gpu.denoise_lum_variance(), want_v, f"{name} {w}x{h}, {iterations} levels: the variance plane")
        assert_bits(gpu.download_rgb(w, h), got, f"{name} {w}x{h}: out_rgb against download_rgb")
        assert not np.array_equal(bits(got), bits(raw)) and want_v.max() > 0
    raw = frame0(gpu, cam, w, h)
    p = P(iterations=3, normal_power_log2=3, sigma_plane=0.1, sigma_lum=1.5)
    want, want_v = restir.denoise_lum_host(raw, n_t, p_mat, miss_of(name), p)
    assert_bits(gpu.denoise_lum(cam, w, h, params=p), want, f"{name} {w}x{h}: other parameters")
    assert_bits(gpu.denoise_lum_variance(), want_v, f"{name} {w}x{h}: other parameters, the variance plane")


@pytest.mark.parametrize("name,w,h", [(NIGHT, 70, 37), (MONKEY, 130, 70)])
def test_tone_mapping_follows_the_last_level(gpu, oracle, name, w, h):
    gpu.set_scene(the_scene(name))
    cam = the_camera(name, CAMS[name], w, h)
    n_t, p_mat = gbuffer(oracle, name, w, h)
    raw = frame0(gpu, cam, w, h)
    want, want_v = restir.denoise_lum_host(raw, n_t, p_mat, miss_of(name))
    for tone in (None, _abi.default_features(**LIN), _abi.default_features(gamma=1.0, exposure=1.0),
                 _abi.default_features(gamma=2.2, exposure=0.7)):
        assert_bits(frame0(gpu, cam, w, h), raw, "frame 0 again")
        got = gpu.denoise_lum(cam, w, h, tone=tone)
        assert_bits(gpu.denoise_lum_variance(), want_v, "the variance is the linear image's")
        if tone is None or not tone.enable_tone_mapping:
            assert_bits(got, want, f"{name} {w}x{h}: no tone mapping")
        else:
            assert_bits(got, exact_spec.tonemap(oracle, want, tone.exposure, tone.gamma), f"{name} {w}x{h}: gamma {tone.gamma}")
            assert got.min() >= 0.0 and got.max() <= 1.0 and not np.array_equal(bits(got), bits(want))


# ---- 2: ACCUM against the host --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(70, 37), (130, 70)])
def test_accum_equals_the_host_function(gpu, oracle, w, h):
    gpu.set_scene(the_scene(NIGHT))
    cam = scene.nightclub_camera(w, h)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    miss = miss_of(NIGHT)
    gpu.accum_begin(True)
    try:
        frames = accumulate(gpu, cam, w, h, 4)
        mean, m2 = gpu.accum_state(w, h)
        assert m2.max() > 0 and not np.array_equal(bits(mean), bits(frames[-1]))
        v0 = lspec.var_accum(m2, 4)
        assert v0.shape == (h, w) and (v0 > 0).sum() > w * h // 8
        for iterations in range(1, 6):
            p = P(iterations=iterations, variance_source=ACCUM, sigma_lum=2.0)
            got = gpu.denoise_lum(cam, w, h, params=p)   # (the last image: a frame at first, then the call's own result)
            want, want_v = restir.denoise_lum_host(mean, n_t, p_mat, miss, p, var=v0)
            assert_bits(got, want, f"{w}x{h}, {iterations} levels")
            assert_bits(gpu.denoise_lum_variance(), want_v, f"{w}x{h}, {iterations} levels: the variance plane")
            assert_bits(gpu.download_rgb(w, h), got, "download_rgb")
        # the accumulation is as it was, and goes on
        mean2, m22 = gpu.accum_state(w, h)
        assert_bits(mean2, mean, "the mean afterwards")
        assert_bits(m22, m2, "m2 afterwards")
        assert gpu.accum_stats().frames == 4
        with pytest.raises(_abi.RestirError, match="STATE"):
            gpu.accum_add()   # the result is no frame
        fifth = accumulate(gpu, cam, w, h, 1, first=4)[0]
        assert gpu.accum_stats().frames == 5
        restir.accum_fold(mean, m2, fifth, 5)
        mean5, m25 = gpu.accum_state(w, h)
        assert_bits(mean5, mean, "the mean of five")
        assert_bits(m25, m2, "m2 of five")
        # the input is what a resolve writes
        gpu.accum_resolve(None)
        assert_bits(gpu.download_rgb(w, h), mean, "the resolve")
    finally:
        gpu.accum_end()


def test_accum_after_an_image_of_another_size(gpu, oracle):
    """The mean is the input whatever the last image is: here a larger frame of another view came between."""
    w, h = 33, 17
    gpu.set_scene(the_scene(NIGHT))
    cam = scene.nightclub_camera(w, h)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    gpu.accum_begin(True)
    try:
        accumulate(gpu, cam, w, h, 3)
        mean, m2 = gpu.accum_state(w, h)
        frame0(gpu, scene.nightclub_camera(70, 37), 70, 37)
        p = P(variance_source=ACCUM)
        got = gpu.denoise_lum(cam, w, h, params=p)
        want, _ = restir.denoise_lum_host(mean, n_t, p_mat, miss_of(NIGHT), p, var=lspec.var_accum(m2, 3))
        assert_bits(got, want, "after a 70 x 37 frame")
        assert_bits(gpu.download_rgb(w, h), got, "the image has the accumulation's size now")
    finally:
        gpu.accum_end()


# ---- 3: the edge on the device --------------------------------------------------------------------------------------------
def test_a_lighting_edge_survives_on_the_device(gpu, oracle):
    w, h = 70, 37
    gpu.set_scene(the_scene(NIGHT))
    cam = scene.nightclub_camera(w, h)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    miss = miss_of(NIGHT)
    img = np.zeros((h, w, 3), F32)
    img[:, w // 2:] = 1.0
    old = restir.denoise_host(img, n_t, p_mat, miss, restir.denoise_params(iterations=2))
    old_moved = np.abs(old - img).max()
    print(f"restir_denoise_host moves the step image by up to {old_moved:.4f}")
    assert old_moved >= 0.25, "the edge crosses one surface in this view"
    gpu.accum_begin(True)
    try:
        for _ in range(2):
            gpu.stage_configure(w, h, 1)
            gpu.upload(_abi.BUF_RGB, img)
            gpu.accum_add()
        mean, m2 = gpu.accum_state(w, h)
        assert_bits(mean, img, "the mean of two equal images")
        assert not bits(m2).any()
        p = P(iterations=2, variance_source=ACCUM)
        got = gpu.denoise_lum(cam, w, h, params=p)
        want, want_v = restir.denoise_lum_host(img, n_t, p_mat, miss, p, var=np.zeros((h, w), F32))
        assert_bits(got, want, "the step, ACCUM")
        assert not bits(gpu.denoise_lum_variance()).any() and not bits(want_v).any()
        moved = np.abs(got - img).max()
        print(f"restir_denoise_lum moves it by up to {moved:.3e}")
        assert moved <= 1e-6
        gpu.stage_configure(w, h, 1)
        gpu.upload(_abi.BUF_RGB, img)
        assert_bits(gpu.denoise(cam, w, h, params=restir.denoise_params(iterations=2)), old, "restir_denoise on the step")
    finally:
        gpu.accum_end()


# ---- 4: NaN and inf ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_uploaded_image_with_nan_and_inf(gpu, oracle, w, h):
    gpu.set_scene(the_scene(NIGHT))
    cam = scene.nightclub_camera(w, h)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    n = 3 * w * h
    u = (np.arange(n, dtype=np.uint64) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    img = ((u >> 8).astype(F32) * F32(2.0 ** -22)).astype(F32).reshape(h, w, 3)
    bad = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFA55A5A], U32).view(F32)
    flat = img.reshape(-1)
    flat[(np.arange(len(bad)) * 131 + 7) % n] = bad
    flat[n - 1] = np.inf
    nonfinite = ~np.isfinite(img).all(axis=-1)
    assert 4 <= nonfinite.sum() <= 5
    for iterations in (1, 3, 5):
        gpu.stage_configure(w, h, 1)
        gpu.upload(_abi.BUF_RGB, img)
        p = P(iterations=iterations)
        got = gpu.denoise_lum(cam, w, h, params=p)
        want, want_v = restir.denoise_lum_host(img, n_t, p_mat, miss_of(NIGHT), p)
        assert_bits(got, want, f"uploaded {w}x{h}, {iterations} levels")
        assert_bits(gpu.denoise_lum_variance(), want_v, f"uploaded {w}x{h}, {iterations} levels: the variance plane")
        assert_bits(got[nonfinite], img[nonfinite], "the pixels that are not finite")
        assert np.isfinite(got[~nonfinite]).all() and not bits(want_v[nonfinite]).any()


# ---- 5: tiles ---------------------------------------------------------------------------------------------------------------
def test_tiles_equal_the_host_function_per_tile(gpu, oracle):
    gpu.set_scene(the_scene(NIGHT))
    w, h = 70, 37
    f = c2(**LIN)
    cam = scene.nightclub_camera(w, h)
    layout = restir.layout_even(w, h, 2, 2)
    p = P(iterations=2)
    frame0(gpu, cam, w, h)
    whole = gpu.denoise_lum(cam, w, h, params=p)
    out = np.full((h, w, 3), np.nan, F32)
    for rank in range(4):
        t = restir.tile_plan(w, h, 2, 2, rank, f.spatial_resample_radius, layout=layout)
        raw = frame0(gpu, cam, w, h, tile=t)
        got = gpu.denoise_lum(cam, w, h, tile=t, params=p)
        assert got.shape == (t.height, t.width, 3)
        n_t, p_mat = gbuffer(oracle, NIGHT, w, h, oracle.Rect(t.x0, t.y0, t.width, t.height))
        want, want_v = restir.denoise_lum_host(raw, n_t, p_mat, miss_of(NIGHT), p)
        assert_bits(got, want, f"tile {rank}")
        assert_bits(gpu.denoise_lum_variance(), want_v, f"tile {rank}: the variance plane")
        top = h - (t.y0 + t.height)
        out[top:top + t.height, t.x0:t.x0 + t.width] = got
    # away from the seams -- the variance estimate's 3 pixels, then the levels' 2 (2^2 - 1) = 6, and one more per level
    # as a bound on the pre-filter's reach -- the stitched image is the whole image's
    reach = 3 + 2 * (2 ** p.geo.iterations - 1) + p.geo.iterations
    xs, ys = layout.x_cuts[1], h - layout.y_cuts[0][1]
    far = np.ones((h, w), bool)
    far[:, max(0, xs - reach):xs + reach] = False
    far[max(0, ys - reach):ys + reach, :] = False
    assert far.any()
    assert_bits(out[far], whole[far], "stitched tiles away from the seams")
    assert not np.array_equal(bits(out), bits(whole)), "taps across a seam are skipped"


# ---- 6: no side effects; served like a resolve ------------------------------------------------------------------------------
def still_run(sc, cam, w, h, f, denoise):
    r = restir.Renderer(0)
    try:
        r.set_scene(sc)
        r.set_seed(SEED, 0)
        out = dict(images=[], grids=[], denoised=[])
        prev = None
        for k in range(FRAMES):
            rgb, grid = r.render_restir(prev if f.temporal_reuse else None, cam, w, h, f, want_grid=True)
            out["images"].append(rgb)
            out["grids"].append([np.asarray(a).copy() for a in grid.download()])
            prev = grid
            if denoise:
                tone = _abi.default_features() if k % 2 else None
                if k in (1, 4):   # the old call between the new one's
                    out["denoised"].append(r.denoise(cam, w, h, params=restir.denoise_params(iterations=1 + k % 5), tone=tone))
                else:
                    out["denoised"].append(r.denoise_lum(cam, w, h, params=P(iterations=1 + k % 5), tone=tone, download=k % 3 != 2))
        out["counters"] = counters(r)
        out["guide_builds"] = r.denoise_guide_builds()
        return out
    finally:
        r.close()


@pytest.mark.parametrize("cfg", ["c2", "c3"])
def test_denoising_changes_no_frame_and_no_cache(oracle, cfg):
    w, h = 70, 37
    sc, cam = the_scene(NIGHT), scene.nightclub_camera(w, h)
    f = dict(c2=c2, c3=c3)[cfg](**LIN)
    plain, mixed = still_run(sc, cam, w, h, f, False), still_run(sc, cam, w, h, f, True)
    for k in range(FRAMES):
        assert_bits(mixed["images"][k], plain["images"][k], f"{cfg} frame {k} image")
        for j, (a, b) in enumerate(zip(mixed["grids"][k], plain["grids"][k])):
            assert_bits(a.view(F32), b.view(F32), f"{cfg} frame {k} grid plane {j}")
    assert mixed["counters"] == plain["counters"], cfg
    assert plain["counters"]["gbuf_reuses"] == FRAMES - 1 and plain["counters"]["phat_builds"] == 1   # the still view's routes ran
    assert (plain["guide_builds"], mixed["guide_builds"]) == (0, 1), "one trace per view across both calls"
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    assert [d is None for d in mixed["denoised"]] == [k % 3 == 2 and k not in (1, 4) for k in range(FRAMES)]
    for k in (0, 3):   # one level, linear (k = 0) and four levels, tone mapped (k = 3)
        want, _ = restir.denoise_lum_host(mixed["images"][k], n_t, p_mat, miss_of(NIGHT), P(iterations=1 + k % 5))
        if k % 2:
            want = exact_spec.tonemap(oracle, want, _abi.default_features().exposure, _abi.default_features().gamma)
        assert_bits(mixed["denoised"][k], want, f"{cfg}: the denoised frame {k}")
    want = restir.denoise_host(mixed["images"][4], n_t, p_mat, miss_of(NIGHT), restir.denoise_params(iterations=5))
    assert_bits(mixed["denoised"][4], want, f"{cfg}: restir_denoise over the guides restir_denoise_lum traced")


def test_result_is_served_like_a_resolve(lib, oracle):
    w, h = 33, 17
    cam = scene.nightclub_camera(w, h)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    miss = miss_of(NIGHT)
    r = restir.Renderer(0)
    try:
        r.set_scene(the_scene(NIGHT))
        # the stage API is left unconfigured
        r.stage_configure(w, h, 1)
        r.upload(_abi.BUF_RGB, np.ones((h, w, 3), F32))
        r.denoise_lum(cam, w, h, download=False)
        with pytest.raises(_abi.RestirError, match="STATE"):
            r.download(_abi.BUF_RGB)
        raw = frame0(r, cam, w, h)
        tone = _abi.default_features(gamma=2.2)
        assert r.denoise_lum(cam, w, h, tone=tone, download=False) is None
        img = r.download_rgb(w, h)
        lin, _ = restir.denoise_lum_host(raw, n_t, p_mat, miss)
        assert_bits(img, exact_spec.tonemap(oracle, lin, tone.exposure, 2.2), "enqueue only")
        rgba = np.zeros((h, w, 4), np.uint8)
        assert lib.restir_rgb_to_rgba8(img.ctypes.data, w * h, rgba.ctypes.data) == 0
        assert np.array_equal(r.download_rgba8(w, h), rgba)
        with r.present("rgb32f") as im:
            assert_bits(im.wait(), img, "present rgb32f")
        r.reference_set()
        e = r.error("image")
        assert e.counted == 3 * w * h and e.max_abs == 0.0
        r.accum_begin(False)
        assert lib.restir_accum_add(r.ctx) == STATE
        assert_bits(r.download_rgb(w, h), img, "the image after the refused add")
        r.accum_end()
        # a second call filters the first one's output; restir_denoise serves it too
        frame0(r, cam, w, h)
        r.denoise_lum(cam, w, h, download=False)
        twice = r.denoise_lum(cam, w, h, params=P(iterations=1))
        assert_bits(twice, restir.denoise_lum_host(lin, n_t, p_mat, miss, P(iterations=1))[0], "a second call")
        assert_bits(r.denoise(cam, w, h), restir.denoise_host(twice, n_t, p_mat, miss), "restir_denoise of the result")
        # no frame index is consumed
        assert_bits(frame0(r, cam, w, h), raw, "frame 0 after denoising")
        assert r.denoise_guide_builds() == 1
    finally:
        r.close()


# ---- 7: errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_image_alone(lib):
    w, h = 33, 17
    cam = scene.nightclub_camera(w, h)
    f = c2(spatial_resampling_passes=2, **LIN)
    out = np.full((h, w, 3), 7.0, F32)
    r = restir.Renderer(0)

    def call(cam_=cam, w_=w, h_=h, tile=None, p=P(), ctx=True):
        return lib.restir_denoise_lum(r.ctx if ctx else None, C.byref(cam_) if cam_ is not None else None, w_, h_,
                                      C.byref(tile) if tile is not None else None, C.byref(p) if p is not None else None, None,
                                      out.ctypes.data_as(FP))

    def with_flags(geo=0, own=0):
        p = P()
        p.geo.flags, p.flags = geo, own
        return p
    try:
        assert call() == STATE and b"restir_set_scene" in lib.restir_last_error()     # no scene
        r.set_scene(the_scene(NIGHT))
        assert call() == STATE and b"nothing rendered" in lib.restir_last_error()     # no image
        r.stage_configure(w, h, 1)
        assert call() == STATE                                                        # a buffer without pixels
        last = frame0(r, cam, w, h)
        var = np.full(w * h, 5.0, F32)

        def refused(code, what, **kw):
            assert call(**kw) == code, what
            message = lib.restir_last_error()
            assert message, what
            assert (out == 7.0).all(), what
            assert_bits(r.download_rgb(w, h), last, what + ": the last image")
            assert r.denoise_guide_builds() == 0, what
            assert lib.restir_denoise_lum_variance_download(r.ctx, var.ctypes.data_as(FP), var.size) == STATE, what
            assert (var == 5.0).all(), what
            return message

        refused(INVALID, "a NULL context", ctx=False)
        refused(INVALID, "a NULL camera", cam_=None)
        refused(INVALID, "NULL parameters", p=None)
        refused(INVALID, "no level", p=P(iterations=0))
        refused(INVALID, "six levels", p=P(iterations=6))
        refused(INVALID, "a normal exponent of 2^8", p=P(normal_power_log2=8))
        refused(INVALID, "sigma_plane 0", p=P(sigma_plane=0.0))
        refused(INVALID, "sigma_plane NaN", p=P(sigma_plane=float("nan")))
        refused(INVALID, "geo.flags", p=with_flags(geo=2))
        refused(INVALID, "flags", p=with_flags(own=1))
        refused(INVALID, "an unknown variance source", p=P(variance_source=2))
        refused(INVALID, "sigma_lum 0", p=P(sigma_lum=0.0))
        refused(INVALID, "sigma_lum < 0", p=P(sigma_lum=-4.0))
        refused(INVALID, "sigma_lum NaN", p=P(sigma_lum=float("nan")))
        refused(INVALID, "sigma_lum inf", p=P(sigma_lum=float("inf")))
        refused(INVALID, "an empty image", w_=0)
        refused(INVALID, "a tile of another image", tile=restir.tile_plan(70, 37, 2, 2, 0, 0))
        assert b"33x17" in refused(STATE, "another size", w_=70, h_=37)
        refused(STATE, "a tile smaller than the image", tile=restir.tile_plan(w, h, 2, 1, 0, 0))
        # ACCUM's state
        acc = P(variance_source=ACCUM)
        refused(STATE, "ACCUM without an accumulation", p=acc)
        r.accum_begin(False)
        r.accum_add()
        last = frame0(r, cam, w, h)
        r.accum_add()
        assert b"RESTIR_ACCUM_VARIANCE" in refused(STATE, "ACCUM without the variance", p=acc)
        r.accum_begin(True)
        refused(STATE, "ACCUM with no frame", p=acc)
        last = frame0(r, cam, w, h)
        r.accum_add()
        refused(STATE, "ACCUM with one frame", p=acc)
        r.set_seed(SEED, 1)
        last = r.render_restir(None, cam, w, h, c2(**LIN), want_grid=False)[0]
        r.accum_add()
        mean, m2 = r.accum_state(w, h)
        refused(STATE, "ACCUM with another size", p=acc, w_=70, h_=37)
        refused(STATE, "ACCUM with a tile smaller than the accumulation", p=acc, tile=restir.tile_plan(w, h, 2, 1, 0, 0))
        again = r.accum_state(w, h)
        assert_bits(again[0], mean, "the mean after the refused calls")
        assert_bits(again[1], m2, "m2 after the refused calls")
        assert r.accum_stats().frames == 2
        r.accum_end()
        # the variance hook's own arguments
        assert call() == 0
        assert lib.restir_denoise_lum_variance_download(r.ctx, var.ctypes.data_as(FP), var.size - 1) == INVALID
        assert lib.restir_denoise_lum_variance_download(r.ctx, None, var.size) == INVALID
        assert (var == 5.0).all()
        assert lib.restir_denoise_lum_variance_download(r.ctx, var.ctypes.data_as(FP), var.size) == 0 and (var != 5.0).all()
        # between halo_begin and halo_end
        out[:] = 7.0
        r.halo_record(True)
        r.halo_begin(None, cam, w, h, f, (2, 1), 0)
        assert call() == STATE and b"halo" in lib.restir_last_error()
        assert (out == 7.0).all() and r.denoise_guide_builds() == 1
        for _ in range(f.spatial_resampling_passes):
            r.halo_pass()
        r.halo_end(restir.tile_plan(w, h, 2, 1, 0, f.spatial_resample_radius), False, False)
        r.halo_record(False)
        assert call() == STATE, "the halo frame's tile has not the size asked for"
        assert (out == 7.0).all()
    finally:
        r.close()


# ---- 8: it helps --------------------------------------------------------------------------------------------------------------
def test_it_helps_where_the_old_filter_hurts(gpu, oracle):
    """130 x 70, C2, the defaults, every figure against the exact image; strict inequalities, no tolerance, on the CPU first
    (the oracle's frames, the host functions, the specification's exact image), then the device's restir_error_get figures
    must equal the CPU's exactly.
    One frame, two levels:  rel_mse(lum) < rel_mse(restir_denoise)  and  mse(lum) < mse(raw).
    Mean of 16 frames, ACCUM, one level:  rel_mse(lum) < rel_mse(raw mean) < rel_mse(restir_denoise).
    When this was written: 0.2944 < 1.2560 and 2.7271 < 10.1172; 0.05219 < 0.06949 < 0.29406."""
    w, h = 130, 70
    cam = scene.nightclub_camera(w, h)
    lin = _abi.default_features(**LIN)
    miss = miss_of(NIGHT)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    exact = spec_image(oracle, NIGHT, None, w, h, lin)
    err = lambda img: restir.error_measure(img, exact)   # noqa: E731
    oframes = [oracle.render_frame(oscene(oracle, NIGHT), cam, c2(**LIN), w, h, SEED, k)[0] for k in range(16)]

    # one frame, the defaults at two levels
    one = P(iterations=2)
    old2 = restir.denoise_params(iterations=2)
    cpu = dict(raw=err(oframes[0]), old=err(restir.denoise_host(oframes[0], n_t, p_mat, miss, old2)),
               lum=err(restir.denoise_lum_host(oframes[0], n_t, p_mat, miss, one)[0]))
    for k, e in cpu.items():
        print(f"one frame, {k}: mse {e.mse:.4f} rel_mse {e.rel_mse:.4f}")
    assert cpu["lum"].rel_mse < cpu["old"].rel_mse
    assert cpu["lum"].mse < cpu["raw"].mse

    # the mean of 16, one level
    mean, m2 = np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32)
    for k, x in enumerate(oframes):
        restir.accum_fold(mean, m2, x, k + 1)
    acc = P(iterations=1, variance_source=ACCUM)
    old1 = restir.denoise_params(iterations=1)
    cpu16 = dict(raw=err(mean), old=err(restir.denoise_host(mean, n_t, p_mat, miss, old1)),
                 lum=err(restir.denoise_lum_host(mean, n_t, p_mat, miss, acc, var=lspec.var_accum(m2, 16))[0]))
    for k, e in cpu16.items():
        print(f"mean of 16, {k}: mse {e.mse:.4f} rel_mse {e.rel_mse:.5f}")
    assert cpu16["lum"].rel_mse < cpu16["raw"].rel_mse < cpu16["old"].rel_mse

    def figures(e):
        return (e.mse, e.rel_mse, e.mae, e.bias)

    gpu.set_scene(the_scene(NIGHT))
    assert_bits(gpu.render_exact(cam, w, h, lin), exact, "the exact image")
    gpu.reference_set()
    try:
        assert_bits(frame0(gpu, cam, w, h), oframes[0], "the frame")
        assert figures(gpu.error("image")) == figures(cpu["raw"])
        gpu.denoise(cam, w, h, params=old2, download=False)
        dev_old = gpu.error("image")
        frame0(gpu, cam, w, h)
        gpu.denoise_lum(cam, w, h, params=one, download=False)
        dev_lum = gpu.error("image")
        print(f"one frame on the device: rel_mse {dev_old.rel_mse:.4f} (restir_denoise) {dev_lum.rel_mse:.4f} (lum)")
        assert figures(dev_old) == figures(cpu["old"]) and figures(dev_lum) == figures(cpu["lum"])
        assert dev_lum.rel_mse < dev_old.rel_mse and dev_lum.mse < cpu["raw"].mse

        gpu.accum_begin(True)
        frames = accumulate(gpu, cam, w, h, 16)
        assert_bits(frames[15], oframes[15], "frame 15")
        dev_raw = gpu.error("accum")
        gpu.denoise_lum(cam, w, h, params=acc, download=False)
        dev_lum = gpu.error("image")
        gpu.accum_resolve(None)
        gpu.denoise(cam, w, h, params=old1, download=False)
        dev_old = gpu.error("image")
        print(f"mean of 16 on the device: rel_mse {dev_lum.rel_mse:.5f} (lum) {dev_raw.rel_mse:.5f} (raw) {dev_old.rel_mse:.5f} (restir_denoise)")
        assert (figures(dev_raw), figures(dev_old), figures(dev_lum)) == (figures(cpu16["raw"]), figures(cpu16["old"]), figures(cpu16["lum"]))
        assert dev_lum.rel_mse < dev_raw.rel_mse < dev_old.rel_mse
    finally:
        gpu.accum_end()
        gpu.reference_clear()
