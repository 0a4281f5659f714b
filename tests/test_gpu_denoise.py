"""restir_denoise on the device (include/restir_c.h "denoising the last image", csrc/denoise.h / denoise.hip): the
edge-avoiding a-trous filter over the context's last image.

A  bit-exact, no tolerance, against restir_denoise_host fed the oracle's G-buffer of the view and the frame the device
   rendered: 33 x 17, 70 x 37 and 130 x 70 (the last has a second lattice tile at step 4; at 70 x 37 with five levels
   most taps of step 16 fall outside the image), the 128-light nightclub and Monkey (curved normals, a BVH past the LDS
   budget for the guide trace), one to five levels; tone mapping off and on at two gammas, the tone-mapped image against
   or_tonemap of the host function's; an uploaded image with NaN and inf through RESTIR_BUF_RGB;
B  a 2 x 2 split denoised tile by tile equals the host function run per tile;
C  no side effects on frames: seven C2 and seven C3 still frames with a denoise after each equal, bit for bit and counter
   for counter, a context's that never denoises;
D  the result is served like a resolve and refused by accum_add; a second denoise and a denoise of a resolve work;
E  the guides are traced once per view, again after another camera, update_meshes and set_scene, not after set_lights;
F  every error leaves the image's bits alone;
G  it helps: the C2 frame's true MSE against the exact image falls, confirmed on the CPU first.
GPU against the CPU; images are at most 130 x 70."""
import ctypes as C

import numpy as np
import pytest

import exact_spec
from romis_amd import _abi, restir, scene
from test_gpu_dynamic_scene import NIGHT_BOX, toward_camera, with_positions
from test_gpu_exact import NIGHT, SEED, assert_bits, bits, c2, c3, counters, oscene, spec_image, the_camera, the_scene
from test_gpu_scene_shapes import LDS_BUDGET

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 4
F32, U32 = np.float32, np.uint32
FP = C.POINTER(C.c_float)
SIZES = [(33, 17), (70, 37), (130, 70)]
MONKEY = "monkey16"
CAMS = {NIGHT: None, MONKEY: "toml"}
LIN = dict(enable_tone_mapping=0)


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


_gbufs = {}


def gbuffer(oracle, name, w, h, view=None):
    """the oracle's (n_t, p_mat) of the view, computed once"""
    k = (name, w, h, None if view is None else (view.x0, view.y0, view.w, view.h))
    if k not in _gbufs:
        n_t, p_mat = oracle.gbuffer(oscene(oracle, name), the_camera(name, CAMS[name], w, h), w, h, view)
        n_t.flags.writeable = p_mat.flags.writeable = False
        _gbufs[k] = (n_t, p_mat)
    return _gbufs[k]


def miss_of(name):
    return len(the_scene(name).meshes)


def frame0(r, cam, w, h, f=None, tile=None):
    """frame 0 of the C2 configuration, linear, as the context's image"""
    r.set_seed(SEED, 0)
    return r.render_restir(None, cam, w, h, f or c2(**LIN), tile=tile, want_grid=False)[0]


# ---- A: bit-exact against the host function -----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHT, MONKEY])
def test_equals_the_host_function(gpu, oracle, name, w, h):
    gpu.set_scene(the_scene(name))
    info = gpu.scene_info()
    if name == MONKEY:
        assert info.bvh_lds_bytes > LDS_BUDGET, f"the BVH takes {info.bvh_lds_bytes} bytes: it fits LDS"
    cam = the_camera(name, CAMS[name], w, h)
    n_t, p_mat = gbuffer(oracle, name, w, h)
    hit = bits(p_mat[:, 3]) != miss_of(name)
    assert hit.sum() >= 32 and (~hit).sum() >= 32, "the view sees surface and background"
    if name == MONKEY:   # curved: many distinct normals among the hits
        assert len(np.unique(bits(n_t[hit, :3]), axis=0)) >= hit.sum() // 4
    if (w, h) == (130, 70):
        assert (w + 3) // 4 > 32, "a second lattice tile at step 4"
    for iterations in range(1, 6):
        raw = frame0(gpu, cam, w, h)
        assert raw.var() > 0
        p = restir.denoise_params(iterations=iterations)
        got = gpu.denoise(cam, w, h, params=p)
        want = restir.denoise_host(raw, n_t, p_mat, miss_of(name), p)
        assert_bits(got, want, f"{name} {w}x{h}, {iterations} levels")
        assert_bits(gpu.download_rgb(w, h), got, f"{name} {w}x{h}: out_rgb against download_rgb")
        assert not np.array_equal(bits(got), bits(raw))
    if name == MONKEY:   # where normals curve, the exponent and the plane term's support decide weights
        raw = frame0(gpu, cam, w, h)
        seen = [restir.denoise_host(raw, n_t, p_mat, miss_of(name), restir.denoise_params(iterations=2))]
        for power, sigma in [(0, 0.1), (7, 0.003), (3, 1.0)]:
            assert_bits(frame0(gpu, cam, w, h), raw, "frame 0 again")
            p = restir.denoise_params(2, power, sigma)
            want = restir.denoise_host(raw, n_t, p_mat, miss_of(name), p)
            assert_bits(gpu.denoise(cam, w, h, params=p), want, f"{name} {w}x{h}, exponent 2^{power}, sigma {sigma}")
            assert all(not np.array_equal(bits(want), bits(s)) for s in seen), "the parameters matter in this view"
            seen.append(want)
    assert gpu.denoise_guide_builds() >= 1


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHT, MONKEY])
def test_tone_mapping_follows_the_last_level(gpu, oracle, name, w, h):
    gpu.set_scene(the_scene(name))
    cam = the_camera(name, CAMS[name], w, h)
    n_t, p_mat = gbuffer(oracle, name, w, h)
    raw = frame0(gpu, cam, w, h)
    want = restir.denoise_host(raw, n_t, p_mat, miss_of(name))
    for tone in (None, _abi.default_features(**LIN), _abi.default_features(gamma=1.0, exposure=1.0),
                 _abi.default_features(gamma=2.2, exposure=0.7)):
        assert_bits(frame0(gpu, cam, w, h), raw, "frame 0 again")
        got = gpu.denoise(cam, w, h, tone=tone)
        if tone is None or not tone.enable_tone_mapping:
            assert_bits(got, want, f"{name} {w}x{h}: no tone mapping")
        else:
            toned = exact_spec.tonemap(oracle, want, tone.exposure, tone.gamma)
            assert_bits(got, toned, f"{name} {w}x{h}: gamma {tone.gamma}")
            assert got.min() >= 0.0 and got.max() <= 1.0 and not np.array_equal(bits(got), bits(want))


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
        p = restir.denoise_params(iterations=iterations)
        got = gpu.denoise(cam, w, h, params=p)
        assert_bits(got, restir.denoise_host(img, n_t, p_mat, miss_of(NIGHT), p), f"uploaded {w}x{h}, {iterations} levels")
        assert_bits(got[nonfinite], img[nonfinite], "the pixels that are not finite")
        assert np.isfinite(got[~nonfinite]).all()


# ---- B: tiles -----------------------------------------------------------------------------------------------------------
def test_tiles_equal_the_host_function_per_tile(gpu, oracle):
    gpu.set_scene(the_scene(NIGHT))
    w, h = 70, 37
    f = c2(**LIN)
    cam = scene.nightclub_camera(w, h)
    layout = restir.layout_even(w, h, 2, 2)
    p = restir.denoise_params(iterations=3)
    whole_raw = frame0(gpu, cam, w, h)
    whole = gpu.denoise(cam, w, h, params=p)
    out = np.full((h, w, 3), np.nan, F32)
    for rank in range(4):
        t = restir.tile_plan(w, h, 2, 2, rank, f.spatial_resample_radius, layout=layout)
        raw = frame0(gpu, cam, w, h, tile=t)
        top = h - (t.y0 + t.height)
        assert_bits(raw, whole_raw[top:top + t.height, t.x0:t.x0 + t.width], f"tile {rank}: the frame")
        got = gpu.denoise(cam, w, h, tile=t, params=p)
        assert got.shape == (t.height, t.width, 3)
        n_t, p_mat = gbuffer(oracle, NIGHT, w, h, oracle.Rect(t.x0, t.y0, t.width, t.height))
        assert_bits(got, restir.denoise_host(raw, n_t, p_mat, miss_of(NIGHT), p), f"tile {rank}")
        out[top:top + t.height, t.x0:t.x0 + t.width] = got
    # away from the seams -- 2 (2^3 - 1) = 14 pixels -- the stitched image is the whole image's
    reach = 2 * (2 ** p.iterations - 1)
    xs, ys = layout.x_cuts[1], h - layout.y_cuts[0][1]
    far = np.ones((h, w), bool)
    far[:, max(0, xs - reach):xs + reach] = False
    far[max(0, ys - reach):ys + reach, :] = False
    assert far.any()
    assert_bits(out[far], whole[far], "stitched tiles away from the seams")
    assert not np.array_equal(bits(out), bits(whole)), "taps across a seam are skipped"


# ---- C: no side effects -------------------------------------------------------------------------------------------------
FRAMES = 7


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
                out["denoised"].append(r.denoise(cam, w, h, params=restir.denoise_params(iterations=1 + k % 5),
                                                 tone=_abi.default_features() if k % 2 else None, download=k % 3 != 2))
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
    assert not np.array_equal(bits(plain["images"][0]), bits(plain["images"][1]))   # independent frames
    assert mixed["counters"] == plain["counters"], cfg
    assert plain["counters"]["gbuf_reuses"] == FRAMES - 1 and plain["counters"]["phat_builds"] == 1   # the still view's routes ran
    assert (plain["guide_builds"], mixed["guide_builds"]) == (0, 1)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    assert [d is None for d in mixed["denoised"]] == [k % 3 == 2 for k in range(FRAMES)]
    for k in (0, 3):   # one level, linear (k = 0) and four levels, tone mapped (k = 3)
        want = restir.denoise_host(mixed["images"][k], n_t, p_mat, miss_of(NIGHT), restir.denoise_params(iterations=1 + k % 5))
        if k % 2:
            want = exact_spec.tonemap(oracle, want, _abi.default_features().exposure, _abi.default_features().gamma)
        assert_bits(mixed["denoised"][k], want, f"{cfg}: the denoised frame {k}")


# ---- D: served like a resolve ------------------------------------------------------------------------------------------
def test_result_is_served_like_a_resolve(lib, oracle, tmp_path):
    w, h = 33, 17
    cam = scene.nightclub_camera(w, h)
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    miss = miss_of(NIGHT)
    r = restir.Renderer(0)
    try:
        r.set_scene(the_scene(NIGHT))
        raw = frame0(r, cam, w, h)
        tone = _abi.default_features(gamma=2.2)
        img = r.denoise(cam, w, h, tone=tone, download=False)
        assert img is None
        img = r.download_rgb(w, h)
        assert_bits(img, exact_spec.tonemap(oracle, restir.denoise_host(raw, n_t, p_mat, miss), tone.exposure, 2.2), "enqueue only")
        # present and write_bmp serve it
        rgba = np.zeros((h, w, 4), np.uint8)
        assert lib.restir_rgb_to_rgba8(img.ctypes.data, w * h, rgba.ctypes.data) == 0
        assert np.array_equal(r.download_rgba8(w, h), rgba)
        with r.present("rgba8") as im:
            assert (im.width, im.height) == (w, h) and np.array_equal(im.wait().reshape(h, w, 4), rgba)
        with r.present("rgb32f") as im:
            assert_bits(im.wait(), img, "present rgb32f")
        a, b = tmp_path / "device.bmp", tmp_path / "host.bmp"
        r.write_bmp(a)
        assert lib.restir_write_bmp(str(b).encode(), img.ctypes.data, w, h) == 0
        assert a.read_bytes() == b.read_bytes()
        # reference_set and error accept it; accum_add refuses it
        r.reference_set()
        assert r.reference_info() == (w, h, True)
        e = r.error("image")
        assert e.counted == 3 * w * h and e.max_abs == 0.0
        r.accum_begin(False)
        assert lib.restir_accum_add(r.ctx) == STATE and b"restir_denoise" in lib.restir_last_error()
        assert_bits(r.download_rgb(w, h), img, "the image after the refused add")
        # a second denoise filters the first one's output
        lin = restir.denoise_host(raw, n_t, p_mat, miss)
        frame0(r, cam, w, h)
        r.denoise(cam, w, h, download=False)
        twice = r.denoise(cam, w, h, params=restir.denoise_params(iterations=2))
        assert_bits(twice, restir.denoise_host(lin, n_t, p_mat, miss, restir.denoise_params(iterations=2)), "a second denoise")
        assert r.error("image").mse > 0.0
        # an accumulation's resolve
        r.set_seed(SEED, 0)
        frames = []
        for _ in range(3):
            frames.append(r.render_restir(None, cam, w, h, c2(**LIN), want_grid=False)[0])
            r.accum_add()
        r.accum_resolve(None)
        mean = r.download_rgb(w, h)
        assert not np.array_equal(bits(mean), bits(frames[-1]))
        got = r.denoise(cam, w, h)
        assert_bits(got, restir.denoise_host(mean, n_t, p_mat, miss), "a resolve, denoised")
        assert lib.restir_accum_add(r.ctx) == STATE
        r.accum_end()
        # no frame index is consumed: the next frame is frame 0's
        first = frame0(r, cam, w, h)
        r.denoise(cam, w, h, download=False)
        assert_bits(first, raw, "frame 0 after denoising")
        assert r.denoise_guide_builds() == 1
    finally:
        r.close()


def test_the_stage_api_is_left_unconfigured(gpu):
    gpu.set_scene(the_scene(NIGHT))
    w, h = 33, 17
    gpu.stage_configure(w, h, 1)
    gpu.upload(_abi.BUF_RGB, np.ones((h, w, 3), F32))
    gpu.denoise(scene.nightclub_camera(w, h), w, h, download=False)
    with pytest.raises(_abi.RestirError, match="STATE"):
        gpu.download(_abi.BUF_RGB)
    gpu.stage_configure(w, h, 1)
    assert gpu.download(_abi.BUF_RGB).size == w * h * 3


# ---- E: the guides are kept ----------------------------------------------------------------------------------------------
def test_guides_are_traced_once_per_view(oracle):
    w, h = 70, 37
    sc = the_scene(NIGHT)
    cam, cam2 = scene.nightclub_camera(w, h), scene.make_camera(30.0, 24.0, (2.57, 1.23, -1.35), (10.3, 31.0, 0.0), w, h)
    miss = miss_of(NIGHT)
    r = restir.Renderer(0)
    try:
        r.set_scene(sc)
        assert r.denoise_guide_builds() == 0
        for k in range(3):
            frame0(r, cam, w, h)
            r.denoise(cam, w, h, params=restir.denoise_params(iterations=1 + k, sigma_plane=0.01 * (1 + k)))
            assert r.denoise_guide_builds() == 1, "a still view, whatever the parameters"
        raw = frame0(r, cam2, w, h)
        got = r.denoise(cam2, w, h)
        assert r.denoise_guide_builds() == 2, "another camera"
        n_t2, p_mat2 = oracle.gbuffer(oscene(oracle, NIGHT), cam2, w, h)
        assert_bits(got, restir.denoise_host(raw, n_t2, p_mat2, miss), "the second camera's guides")
        r.set_lights(the_scene("pt3").lights)
        frame0(r, cam2, w, h)
        r.denoise(cam2, w, h, download=False)
        assert r.denoise_guide_builds() == 2, "new lights leave the geometry alone"
        r.set_lights(sc.lights)
        # another size and a tile are other views
        frame0(r, scene.nightclub_camera(33, 17), 33, 17)
        r.denoise(scene.nightclub_camera(33, 17), 33, 17, download=False)
        assert r.denoise_guide_builds() == 3
        # update_meshes: the box moves towards the camera
        p1 = toward_camera(oracle, sc, cam, NIGHT_BOX, 0.35)
        moved = with_positions(sc, p1)
        frame0(r, cam, w, h)
        r.denoise(cam, w, h, download=False)
        assert r.denoise_guide_builds() == 4
        r.update_meshes({NIGHT_BOX: (p1[NIGHT_BOX], None)})
        raw = frame0(r, cam, w, h)
        got = r.denoise(cam, w, h)
        assert r.denoise_guide_builds() == 5, "update_meshes drops the guides"
        fresh = restir.Renderer(0)
        try:
            fresh.set_scene(moved)
            assert_bits(frame0(fresh, cam, w, h), raw, "the moved scene's frame")
            assert_bits(got, fresh.denoise(cam, w, h), "after update_meshes against a fresh context")
        finally:
            fresh.close()
        n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
        before = restir.denoise_host(raw, n_t, p_mat, miss)
        assert not np.array_equal(bits(got), bits(before)), "the moved box changes the guides"
        r.set_scene(moved)
        frame0(r, cam, w, h)
        r.denoise(cam, w, h, download=False)
        assert r.denoise_guide_builds() == 6, "set_scene drops the guides"
    finally:
        r.close()


# ---- F: errors ----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_image_alone(lib):
    w, h = 33, 17
    cam = scene.nightclub_camera(w, h)
    f = c2(spatial_resampling_passes=2, **LIN)
    out = np.full((h, w, 3), 7.0, F32)
    r = restir.Renderer(0)

    def call(cam_=cam, w_=w, h_=h, tile=None, p=restir.denoise_params(), ctx=True):
        return lib.restir_denoise(r.ctx if ctx else None, C.byref(cam_) if cam_ is not None else None, w_, h_,
                                  C.byref(tile) if tile is not None else None, C.byref(p) if p is not None else None, None,
                                  out.ctypes.data_as(FP))
    try:
        assert call() == STATE and b"restir_set_scene" in lib.restir_last_error()     # no scene
        r.set_scene(the_scene(NIGHT))
        assert call() == STATE and b"nothing rendered" in lib.restir_last_error()     # no image
        r.stage_configure(w, h, 1)
        assert call() == STATE                                                        # a buffer without pixels
        last = frame0(r, cam, w, h)

        def refused(code, what, **kw):
            assert call(**kw) == code, what
            assert lib.restir_last_error(), what
            assert (out == 7.0).all(), what
            assert_bits(r.download_rgb(w, h), last, what + ": the last image")
            assert r.denoise_guide_builds() == 0, what

        refused(INVALID, "a NULL context", ctx=False)
        refused(INVALID, "a NULL camera", cam_=None)
        refused(INVALID, "NULL parameters", p=None)
        refused(INVALID, "no level", p=restir.denoise_params(iterations=0))
        refused(INVALID, "six levels", p=restir.denoise_params(iterations=6))
        refused(INVALID, "a normal exponent of 2^8", p=restir.denoise_params(normal_power_log2=8))
        refused(INVALID, "sigma_plane 0", p=restir.denoise_params(sigma_plane=0.0))
        refused(INVALID, "sigma_plane NaN", p=restir.denoise_params(sigma_plane=float("nan")))
        refused(INVALID, "sigma_plane inf", p=restir.denoise_params(sigma_plane=float("inf")))
        refused(INVALID, "flags", p=_abi.DenoiseParams(3, 5, 0.01, 2))
        refused(INVALID, "an empty image", w_=0)
        t = restir.tile_plan(70, 37, 2, 2, 0, 0)
        refused(INVALID, "a tile of another image", tile=t)
        refused(STATE, "another size", w_=70, h_=37)
        assert b"33x17" in lib.restir_last_error()
        t = restir.tile_plan(w, h, 2, 1, 0, 0)
        refused(STATE, "a tile smaller than the image", tile=t)
        # between halo_begin and halo_end
        r.halo_record(True)
        r.halo_begin(None, cam, w, h, f, (2, 1), 0)
        assert call() == STATE and b"halo" in lib.restir_last_error()
        assert (out == 7.0).all() and r.denoise_guide_builds() == 0
        for _ in range(f.spatial_resampling_passes):
            r.halo_pass()
        r.halo_end(restir.tile_plan(w, h, 2, 1, 0, f.spatial_resample_radius), False, False)
        r.halo_record(False)
        assert call() == STATE, "the halo frame's tile has not the size asked for"
        assert (out == 7.0).all()
    finally:
        r.close()


# ---- G: it helps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(70, 37), (130, 70)])
def test_denoising_lowers_the_true_mse(gpu, oracle, w, h):
    """The C2 frame, default parameters, against the exact image: mse(denoised) < mse(raw), strictly and without a
    tolerance.  On the CPU first -- the oracle's frame, the host function, the specification's exact image (21.55 -> 3.63
    at 70 x 37, 10.12 -> 3.05 at 130 x 70 when this was written) -- then on the device with its own error figures."""
    cam = scene.nightclub_camera(w, h)
    lin = _abi.default_features(**LIN)
    exact = spec_image(oracle, NIGHT, None, w, h, lin)
    oraw = oracle.render_frame(oscene(oracle, NIGHT), cam, c2(**LIN), w, h, SEED, 0)[0]
    n_t, p_mat = gbuffer(oracle, NIGHT, w, h)
    oden = restir.denoise_host(oraw, n_t, p_mat, miss_of(NIGHT))
    cpu_raw, cpu_den = restir.error_measure(oraw, exact).mse, restir.error_measure(oden, exact).mse
    print(f"{w}x{h}: true mse on the CPU {cpu_raw:.4f} -> {cpu_den:.4f}")
    assert cpu_den < cpu_raw

    gpu.set_scene(the_scene(NIGHT))
    assert_bits(gpu.render_exact(cam, w, h, lin), exact, "the exact image")
    gpu.reference_set()
    raw = frame0(gpu, cam, w, h)
    assert_bits(raw, oraw, "the frame")
    mse_raw = gpu.error("image").mse
    den = gpu.denoise(cam, w, h)
    assert_bits(den, oden, "the denoised frame")
    mse_den = gpu.error("image").mse
    print(f"{w}x{h}: true mse on the device {mse_raw:.4f} -> {mse_den:.4f}")
    assert (mse_raw, mse_den) == (cpu_raw, cpu_den)
    assert mse_den < mse_raw
    gpu.reference_clear()
