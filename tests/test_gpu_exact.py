"""The exact direct-lighting image, the kept reference and the device-side error figures (include/restir_c.h "the exact
direct-lighting image", csrc/exact.h / exact.hip).

A  restir_render_exact equals the specification bit for bit, no tolerance: tests/exact_spec.py builds the image on the CPU
   from the oracle's G-buffer and one run of its final shading per light (N = 1, tone mapping off, the reservoir set to
   light i with W = 1, M = 1), float32-summed in light order, then or_tonemap.  Scenes: the 128-light nightclub; Monkey
   under 16 point lights with the BVH past the LDS budget (the global-BVH kernel) and with a larger leaf (the LDS
   kernel); the nightclub under 1, 3, 255 and no lights; shading off; tone mapping off, with gamma 1 and gamma 2.2; a
   textured cube with texture mapping on and off; 1 x 1 and 3 x 2 frames.  Every ray test first asserts on the CPU that
   its frame holds at least 16 lit (pixel, light) pairs that are visible and 16 that are occluded.
B  a 2 x 2 split rendered tile by tile stitches to the whole image;
C  the call has no side effects on frames: seven C2 and seven C3 still frames with an exact render between every two,
   and a reference and error figures after some, equal bit for bit and counter for counter a context's that never
   renders the exact image; two exact renders are identical;
D  it is a producer: one add per exact image, present and write_bmp serve it;
E  scenes with a segment or parallelogram light are RESTIR_ERR_UNSUPPORTED and leave the last image alone;
F  restir_error_get equals restir_error_measure over the downloaded arrays bit for bit: a frame, an accumulated mean,
   uploaded images with NaN / inf; the reference is a snapshot, and every state error leaves it and the image alone;
G  the exact image is the estimator's expectation: RIS alone over one light reproduces it up to its roundings.
GPU against the CPU oracle; images are at most 70 x 37."""
import ctypes as C

import numpy as np
import pytest

import exact_spec as spec
from romis_amd import _abi, restir, scene
from test_gpu_parity import get_scene
from test_gpu_scene_shapes import LDS_BUDGET, camera as shape_camera, shape_scene, _points
from test_gpu_shadow_lists import lights_around

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = 1, 4, 5
NIGHT = "nightclub_128pt"
SEED = _abi.RESTIR_DEFAULT_SEED
SIZES = [(33, 17), (70, 37)]   # 2 x 3 and 3 x 5 tiles of 32 x 8, the last ragged on both axes
F32 = np.float32
FP = C.POINTER(C.c_float)
MIN_PAIRS = 16


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_bits(got, want, what):
    g, w_ = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w_.shape, f"{what}: shape {g.shape} != {w_.shape}"
    bad = np.flatnonzero(g != w_)
    assert bad.size == 0, f"{what}: {bad.size}/{g.size} words differ; first idx {bad[:4].tolist()} " \
                          f"got {g[bad[:4]].view(F32).tolist()} want {w_[bad[:4]].view(F32).tolist()}"


def figures(s):
    """an ErrorStats' measured fields (counted .. ref_mean) as bytes: NaN compares equal to the same NaN"""
    return bytes(s)[16:]


def c2(**kw):
    """bench.py's C2: N = 1, M = 32, k = 5, r = 10, one biased pass, no temporal reuse"""
    kw.setdefault("temporal_reuse", 0)
    kw.setdefault("spatial_resampling_passes", 1)
    return _abi.default_features(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5,
                                 spatial_resample_radius=10, spatial_reuse=1, **kw)


def c3(**kw):
    return c2(temporal_reuse=1, spatial_resampling_passes=2, **kw)


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


# ---- scenes, cameras and the CPU side, computed once and shared -----------------------------------------------------
_scenes, _oscenes, _specs, _census = {}, {}, {}, {}


def the_scene(name):
    if name not in _scenes:
        night = get_scene(NIGHT)
        if name == "pt1":
            _scenes[name] = scene.Scene(night.meshes, _points((8, 8), 1), name)
        elif name == "dark":
            _scenes[name] = scene.Scene(night.meshes, [], name)
        elif name == "monkey16":
            base = scene.load_prebuilt("Monkey")
            _scenes[name] = scene.Scene(base.meshes, lights_around(base, 15, 3), name)
        elif name == "tex16":   # test_gpu_parity.py's textured cube (its own light is a segment) under 16 point lights
            base = get_scene("CubeTextured")
            _scenes[name] = scene.Scene(base.meshes, lights_around(base, 15, 3), name)
        else:
            _scenes[name] = shape_scene(name)   # nightclub_128pt, pt3, pt255, mixed17, cornell_1024
    return _scenes[name]


def the_camera(name, cam, w, h):
    if name == "monkey16":
        return shape_camera("Monkey", cam, w, h)
    if name == "tex16":
        return scene.camera_for("CubeTextured", w, h)
    return scene.nightclub_camera(w, h)


def oscene(oracle, name):
    if name not in _oscenes:
        _oscenes[name] = oracle.OracleScene(the_scene(name))
    return _oscenes[name]


def spec_image(oracle, name, cam, w, h, f):
    k = (name, cam, w, h, f.enable_shading, f.enable_texture_mapping, f.enable_tone_mapping, f.gamma, f.exposure)
    if k not in _specs:
        img = spec.exact_image(oracle, oscene(oracle, name), the_scene(name), the_camera(name, cam, w, h), w, h, f)
        img.flags.writeable = False
        _specs[k] = img
    return _specs[k]


def assert_rays_matter(oracle, name, cam, w, h):
    """the frame holds lit pairs the shadow ray lets through and lit pairs it blocks"""
    k = (name, cam, w, h)
    if k not in _census:
        _census[k] = spec.pair_census(oracle, oscene(oracle, name), the_scene(name), the_camera(name, cam, w, h), w, h)
    vis, occ = _census[k]
    assert vis >= MIN_PAIRS and occ >= MIN_PAIRS, f"{name} {w}x{h}: {vis} visible and {occ} occluded lit pairs"
    return vis, occ


def check_exact(gpu, oracle, name, cam, w, h, f, what, rays=True):
    """render_exact of the uploaded scene against the specification; returns the image"""
    if rays:
        assert_rays_matter(oracle, name, cam, w, h)
    want = spec_image(oracle, name, cam, w, h, f)
    got = gpu.render_exact(the_camera(name, cam, w, h), w, h, f)
    assert_bits(got, want, f"{what} {w}x{h}")
    assert_bits(gpu.download_rgb(w, h), got, f"{what} {w}x{h}: out_rgb against download_rgb")
    return got


# ---- A: bit-exact against the specification ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_nightclub_128_lights(gpu, oracle, w, h):
    gpu.set_scene(the_scene(NIGHT))
    info = gpu.scene_info()
    assert info.num_lights == 128 and info.light_types == 1 and info.bvh_lds_bytes <= LDS_BUDGET
    img = check_exact(gpu, oracle, NIGHT, None, w, h, _abi.default_features(), "nightclub")
    assert 0.0 < img.mean() < 1.0 and (img == 0).any() and (img > 0).any()


@pytest.mark.parametrize("cam,w,h", [("toml", 33, 17), ("toml", 70, 37), ("framed", 70, 37)])
def test_monkey_over_the_lds_budget_walks_the_global_bvh(gpu, oracle, cam, w, h):
    gpu.set_scene(the_scene("monkey16"))          # bvh.max_leaf = 2, the default
    info = gpu.scene_info()
    assert info.num_lights == 16 and info.light_types == 1
    assert info.bvh_lds_bytes > LDS_BUDGET, f"the BVH takes {info.bvh_lds_bytes} bytes: it fits LDS"
    check_exact(gpu, oracle, "monkey16", cam, w, h, _abi.default_features(), f"Monkey {cam}, global BVH")


@pytest.mark.parametrize("w,h", SIZES)
def test_monkey_with_a_larger_leaf_stages_the_bvh(gpu, oracle, w, h):
    try:
        gpu.set_tuning("bvh.max_leaf", 5)
        gpu.set_scene(the_scene("monkey16"))
        info = gpu.scene_info()
        # (with the kernel's static LDS, at most 1 KB: csrc/exact.h kExactStaticLds)
        assert info.bvh_lds_bytes + 1024 <= LDS_BUDGET, f"the BVH takes {info.bvh_lds_bytes} bytes: past the LDS budget"
        check_exact(gpu, oracle, "monkey16", "toml", w, h, _abi.default_features(), "Monkey, BVH in LDS")
    finally:
        gpu.set_tuning("bvh.max_leaf", 2)


@pytest.mark.parametrize("name,L", [("pt1", 1), ("pt3", 3), ("pt255", 255)])
def test_nightclub_light_counts(gpu, oracle, name, L):
    """1 and 3 lights take the census of the frame they render.  255 lights render 70 x 37 but take it at 33 x 17, the same
    scene and camera: or_target_pdf is one call per pair, and 660,000 pairs cost 2.8 s of CPU against 0.7 s for the small
    frame's 143,000 (71,103 visible, 17,899 occluded), which already shows that this light set casts rays both ways."""
    gpu.set_scene(the_scene(name))
    info = gpu.scene_info()
    assert info.num_lights == L and info.light_types == 1
    # one light at 70 x 37 lights pairs enough; the census of 255 lights is taken at the small size (660,000 pairs else)
    w, h = (70, 37)
    if L == 255:
        assert_rays_matter(oracle, name, None, 33, 17)
    img = check_exact(gpu, oracle, name, None, w, h, _abi.default_features(enable_tone_mapping=0), f"{L} lights", rays=L != 255)
    assert (img > 0).any()


def test_no_lights_is_the_tone_mapped_zero_image(gpu, oracle):
    gpu.set_scene(the_scene("dark"))
    assert gpu.scene_info().num_lights == 0
    for f in (_abi.default_features(), _abi.default_features(gamma=2.2), _abi.default_features(enable_tone_mapping=0)):
        img = check_exact(gpu, oracle, "dark", None, 33, 17, f, "no lights", rays=False)
        assert not bits(img).any()    # +0 everywhere: 1 - exp(-0) = +0 and pow(+0, 1 / 2.2) = +0


def test_shading_off_adds_kd_per_visible_light(gpu, oracle):
    gpu.set_scene(the_scene(NIGHT))
    f = _abi.default_features(enable_shading=0, enable_tone_mapping=0)
    w, h = 33, 17
    img = check_exact(gpu, oracle, NIGHT, None, w, h, f, "shading off")
    lit = check_exact(gpu, oracle, NIGHT, None, w, h, _abi.default_features(enable_tone_mapping=0), "shading on")
    assert not np.array_equal(bits(img), bits(lit)) and img.max() > 1.0   # kd times the number of visible lights


@pytest.mark.parametrize("tone", [dict(enable_tone_mapping=0), dict(gamma=1.0, exposure=1.5), dict(gamma=2.2, exposure=0.7)])
@pytest.mark.parametrize("w,h", SIZES)
def test_tone_mapping(gpu, oracle, w, h, tone):
    gpu.set_scene(the_scene(NIGHT))
    img = check_exact(gpu, oracle, NIGHT, None, w, h, _abi.default_features(**tone), f"tone {tone}")
    if tone.get("enable_tone_mapping", 1):
        assert img.max() <= 1.0   # (1 - exp(-x) rounds to 1 where a light is close)
    else:
        assert img.max() > 1.0    # linear: the tone-mapped range does not hold it


@pytest.mark.parametrize("texture", [1, 0])
def test_textured_scene(gpu, oracle, texture):
    gpu.set_scene(the_scene("tex16"))
    info = gpu.scene_info()
    assert info.num_lights == 16 and info.light_types == 1
    w, h = 70, 37
    f = _abi.default_features(enable_texture_mapping=texture, enable_tone_mapping=0)
    img = check_exact(gpu, oracle, "tex16", None, w, h, f, f"texture {texture}", rays=False)
    other = spec_image(oracle, "tex16", None, w, h, _abi.default_features(enable_texture_mapping=1 - texture, enable_tone_mapping=0))
    assert (img > 0).any() and not np.array_equal(bits(img), bits(other))   # the texels change the image


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2)])
def test_frames_below_one_tile(gpu, oracle, w, h):
    gpu.set_scene(the_scene(NIGHT))
    check_exact(gpu, oracle, NIGHT, None, w, h, _abi.default_features(), "tiny frame", rays=False)


def test_without_out_rgb_it_only_enqueues_the_same_image(gpu, oracle):
    gpu.set_scene(the_scene(NIGHT))
    w, h = 33, 17
    f = _abi.default_features()
    assert gpu.render_exact(scene.nightclub_camera(w, h), w, h, f, download=False) is None
    assert_bits(gpu.download_rgb(w, h), spec_image(oracle, NIGHT, None, w, h, f), "download after an enqueue-only render")


def test_exact_render_leaves_the_stage_api_unconfigured(gpu):
    """Like a frame, the call gives the image buffer another size: the stage API reports RESTIR_ERR_STATE until
    restir_stage_configure runs again, instead of serving a stage image with the exact image's size."""
    gpu.set_scene(the_scene(NIGHT))
    gpu.stage_configure(33, 17, 1)
    gpu.render_exact(scene.nightclub_camera(70, 37), 70, 37, _abi.default_features(), download=False)
    with pytest.raises(_abi.RestirError, match="STATE"):
        gpu.download(_abi.BUF_RGB)
    gpu.stage_configure(33, 17, 1)
    assert gpu.download(_abi.BUF_RGB).size == 33 * 17 * 3   # configured again: the download is served


# ---- B: tiles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ghost", [0, 10])
def test_tiles_stitch_to_the_whole_image(gpu, oracle, ghost):
    gpu.set_scene(the_scene(NIGHT))
    w, h = 70, 37
    f = _abi.default_features()
    cam = scene.nightclub_camera(w, h)
    layout = restir.layout_even(w, h, 2, 2)
    out = np.full((h, w, 3), np.nan, F32)
    for rank in range(4):
        t = restir.tile_plan(w, h, 2, 2, rank, ghost, layout=layout)   # a ghost ring is accepted and not computed
        img = gpu.render_exact(cam, w, h, f, tile=t)
        assert img.shape == (t.height, t.width, 3)
        assert_bits(gpu.download_rgb(t.width, t.height), img, f"tile {rank}: out_rgb against download_rgb")
        top = h - (t.y0 + t.height)                                    # y = 0 is the bottom row, row 0 the top
        out[top:top + t.height, t.x0:t.x0 + t.width] = img
    assert_bits(out, spec_image(oracle, NIGHT, None, w, h, f), "stitched tiles")
    assert_bits(out, gpu.render_exact(cam, w, h, f), "stitched tiles against the whole image")


# ---- C: no side effects ----------------------------------------------------------------------------------------------
FRAMES = 7


def counters(r):
    return dict(gbuf_reuses=r.gbuf_reuses(), shadow_list_frames=r.shadow_list_frames(), shadow_vis_frames=r.shadow_vis_frames(),
                shadow_vis_builds=r.shadow_vis_builds(), phat_frames=r.phat_frames(), phat_builds=r.phat_builds())


def still_run(sc, cam, w, h, f, exact):
    r = restir.Renderer(0)
    try:
        r.set_scene(sc)
        r.set_seed(SEED, 0)
        out = dict(images=[], grids=[], exact=[])
        fe = _abi.default_features(enable_tone_mapping=0)
        prev = None
        for k in range(FRAMES):
            rgb, grid = r.render_restir(prev if f.temporal_reuse else None, cam, w, h, f, want_grid=True)
            out["images"].append(rgb)
            out["grids"].append([np.asarray(a).copy() for a in grid.download()])
            prev = grid
            if exact:
                out["exact"].append(r.render_exact(cam, w, h, fe, download=k % 2 == 0))
                if k in (1, 4):
                    r.reference_set()
                if k in (2, 5):
                    assert r.error("image").mse == 0.0     # the exact image against the kept one
        out["counters"] = counters(r)
        return out
    finally:
        r.close()


@pytest.mark.parametrize("cfg", ["c2", "c3"])
def test_exact_renders_change_no_frame_and_no_cache(oracle, cfg):
    w, h = 70, 37
    sc, cam = the_scene(NIGHT), scene.nightclub_camera(w, h)
    f = dict(c2=c2, c3=c3)[cfg](enable_tone_mapping=0)
    plain, mixed = still_run(sc, cam, w, h, f, False), still_run(sc, cam, w, h, f, True)
    for k in range(FRAMES):
        assert_bits(mixed["images"][k], plain["images"][k], f"{cfg} frame {k} image")
        for j, (a, b) in enumerate(zip(mixed["grids"][k], plain["grids"][k])):
            assert_bits(a.view(F32), b.view(F32), f"{cfg} frame {k} grid plane {j}")
    assert not np.array_equal(bits(plain["images"][0]), bits(plain["images"][1]))   # independent frames
    assert mixed["counters"] == plain["counters"], cfg
    assert plain["counters"]["gbuf_reuses"] == FRAMES - 1 and plain["counters"]["phat_builds"] == 1   # the still view's routes ran
    want = spec_image(oracle, NIGHT, None, w, h, _abi.default_features(enable_tone_mapping=0))
    got = [e for e in mixed["exact"] if e is not None]
    assert len(got) == 4
    for e in got:
        assert_bits(e, want, f"{cfg}: an exact image between frames")   # the same bits every time


# ---- D: the producer rule --------------------------------------------------------------------------------------------
def test_exact_image_is_a_produced_image(lib, oracle, tmp_path):
    w, h = 33, 17
    f = _abi.default_features(gamma=2.2)
    cam = scene.nightclub_camera(w, h)
    r = restir.Renderer(0)
    try:
        r.set_scene(the_scene(NIGHT))
        r.accum_begin(False)
        img = r.render_exact(cam, w, h, f)
        r.accum_add()
        assert lib.restir_accum_add(r.ctx) == STATE                      # each image once
        assert_bits(r.accum_state(w, h)[0], img, "the mean after one add")
        img2 = r.render_exact(cam, w, h, f, download=False)              # a new serial
        assert img2 is None
        r.accum_add()
        assert lib.restir_accum_add(r.ctx) == STATE
        assert_bits(r.accum_state(w, h)[0], img, "the mean of two equal images")
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
        # no frame index is consumed: the next frame is frame 0's
        r.set_seed(SEED, 0)
        r.render_exact(cam, w, h, f, download=False)
        first, _ = r.render_restir(None, cam, w, h, c2(), want_grid=False)
        r.set_seed(SEED, 0)
        again, _ = r.render_restir(None, cam, w, h, c2(), want_grid=False)
        assert_bits(first, again, "frame 0 after an exact render")
    finally:
        r.close()


# ---- E: unsupported scenes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,word", [("cornell_1024", b"parallelogram"), ("mixed17", b"segment")])
def test_area_lights_are_unsupported(lib, name, word):
    w, h = 33, 17
    r = restir.Renderer(0)
    try:
        sc = the_scene(name)
        r.set_scene(sc)
        assert r.scene_info().light_types != 1
        cam = scene.camera_for(name, w, h) if name == "cornell_1024" else scene.nightclub_camera(w, h)
        f = _abi.default_features()
        out = np.full((h, w, 3), 7.0, F32)
        call = lambda: lib.restir_render_exact(r.ctx, C.byref(cam), C.byref(f), w, h, None, out.ctypes.data_as(FP))
        assert call() == UNSUPPORTED                                      # before anything was rendered
        msg = lib.restir_last_error()
        assert b"restir_render_exact" in msg and word in msg
        assert (out == 7.0).all()
        assert lib.restir_reference_set(r.ctx) == STATE                   # still no image
        last, _ = r.render_restir(None, cam, w, h, c2(), want_grid=False)
        assert call() == UNSUPPORTED
        assert (out == 7.0).all()
        assert_bits(r.download_rgb(w, h), last, "the last image after a refused call")
        r.accum_begin(False)
        r.accum_add()                                                     # ... and it is still that frame's, never added
        assert lib.restir_accum_add(r.ctx) == STATE
    finally:
        r.close()


# ---- F: error figures ------------------------------------------------------------------------------------------------
def test_error_figures_equal_the_host_measure(lib, oracle):
    w, h = 70, 37
    cam = scene.nightclub_camera(w, h)
    lin = _abi.default_features(enable_tone_mapping=0)
    r = restir.Renderer(0)
    try:
        r.set_scene(the_scene(NIGHT))
        r.set_seed(SEED, 0)
        ref = r.render_exact(cam, w, h, lin)
        assert_bits(ref, spec_image(oracle, NIGHT, None, w, h, lin), "the reference")
        r.reference_set()
        assert r.reference_info() == (w, h, True)
        e = r.error("image")
        assert (e.width, e.height, e.source, e.frames) == (w, h, _abi.RESTIR_ERROR_SRC_IMAGE, 0)
        assert e.counted == 3 * w * h and e.nonfinite == 0
        assert (e.mse, e.mae, e.rel_mse, e.bias, e.max_abs) == (0.0, 0.0, 0.0, 0.0, 0.0)
        assert figures(e) == figures(restir.error_measure(ref, ref))
        # a C2 frame as the image
        frame, _ = r.render_restir(None, cam, w, h, c2(enable_tone_mapping=0), want_grid=False)
        e = r.error("image")
        assert figures(e) == figures(restir.error_measure(frame, ref))
        assert e.mse > 0.0 and e.max_abs > 0.0 and e.counted == 3 * w * h
        assert figures(r.error(_abi.RESTIR_ERROR_SRC_IMAGE)) == figures(e)          # the same bits every time
        # the mean of five frames
        r.accum_begin(True)
        r.accum_add()
        for _ in range(4):
            r.render_restir(None, cam, w, h, c2(enable_tone_mapping=0), want_rgb=False, want_grid=False)
            r.accum_add()
        e5 = r.error("accum")
        mean, _ = r.accum_state(w, h)
        assert (e5.width, e5.height, e5.source, e5.frames) == (w, h, _abi.RESTIR_ERROR_SRC_ACCUM_MEAN, 5)
        assert figures(e5) == figures(restir.error_measure(mean, ref))
        assert 0.0 < e5.mse and not np.array_equal(bits(mean), bits(frame))
        # the reference is a snapshot: new lights, a new frame, the accumulation's end leave it alone
        r.set_lights(the_scene("pt3").lights)
        other, _ = r.render_restir(None, cam, w, h, c2(enable_tone_mapping=0), want_grid=False)
        r.accum_end()
        assert r.reference_info() == (w, h, True)
        assert figures(r.error("image")) == figures(restir.error_measure(other, ref))
        r.reference_clear()
        assert r.reference_info() == (0, 0, False)
        assert lib.restir_error_get(r.ctx, 0, C.byref(_abi.ErrorStats())) == STATE
    finally:
        r.close()


@pytest.mark.parametrize("w,h", [(1, 1), (33, 17), (70, 37)])
def test_error_figures_of_uploaded_images_with_non_finite_floats(lib, w, h):
    n = 3 * w * h
    u = (np.arange(n, dtype=np.uint64) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    ref = ((u >> 8).astype(F32) * F32(2.0 ** -21) - F32(2.0)).astype(F32)
    img = (ref * F32(0.75) + ((u >> 3) & 0xFF).astype(F32) * F32(2.0 ** -9)).astype(F32)
    bad = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFA55A5A, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000000], np.uint32).view(F32)
    if n > 64:
        ref[(np.arange(len(bad)) * 7) % n] = bad                      # in the reference
        img[(np.arange(len(bad)) * 11 + 5) % n] = np.roll(bad, 3)     # in the image
        img[(np.arange(4) * 7) % n] = bad[:4]                         # in both
    else:
        img[0] = np.inf
    r = restir.Renderer(0)
    try:
        r.stage_configure(w, h, 1)
        r.upload(_abi.BUF_RGB, ref)
        r.reference_set()
        r.upload(_abi.BUF_RGB, img)
        e = r.error("image")
        want = restir.error_measure(img, ref)
        assert figures(e) == figures(want)
        assert e.nonfinite == int((~(np.isfinite(img) & np.isfinite(ref))).sum()) > 0 and e.counted + e.nonfinite == n
    finally:
        r.close()


def test_state_errors_leave_the_reference_and_the_image_alone(lib):
    w, h = 33, 17
    cam, cam2 = scene.nightclub_camera(w, h), scene.nightclub_camera(70, 37)
    lin = _abi.default_features(enable_tone_mapping=0)
    f = c2(enable_tone_mapping=0, spatial_resampling_passes=2)
    r = restir.Renderer(0)
    get = lambda src: lib.restir_error_get(r.ctx, src, C.byref(_abi.ErrorStats()))
    try:
        r.set_scene(the_scene(NIGHT))
        assert lib.restir_reference_set(r.ctx) == STATE and b"restir_reference_set" in lib.restir_last_error()
        assert r.reference_info() == (0, 0, False)
        assert get(0) == STATE                                  # no reference
        ref = r.render_exact(cam, w, h, lin)
        r.reference_set()

        def refused(call, code, what, last):
            assert call() == code, what
            assert lib.restir_last_error(), what
            assert r.reference_info() == (w, h, True), what
            assert_bits(r.download_rgb(last.shape[1], last.shape[0]), last, what + ": the last image")

        refused(lambda: get(1), STATE, "the mean without an accumulation", ref)
        r.accum_begin(False)
        refused(lambda: get(1), STATE, "the mean of no frame", ref)
        refused(lambda: get(2), INVALID, "an unknown source", ref)
        refused(lambda: lib.restir_error_get(r.ctx, 0, None), INVALID, "a NULL struct", ref)
        big, _ = r.render_restir(None, cam2, 70, 37, f, want_grid=False)
        refused(lambda: get(0), STATE, "an image of another size", big)
        r.accum_add()
        refused(lambda: get(1), STATE, "a mean of another size", big)
        assert b"70x37" in lib.restir_last_error()
        # between halo_begin and halo_end the image has its size but not its pixels
        r.halo_record(True)
        r.halo_begin(None, cam, w, h, f, (2, 1), 0)
        assert lib.restir_reference_set(r.ctx) == STATE and b"halo" in lib.restir_last_error()
        assert lib.restir_render_exact(r.ctx, C.byref(cam), C.byref(lin), w, h, None, None) == STATE
        assert get(0) == STATE
        assert r.reference_info() == (w, h, True)
        for _ in range(f.spatial_resampling_passes):
            r.halo_pass()
        r.halo_end(restir.tile_plan(w, h, 2, 1, 0, f.spatial_resample_radius), False, False)
        r.halo_record(False)
        # the reference is still the first exact image
        again = r.render_exact(cam, w, h, lin)
        assert_bits(again, ref, "the exact image again")
        e = r.error("image")
        assert e.counted == 3 * w * h and e.max_abs == 0.0
    finally:
        r.close()


# ---- G: the exact image is the estimator's expectation ---------------------------------------------------------------
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
RIS_M = 4


def ris_bound(exact):
    """Per float, the bound of test_ris_over_one_light_reproduces_the_exact_image's docstring, in float64"""
    e = exact.astype(np.float64)
    phat = np.sqrt((e * e).sum(axis=-1, keepdims=True))
    ops = RIS_M + 4
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = (1.0 + FLT_MIN / (RIS_M * phat)) * (1.0 + ops * U / (1.0 - ops * U)) - 1.0
        return np.where(e != 0.0, np.abs(e) * rel + 2.0 ** -150, 0.0)


def test_ris_over_one_light_reproduces_the_exact_image(gpu, oracle):
    """Nightclub geometry, one point light, RIS only (no spatial, no temporal reuse), N = 1, M = 4, tone mapping off.
    Every candidate is the one light, with weight w = p / (1 / 1) = p exactly, p the target pdf |sc| of the light's
    unshadowed shade sc.  The reservoir's wSum is the FLT_MIN-seeded float32 sum of M = 4 equal weights -- four adds,
    each within 2^-24 relative: wSum = (4 p + FLT_MIN) (1 + t4); W = ((1 / p) (1 / M)) wSum adds one division and two
    products; the frame's colour is 0 + (vis ? sc : 0) W over N = 1: one more product (the add to +0 and the division by
    1 are exact).  M + 4 = 8 roundings in all, so for every float of a visible pixel

        |frame - exact| <= |exact| ((1 + FLT_MIN / (4 p)) (1 + 8 u / (1 - 8 u)) - 1) + 2^-150,  u = 2^-24,

    p the same float on both sides of W's quotient (its own rounding cancels), and a float whose exact value is 0 --
    occluded, back-facing or a zero component -- is 0.  2^-150 is half a step of the subnormal grid, where the last
    product of a subnormal component (a specular term about to underflow: the image holds some) lands.  The relative
    part holds while nothing else underflows or overflows: the test first asserts 2^-100 <= p <= 2^100 at every lit
    pixel, so 1 / p and W (1 within the roundings) are normal.  The oracle's own frames are confirmed inside the bound
    on the CPU before the device's are asked."""
    name, w, h = "pt1", 70, 37
    sc, cam = the_scene(name), scene.nightclub_camera(w, h)
    vis, occ = assert_rays_matter(oracle, name, None, w, h)
    f = _abi.default_features(num_samples_in_reservoir=1, initial_light_samples=RIS_M, spatial_reuse=0,
                              spatial_resampling_passes=0, temporal_reuse=0, enable_tone_mapping=0)
    exact = spec_image(oracle, name, None, w, h, _abi.default_features(enable_tone_mapping=0))
    nz = exact != 0
    phat = np.sqrt((exact.astype(np.float64) ** 2).sum(axis=-1))
    lit = nz.any(axis=-1)
    assert lit.any() and (~lit).any() and phat[lit].min() >= 2.0 ** -100 and phat[lit].max() <= 2.0 ** 100
    bound = ris_bound(exact)
    assert bound.max() < 1e-6 * np.abs(exact).max()       # eight roundings, not a tolerance one can hide in

    def inside(frame, what):
        d = np.abs(frame.astype(np.float64) - exact.astype(np.float64))
        bad = np.flatnonzero((d > bound).reshape(-1))
        assert bad.size == 0, f"{what}: {bad.size} floats outside the bound; worst {d.max()!r} against {bound.reshape(-1)[d.argmax()]!r}"
        assert not frame[~nz].any(), f"{what}: light where the exact image has none"

    osc = oscene(oracle, name)
    for frame in range(3):
        inside(oracle.render_frame(osc, cam, f, w, h, SEED, frame)[0], f"the oracle's frame {frame}")
    gpu.set_scene(sc)
    got = gpu.render_exact(cam, w, h, _abi.default_features(enable_tone_mapping=0))
    assert_bits(got, exact, "the exact image")
    gpu.reference_set()
    gpu.set_seed(SEED, 0)
    for frame in range(3):
        rgb, _ = gpu.render_restir(None, cam, w, h, f, want_grid=False)
        inside(rgb, f"the device's frame {frame}")
        e = gpu.error("image")
        assert e.max_abs <= bound.max() and e.nonfinite == 0
    gpu.reference_clear()
