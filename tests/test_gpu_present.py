"""Presenting a frame (include/restir_c.h "presenting a frame"): the device conversion of the last image into 8-bit
pixels equals the host's restir_rgb_to_rgba8 / restir_encode_bmp byte for byte on both sides of every byte boundary (A),
a rendered frame and a screen tile come out as the host converts their floats (B), a snapshot is not reached by the
frame enqueued behind it (C), the slots behave as documented (D), and the C++ example writes the files the Python
binding writes (E).  GPU against host code and GPU against GPU: no oracle frame is needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from romis_amd import _abi, restir, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = 4, 1
NAME = "nightclub_128pt"
SIZES = [(1, 1), (3, 2), (4, 1), (5, 3), (7, 5), (33, 17), (70, 37), (256, 4)]


def host_rgba8(lib, rgb):
    """restir_rgb_to_rgba8 of [..][3] floats -> [..][4] bytes"""
    a = np.ascontiguousarray(rgb, np.float32)
    out = np.zeros(a.shape[:-1] + (4,), np.uint8)
    assert lib.restir_rgb_to_rgba8(a.ctypes.data, a.size // 3, out.ctypes.data) == 0
    return out


def host_bmp(lib, rgb):
    """restir_encode_bmp of an [H][W][3] image: the file's bytes"""
    a = np.ascontiguousarray(rgb, np.float32)
    h, w = a.shape[:2]
    n = C.c_size_t()
    assert lib.restir_encode_bmp(a.ctypes.data, w, h, None, 0, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint8)
    assert lib.restir_encode_bmp(a.ctypes.data, w, h, buf.ctypes.data, n.value, C.byref(n)) == 0
    return buf


def host_byte(lib, bits):
    """the byte the host conversion makes of each float given by its bit pattern"""
    b = np.ascontiguousarray(bits, np.uint32)
    px = np.zeros((b.size, 3), np.uint32)
    px[:, 0] = b
    return host_rgba8(lib, px.view(np.float32))[:, 0].astype(np.int64)


def fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


@pytest.fixture(scope="module")
def boundary_bits(lib):
    """For each byte k = 1..255 the first float of [0, 1] (by bit pattern, where the host conversion is monotone) that
    converts to k and the float before it; then the special values and 4,096 hashed patterns.  Asserted from the host
    conversion alone: the set yields every byte and both sides of all 255 boundaries."""
    k = np.arange(1, 256, dtype=np.int64)
    lo = np.zeros(255, np.int64)                    # host(lo) < k
    hi = np.full(255, 0x3F800000, np.int64)         # host(hi) >= k  (1.0f -> 255)
    assert (host_byte(lib, lo) < k).all() and (host_byte(lib, hi) >= k).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ge = host_byte(lib, mid) >= k
        hi = np.where(ge, mid, hi)
        lo = np.where(ge, lo, mid)
    assert (hi - lo == 1).all()
    assert (host_byte(lib, hi) == k).all() and (host_byte(lib, lo) == k - 1).all()   # both sides of all 255 boundaries
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    special = [0x00000000, 0x80000000, 0x00000001, f32(-1e-30), 0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x7F7FFFFF,
               0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA55A5A, 0x7FFFFFFF]
    hashed = fmix32(np.arange(4096, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15))
    bits = np.concatenate([hi, lo, np.array(special, np.int64), hashed.astype(np.int64)]).astype(np.uint32)
    assert set(host_byte(lib, bits).tolist()) == set(range(256))                       # every byte 0..255
    return bits


@pytest.fixture(scope="module")
def renderer():
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene(NAME))
    yield r
    r.close()


def features(**kw):
    return _abi.default_features(num_samples_in_reservoir=1, spatial_resampling_passes=2, temporal_reuse=0,
                                 enable_tone_mapping=0, **kw)


# ---- A: conversion, every byte boundary ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_conversion_matches_the_host_on_every_boundary(lib, boundary_bits, W, H):
    n = W * H * 3
    # every value at every size: the windows tile the set (1,540 of them at 1 x 1)
    starts = [i * n for i in range(-(-boundary_bits.size // n))]
    r = restir.Renderer(0)
    try:
        r.stage_configure(W, H, 1)
        for s in starts:
            img = np.take(boundary_bits, np.arange(s, s + n), mode="wrap").reshape(H, W, 3)
            r.upload(_abi.BUF_RGB, img.view(np.float32))
            with r.present("rgba8") as a, r.present("bgra8_bottom_up") as b, r.present("rgb32f") as c:
                assert (a.width, a.height, a.nbytes) == (W, H, W * H * 4) and c.nbytes == W * H * 12
                rgba, bgra, f32 = a.wait(), b.wait(), c.wait()
                assert np.array_equal(rgba, host_rgba8(lib, img.view(np.float32))), f"RGBA8 at window {s}"
                assert bgra.tobytes() == host_bmp(lib, img.view(np.float32))[122:].tobytes(), f"BGRA8 at window {s}"
                assert np.array_equal(f32.view(np.uint32), img), f"RGB32F at window {s}"   # NaN payloads included
            got = r.download_rgba8(W, H)
            assert np.array_equal(got, host_rgba8(lib, img.view(np.float32)))
    finally:
        r.close()


# ---- B: a rendered frame ------------------------------------------------------------------------------------------
def test_rendered_frame_as_bytes_and_bmp(lib, renderer, tmp_path):
    r = renderer
    for W, H in [(70, 37), (5, 3)]:
        r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
        rgb, _ = r.render_restir(None, scene.camera_for(NAME, W, H), W, H, features(), want_grid=False)
        if (W, H) == (70, 37):
            assert (rgb > 1.0).any()   # the clamp is exercised
        down = r.download_rgb(W, H)
        assert np.array_equal(down.view(np.uint32), rgb.view(np.uint32))
        assert np.array_equal(r.download_rgba8(W, H), host_rgba8(lib, down))
        assert np.array_equal(r.download_rgba8(), host_rgba8(lib, down))
        got, want = tmp_path / f"got{W}.bmp", tmp_path / f"want{W}.bmp"
        r.write_bmp(got)
        assert lib.restir_write_bmp(os.fsencode(want), down.ctypes.data, W, H) == 0
        assert got.read_bytes() == want.read_bytes()
    small = (C.c_uint8 * 4)()
    assert lib.restir_download_rgba8(r.ctx, small, 1) == INVALID   # below the image's pixel count


def test_screen_tile_snapshot_has_the_owned_size_and_bytes(lib, renderer):
    r = renderer
    W, H = 70, 37
    f = features()
    t = restir.tile_plan(W, H, 2, 2, 1, f.spatial_resampling_passes * f.spatial_resample_radius)
    assert (t.width, t.height) != (W, H)
    r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
    rgb, _ = r.render_restir(None, scene.camera_for(NAME, W, H), W, H, f, tile=t, want_grid=False)
    with r.present("rgba8") as im:
        assert (im.width, im.height, im.nbytes) == (t.width, t.height, t.width * t.height * 4)
        assert np.array_equal(im.wait(), host_rgba8(lib, rgb))


# ---- C: the next frame does not reach a snapshot ------------------------------------------------------------------
@pytest.mark.parametrize("W,H,fmt", [(70, 37, "rgba8"), (1920, 1080, "rgb32f")])
def test_next_frame_does_not_reach_a_snapshot(renderer, W, H, fmt):
    r = renderer
    cam = scene.camera_for(NAME, W, H)
    f = features()
    r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
    r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)   # frame 0: enqueued only
    a = r.present(fmt)
    r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)   # frame 1, at once: no synchronise
    b = r.present(fmt)
    try:
        got = [a.wait().copy(), b.wait().copy()]
    finally:
        a.release()
        b.release()
    # a second pass over the same seeds, each frame read back synchronously
    r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
    want = []
    for _ in range(2):
        r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)
        want.append(r.download_rgba8(W, H) if fmt == "rgba8" else r.download_rgb(W, H))
    for i in range(2):
        assert got[i].tobytes() == want[i].tobytes(), f"frame {i}"
    assert got[0].tobytes() != got[1].tobytes()


# ---- D: slots -----------------------------------------------------------------------------------------------------
def test_slots(lib):
    r = restir.Renderer(0)
    try:
        h = C.c_void_p()
        assert lib.restir_image_begin(r.ctx, _abi.IMAGE_RGBA8, C.byref(h)) == STATE   # nothing rendered yet
        assert not h.value
        r.set_scene(scene.bench_scene(NAME))
        W, H = 33, 17
        r.render_restir(None, scene.camera_for(NAME, W, H), W, H, features(), want_grid=False)
        assert lib.restir_image_begin(r.ctx, 3, C.byref(h)) == INVALID                # unknown format
        held = [r.present("rgba8") for _ in range(_abi.RESTIR_MAX_IMAGES_IN_FLIGHT)]
        assert lib.restir_image_begin(r.ctx, _abi.IMAGE_RGBA8, C.byref(h)) == STATE   # the fifth
        assert b"unreleased" in lib.restir_last_error()
        held.pop().release()
        held.append(r.present("rgba8"))                                              # after one release
        # ready() without a wait(): the context's stream is drained, and releasing the LAST snapshot waits for its
        # copy, which the copy stream runs after the first's
        r.synchronize()
        held.pop().release()
        assert held[0].ready()
        small = held[0].wait().copy()
        for im in held:
            im.release()
        # the slots are re-used for a larger image
        W2, H2 = 70, 37
        rgb, _ = r.render_restir(None, scene.camera_for(NAME, W2, H2), W2, H2, features(), want_grid=False)
        big = [r.present("rgba8") for _ in range(_abi.RESTIR_MAX_IMAGES_IN_FLIGHT)]
        for im in big:
            assert (im.width, im.height) == (W2, H2)
            assert np.array_equal(im.wait(), host_rgba8(lib, rgb))
            im.release()
        assert small.shape == (H, W, 4)
        with pytest.raises(restir.RestirError):
            big[0].wait()   # released
        outstanding = r.present("rgb32f")   # restir_destroy with one snapshot outstanding returns cleanly
        assert outstanding.nbytes == W2 * H2 * 12
    finally:
        r.close()
    outstanding.release()   # a no-op once the Renderer is closed


# ---- E: C++ -------------------------------------------------------------------------------------------------------
def test_cpp_example_writes_the_python_bindings_files(renderer, tmp_path):
    from test_cpp_wrapper import build_cpp, write_scene
    W, H = 70, 37
    cam = scene.camera_for(NAME, W, H)
    write_scene(tmp_path / "s.bin", scene.bench_scene(NAME), cam)
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "present_frames.cpp"),
                    os.path.join(ROOT, "romis_amd", "_build", "present_frames"))
    outs = [tmp_path / "f0.bmp", tmp_path / "f1.bmp"]
    subprocess.check_call([exe, str(tmp_path / "s.bin"), str(outs[0]), str(outs[1]), str(W), str(H)], timeout=120)
    r = renderer
    r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
    for i in range(2):
        r.render_restir(None, cam, W, H, features(), want_rgb=False, want_grid=False)
        want = tmp_path / f"w{i}.bmp"
        r.write_bmp(want)
        assert outs[i].read_bytes() == want.read_bytes(), f"frame {i}"
    assert outs[0].read_bytes() != outs[1].read_bytes()
