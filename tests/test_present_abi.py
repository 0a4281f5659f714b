"""The presenting entry points of the C ABI (include/restir_c.h "presenting a frame") on the host: every symbol resolves
with its prototype, every call refuses a NULL context / image / out-pointer with RESTIR_ERR_INVALID before it touches a
device, restir_image_release(NULL) does nothing, and restir_bmp_header is restir_encode_bmp's header.  No GPU calls."""
import ctypes as C
import os

import numpy as np
import pytest

from romis_amd import _abi

INVALID = 1
NEW = ["restir_image_begin", "restir_image_info", "restir_image_ready", "restir_image_wait", "restir_image_release",
       "restir_download_rgba8", "restir_write_image_bmp", "restir_bmp_header"]


def test_symbols_resolve_with_their_prototypes(abi_lib):
    for name in NEW:
        fn = getattr(abi_lib, name)
        res, args = _abi.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert abi_lib.restir_abi_version() == 5   # the ABI only grew
    assert (_abi.IMAGE_RGB32F, _abi.IMAGE_RGBA8, _abi.IMAGE_BGRA8_BOTTOM_UP) == (0, 1, 2)
    assert _abi.RESTIR_MAX_IMAGES_IN_FLIGHT == 4
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "restir_c.h")) as fh:
        text = fh.read()
    assert "#define RESTIR_MAX_IMAGES_IN_FLIGHT 4u" in text
    assert "RESTIR_IMAGE_RGB32F = 0, RESTIR_IMAGE_RGBA8 = 1" in text and "RESTIR_IMAGE_BGRA8_BOTTOM_UP = 2" in text


def test_null_arguments_are_invalid(abi_lib):
    lib = abi_lib
    out = C.c_void_p(0x1234)
    assert lib.restir_image_begin(None, _abi.IMAGE_RGBA8, C.byref(out)) == INVALID
    assert lib.restir_image_begin(None, _abi.IMAGE_RGBA8, None) == INVALID
    assert b"null" in lib.restir_last_error().lower()
    w, h, f, n = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7), C.c_size_t(7)
    assert lib.restir_image_info(None, C.byref(w), C.byref(h), C.byref(f), C.byref(n)) == INVALID
    assert (w.value, h.value, f.value, n.value) == (7, 7, 7, 7)
    ready = C.c_int(5)
    assert lib.restir_image_ready(None, C.byref(ready)) == INVALID
    assert lib.restir_image_ready(None, None) == INVALID
    data = C.c_void_p()
    assert lib.restir_image_wait(None, C.byref(data)) == INVALID
    assert lib.restir_image_wait(None, None) == INVALID
    assert not data.value
    buf = (C.c_uint8 * 16)()
    assert lib.restir_download_rgba8(None, buf, 4) == INVALID
    assert lib.restir_download_rgba8(None, None, 4) == INVALID
    assert bytes(buf) == bytes(16)
    assert lib.restir_write_image_bmp(None, b"/nonexistent/x.bmp") == INVALID
    assert lib.restir_write_image_bmp(None, None) == INVALID


def test_release_of_null_is_a_no_op(abi_lib):
    assert abi_lib.restir_image_release(None) is None


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (70, 37)])
def test_bmp_header_is_encode_bmps(abi_lib, W, H):
    lib = abi_lib
    n = C.c_size_t()
    assert lib.restir_bmp_header(W, H, None, 0, C.byref(n)) == 0 and n.value == 122
    head = (C.c_uint8 * 122)()
    assert lib.restir_bmp_header(W, H, head, 121, C.byref(n)) == INVALID
    assert lib.restir_bmp_header(W, H, head, 122, C.byref(n)) == 0
    rgb = np.random.default_rng(W * 131 + H).random((H, W, 3), np.float32)
    assert lib.restir_encode_bmp(rgb.ctypes.data, W, H, None, 0, C.byref(n)) == 0
    file = (C.c_uint8 * n.value)()
    assert lib.restir_encode_bmp(rgb.ctypes.data, W, H, file, n.value, C.byref(n)) == 0
    assert bytes(file)[:122] == bytes(head) and n.value == 122 + W * H * 4
