"""restir_accum_fold (include/restir_c.h "accumulating frames"), pure host: the three-line float32 recurrence of
csrc/accum.h against numpy bit for bit, the sign of m2, and the argument errors of every accumulation entry point.
No GPU: the device's side of the same header is tests/test_gpu_accum.py."""
import ctypes as C

import numpy as np
import pytest

from romis_amd import _abi, restir

INVALID = 1
FP = C.POINTER(C.c_float)
F32 = np.float32


def fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def hashed(count, salt):
    return fmix32(np.arange(count, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.uint32(salt)).view(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,   # +-0, denormals
                0x7F7FFFFF, 0xFF7FFFFF, 0x3F7FFFFF, 0x3F800000, 0x3F800001, 0xBF7FFFFF, 0xBF800000, 0xBF800001]
NONFINITE_BITS = [0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA55A5A]


def numpy_fold(mean, m2, x, n):
    """The recurrence in numpy float32, one rounding per operation: returns (mean', m2')."""
    with np.errstate(all="ignore"):
        inv_n = F32(1.0) / F32(n)
        d = x - mean
        mean2 = mean + d * inv_n
        m22 = m2 + d * (x - mean2)
    assert mean2.dtype == F32 and m22.dtype == F32
    return mean2, m22


def same(got, want):
    """Bit for bit where the wanted value is finite or an infinity; a NaN for a NaN (payload and sign are not part of the
    contract)."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def frames(count, nframes, special):
    """nframes images of `count` floats: hashed finite bit patterns, `special` cycled through every position."""
    out = []
    for n in range(nframes):
        x = hashed(count, 0x7F4A7C15 + 977 * n)
        x = x[np.isfinite(x)]
        x = np.resize(x, count).copy()
        s = np.array(special, np.uint32).view(F32)
        at = (np.arange(len(s)) * 7 + 13 * n) % count
        x[at] = np.roll(s, n)
        out.append(x)
    return out


@pytest.mark.parametrize("variance", [True, False])
def test_fold_matches_numpy_bit_for_bit(abi_lib, variance):
    count = 4096
    mean, m2 = np.zeros(count, F32), np.zeros(count, F32)
    wm, w2 = mean.copy(), m2.copy()
    for n, x in enumerate(frames(count, 9, SPECIAL_BITS), start=1):
        assert np.isfinite(x).all()
        assert abi_lib.restir_accum_fold(mean.ctypes.data_as(FP), m2.ctypes.data_as(FP) if variance else None,
                                         x.ctypes.data_as(FP), count, n) == 0
        wm, w2n = numpy_fold(wm, w2, x, n)
        if variance:
            w2 = w2n
        assert same(mean, wm), f"mean after frame {n}"
        assert same(m2, w2), f"m2 after frame {n}"
    assert not variance or (m2 != 0).any()
    assert variance or not m2.any()   # untouched without the plane


def test_fold_propagates_non_finite_values_like_numpy(abi_lib):
    count = 257
    mean, m2 = np.zeros(count, F32), np.zeros(count, F32)
    wm, w2 = mean.copy(), m2.copy()
    for n, x in enumerate(frames(count, 9, SPECIAL_BITS + NONFINITE_BITS), start=1):
        restir.accum_fold(mean, m2, x, n)
        wm, w2 = numpy_fold(wm, w2, x, n)
        for got, want in ((mean, wm), (m2, w2)):
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), n
            fin = np.isfinite(want)
            assert np.array_equal(bits(got)[fin], bits(want)[fin]), n
    assert np.isnan(mean).any() and np.isfinite(mean).any()


def test_m2_is_never_negative_on_finite_states(abi_lib):
    """From the empty state the mean moves towards x by at most the whole way (inv_n <= 1 and rounding is monotone), so
    d and x - mean' never have opposite signs and every product added to m2 is >= 0."""
    count = 4096
    mean, m2 = np.zeros(count, F32), np.zeros(count, F32)
    for n, x in enumerate(frames(count, 9, SPECIAL_BITS), start=1):
        restir.accum_fold(mean, m2, x, n)
        fin = np.isfinite(mean) & np.isfinite(m2)
        assert fin.any() and (m2[fin] >= 0).all(), n
    # small values too, where most hashed patterns (huge magnitudes) do not reach
    mean[:], m2[:] = 0, 0
    for n in range(1, 10):
        x = (hashed(count, 31 * n).view(np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -20) - F32(4.0)
        restir.accum_fold(mean, m2, x, n)
        assert np.isfinite(m2).all() and (m2 >= 0).all(), n
    assert (m2 > 0).all()


def test_argument_errors(abi_lib):
    lib = abi_lib
    a = np.zeros(4, F32)
    p = a.ctypes.data_as(FP)
    assert lib.restir_accum_begin(None, 0) == INVALID
    assert lib.restir_accum_add(None) == INVALID
    assert lib.restir_accum_resolve(None, None) == INVALID
    assert lib.restir_accum_stats_get(None, C.byref(_abi.AccumStats())) == INVALID
    assert lib.restir_accum_download(None, p, None, 4) == INVALID
    assert lib.restir_accum_end(None) == INVALID
    cam, f, req = _abi.Camera(), _abi.default_features(), _abi.AccumRequest(max_frames=1)
    assert lib.restir_render_accumulate(None, C.byref(cam), C.byref(f), 4, 4, None, C.byref(req), None, None) == INVALID
    assert b"NULL" in lib.restir_last_error()
    assert lib.restir_accum_fold(None, None, p, 4, 1) == INVALID
    assert lib.restir_accum_fold(p, None, None, 4, 1) == INVALID
    for n in (0, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF):
        assert lib.restir_accum_fold(p, p, p, 4, n) == INVALID, n
    assert not a.any()
    assert lib.restir_accum_fold(p, None, p, 4, (1 << 24) - 1) == 0    # the last count whose (float)n is exact
    assert _abi.RESTIR_ACCUM_MAX_FRAMES == (1 << 24) - 1 and _abi.RESTIR_ABI_VERSION == 5
