"""restir_error_measure (include/restir_c.h "a kept reference"), pure host: the error figures of csrc/exact.h against numpy
float64 -- the counts and the maximum exactly, every mean within the worst case of any summation order --, the values
that must be left out, the arithmetic pinned to double, and the argument errors of every entry point of the block.
No GPU: the device's side of the same header is tests/test_gpu_exact.py."""
import ctypes as C

import numpy as np
import pytest

from romis_amd import _abi, restir

INVALID = 1
FP = C.POINTER(C.c_float)
F32 = np.float32
COUNTS = [1, 3, 4095, 4096, 4097, 3 * 70 * 37]
EPS = 1e-2

SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,   # +-0, denormals
                0x7F7FFFFF, 0xFF7FFFFF, 0x3F7FFFFF, 0x3F800000, 0x3F800001, 0xBF7FFFFF, 0xBF800000, 0xBF800001]
NONFINITE_BITS = [0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA55A5A]


def fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def hashed_finite(count, salt):
    """`count` hashed bit patterns, the non-finite ones replaced by finite ones"""
    x = fmix32(np.arange(2 * count + 64, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.uint32(salt)).view(F32)
    x = x[np.isfinite(x)]
    return np.resize(x, count).copy()


def moderate(count, salt):
    """hashed values in [-2, 6): images' range, where the relative term's denominator matters"""
    u = fmix32(np.arange(count, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.uint32(salt))
    return ((u >> np.uint32(8)).astype(F32) * F32(2.0 ** -21) - F32(2.0)).astype(F32)


def sprinkle(x, special, step, start):
    s = np.array(special, np.uint32).view(F32)
    at = (np.arange(len(s)) * step + start) % len(x)
    x[at] = s          # (a later entry wins where two land on one place: counts below 15)
    return x


def numpy_figures(a, r):
    """The definition in float64: dict of the struct's fields, and per mean the worst-case bound of any summation
    order, counted x 2^-52 x sum|term| / counted."""
    ok = np.isfinite(a) & np.isfinite(r)
    n = int(ok.sum())
    with np.errstate(all="ignore"):
        a64, r64 = a.astype(np.float64), r.astype(np.float64)   # (a signalling NaN's cast warns)
        d = a64[ok] - r64[ok]
        terms = dict(mse=d * d, mae=np.abs(d), rel_mse=d * d / (r64[ok] * r64[ok] + EPS), bias=d, ref_mean=r64[ok])
    want = dict(counted=n, nonfinite=int(a.size - n), max_abs=float(np.abs(d).max()) if n else 0.0)
    bound = {}
    for k, t in terms.items():
        want[k] = float(np.sum(t) / n) if n else float("nan")
        bound[k] = float(n * 2.0 ** -52 * np.sum(np.abs(t)) / n) if n else 0.0
    return want, bound


def check_against_numpy(a, r, what):
    got = restir.error_measure(a, r)
    want, bound = numpy_figures(a, r)
    assert (got.width, got.height, got.source, got.frames) == (0, 0, 0, 0), what
    assert got.counted == want["counted"] and got.nonfinite == want["nonfinite"], what
    assert got.max_abs == want["max_abs"], what
    for k, b in bound.items():
        g = getattr(got, k)
        if want["counted"] == 0:
            assert np.isnan(g), (what, k)
            continue
        assert np.isfinite(g) and abs(g - want[k]) <= b, f"{what}: {k} = {g!r}, numpy {want[k]!r}, bound {b!r}"
    return got


@pytest.mark.parametrize("count", COUNTS)
def test_figures_match_numpy_float64(abi_lib, count):
    # hashed finite bit patterns (huge magnitudes: d*d reaches 1e77, far outside float32)
    a, r = hashed_finite(count, 0x7F4A7C15), hashed_finite(count, 0x1B873593)
    got = check_against_numpy(a, r, "hashed")
    assert got.counted == count and got.nonfinite == 0
    # images' range with +-0, denormals and the values next to +-1 and +-FLT_MAX in a, in r, and in both
    a, r = moderate(count, 11), moderate(count, 23)
    sprinkle(a, SPECIAL_BITS, 7, 0)
    sprinkle(r, SPECIAL_BITS, 5, 3)
    sprinkle(a, SPECIAL_BITS[:7], 11, 1)
    sprinkle(r, SPECIAL_BITS[:7], 11, 1)
    got = check_against_numpy(a, r, "special")
    assert got.counted == count


@pytest.mark.parametrize("count", COUNTS)
def test_non_finite_values_are_left_out_and_counted(abi_lib, count):
    a, r = moderate(count, 31), moderate(count, 47)
    sprinkle(a, NONFINITE_BITS, 7, 0)            # in a
    sprinkle(r, NONFINITE_BITS, 5, 2)            # in r
    sprinkle(a, NONFINITE_BITS, 13, 4)           # in both, at the same places
    sprinkle(r, NONFINITE_BITS[::-1], 13, 4)
    got = check_against_numpy(a, r, "nonfinite")
    bad = int((~(np.isfinite(a) & np.isfinite(r))).sum())
    assert bad > 0 and got.nonfinite == bad and got.counted == count - bad
    if got.counted:
        assert np.isfinite([got.mse, got.mae, got.rel_mse, got.bias, got.max_abs, got.ref_mean]).all()


def test_nothing_counted_gives_no_figures(abi_lib):
    a = np.array([np.nan, np.inf, 1.0], F32)
    r = np.array([1.0, 2.0, -np.inf], F32)
    got = check_against_numpy(a, r, "all left out")
    assert got.counted == 0 and got.nonfinite == 3 and got.max_abs == 0.0


def test_the_arithmetic_is_double(abi_lib):
    """FLT_MAX against -FLT_MAX: d = 2 FLT_MAX and d*d = 4.6e77 are finite in double; a difference or a square taken in
    float32 would be inf."""
    big = np.array([0x7F7FFFFF], np.uint32).view(F32)[0]
    d = 2.0 * float(big)
    got = restir.error_measure(np.array([big], F32), np.array([-big], F32))
    assert got.counted == 1 and got.nonfinite == 0
    assert got.max_abs == d and got.mae == d and got.bias == d and got.mse == d * d and got.ref_mean == -float(big)
    assert got.rel_mse == d * d / (float(big) ** 2 + EPS)
    # over more than one block (k d is exact in double for k <= 4097; k d d is not: the bound)
    got = check_against_numpy(np.full(4097, big, F32), np.full(4097, -big, F32), "FLT_MAX against -FLT_MAX")
    assert got.max_abs == d and got.mae == d and got.bias == d and np.isfinite(got.mse) and got.mse > 1e77
    # ... and a small difference of large values is not lost to a float32 subtraction of float64 squares
    a, r = np.array([16777216.0], F32), np.array([16777215.0], F32)
    got = restir.error_measure(a, r)
    assert got.mse == 1.0 and got.mae == 1.0 and got.bias == 1.0 and got.max_abs == 1.0


@pytest.mark.parametrize("count", COUNTS)
def test_equal_arrays_have_zero_error(abi_lib, count):
    a = sprinkle(hashed_finite(count, 99), SPECIAL_BITS, 7, 0)
    got = restir.error_measure(a, a.copy())
    assert got.counted == count and got.nonfinite == 0
    assert (got.mse, got.mae, got.rel_mse, got.bias, got.max_abs) == (0.0, 0.0, 0.0, 0.0, 0.0)
    # +0 against -0 is equal too
    z = restir.error_measure(np.zeros(count, F32), -np.zeros(count, F32))
    assert (z.mse, z.mae, z.rel_mse, z.bias, z.max_abs, z.ref_mean) == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_the_result_does_not_depend_on_the_callers_layout(abi_lib):
    """An image [h][w][3] and its flat copy are the same floats in the same order: the same bits."""
    a, r = moderate(3 * 70 * 37, 5), moderate(3 * 70 * 37, 6)
    flat = restir.error_measure(a, r)
    img = restir.error_measure(a.reshape(37, 70, 3), r.reshape(37, 70, 3))
    assert bytes(flat) == bytes(img)


def test_argument_errors(abi_lib):
    lib = abi_lib
    a = np.ones(4, F32)
    p = a.ctypes.data_as(FP)
    out = _abi.ErrorStats()
    assert lib.restir_error_measure(None, p, 4, C.byref(out)) == INVALID
    assert lib.restir_error_measure(p, None, 4, C.byref(out)) == INVALID
    assert lib.restir_error_measure(p, p, 4, None) == INVALID
    assert b"null" in lib.restir_last_error().lower()
    assert lib.restir_error_measure(p, p, 0, C.byref(out)) == INVALID
    assert b"count" in lib.restir_last_error()
    assert bytes(out) == bytes(_abi.ErrorStats())    # untouched
    assert lib.restir_error_measure(p, p, 4, C.byref(out)) == 0 and out.counted == 4
    cam, f = _abi.Camera(), _abi.default_features()
    assert lib.restir_render_exact(None, C.byref(cam), C.byref(f), 4, 4, None, None) == INVALID
    assert lib.restir_reference_set(None) == INVALID
    assert lib.restir_reference_clear(None) == INVALID
    w, h, present = C.c_uint32(), C.c_uint32(), C.c_int()
    assert lib.restir_reference_info(None, C.byref(w), C.byref(h), C.byref(present)) == INVALID
    assert lib.restir_error_get(None, 0, C.byref(out)) == INVALID
    assert b"ull" in lib.restir_last_error()
    assert _abi.RESTIR_ERROR_SRC_IMAGE == 0 and _abi.RESTIR_ERROR_SRC_ACCUM_MEAN == 1 and _abi.RESTIR_ERROR_REL_EPS == EPS
    assert _abi.RESTIR_ABI_VERSION == 5 and lib.restir_abi_version() == 5
