"""restir_denoise_lum_host on the CPU (csrc/denoise.h / denoise_host.cpp; no GPU): the a-trous filter with the
variance-guided luminance term.

1  it equals its numpy restatement (tests/denoise_lum_spec.py) bit for bit, colour and variance: the oracle's nightclub and
   monkey16 G-buffers with a C2 frame at 33 x 17, 70 x 37 and 130 x 70, one to five levels, with the spatial estimate
   (var == NULL) and with an explicit plane; an image with NaN and inf pixels; an explicit plane holding NaN, inf and
   negative entries; the smallest sizes;
2  it contains the old filter: var = 1, sigma_lum = 1e30 gives restir_denoise_host's colour bit for bit;
3  a lighting edge survives where restir_denoise_host blurs it;
4  defaults, struct size, the ABI version and every RESTIR_ERR_INVALID case."""
import ctypes as C

import numpy as np
import pytest

import denoise_lum_spec as lspec
import denoise_spec as spec
from romis_amd import _abi, restir
from test_denoise_host import assert_bits, bits, c2, noise
from test_gpu_exact import NIGHT, SEED, oscene, the_camera, the_scene

F32, U32 = np.float32, np.uint32
FP = C.POINTER(C.c_float)
INVALID = 1
SIZES = [(33, 17), (70, 37), (130, 70)]
MONKEY = "monkey16"
CAMS = {NIGHT: None, MONKEY: "toml"}


@pytest.fixture(scope="module")
def lib(abi_lib):
    return abi_lib


_frames = {}


def frame(oracle, name, w, h):
    """(rgb, n_t, p_mat, miss material) of the oracle's linear C2 frame 0 of the view, computed once"""
    k = (name, w, h)
    if k not in _frames:
        rgb, _, (n_t, p_mat) = oracle.render_frame(oscene(oracle, name), the_camera(name, CAMS[name], w, h),
                                                   c2(enable_tone_mapping=0), w, h, SEED, 0)
        for a in (rgb, n_t, p_mat):
            a.flags.writeable = False
        _frames[k] = (rgb, n_t, p_mat, len(the_scene(name).meshes))
    return _frames[k]


def plane(w, h, seed=11, scale=2.0):
    return (np.random.default_rng(seed).random((h, w)) ** 4 * scale).astype(F32)


def both(rgb, var, n_t, p_mat, miss, what, iterations=2, npl2=5, sigma=0.01, sigma_lum=4.0):
    """the host function's (image, variance), asserted equal to the specification's"""
    p = restir.denoise_lum_params(iterations, npl2, sigma, sigma_lum=sigma_lum)
    got, got_v = restir.denoise_lum_host(rgb, n_t, p_mat, miss, p, var=var)
    want, want_v = lspec.denoise(rgb, var, n_t, p_mat, miss, iterations, npl2, sigma, sigma_lum)
    assert_bits(got, want, what + ": colour")
    assert_bits(got_v, want_v, what + ": variance")
    return got, got_v


# ---- 1: the host function against numpy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHT, MONKEY])
def test_host_equals_the_specification(lib, oracle, name, w, h):
    rgb, n_t, p_mat, miss = frame(oracle, name, w, h)
    hit = bits(p_mat[:, 3]) != miss
    assert hit.sum() >= 32 and (~hit).sum() >= 32, "the view sees surface and background"
    explicit = plane(w, h)
    for iterations in range(1, 6):
        got, got_v = both(rgb, None, n_t, p_mat, miss, f"{name} {w}x{h}, spatial, {iterations} levels", iterations=iterations)
        assert np.isfinite(got).all() and np.isfinite(got_v).all() and (got_v >= 0).all()
        exp, _ = both(rgb, explicit, n_t, p_mat, miss, f"{name} {w}x{h}, explicit, {iterations} levels", iterations=iterations,
                      sigma_lum=2.0)
        assert not np.array_equal(bits(got), bits(exp)) and not np.array_equal(bits(got), bits(rgb))
    # the term matters in this view: it is not restir_denoise_host's image
    old = restir.denoise_host(rgb, n_t, p_mat, miss, restir.denoise_params(iterations=2))
    assert not np.array_equal(bits(both(rgb, None, n_t, p_mat, miss, "defaults")[0]), bits(old))


def test_nan_and_inf_pixels(lib, oracle):
    w, h = 70, 37
    rgb, n_t, p_mat, miss = frame(oracle, NIGHT, w, h)
    img = np.array(rgb)
    img[4, 8, 1] = np.nan
    img[1, 2, 0] = np.inf
    img[h - 1, w - 1, 2] = -np.inf
    img[20, 30] = np.array([0x7FC00000, 0xFFA55A5A, 0x7F800000], U32).view(F32)
    bad = ~np.isfinite(img).all(axis=-1)
    assert bad.sum() == 4
    for var in (None, plane(w, h)):
        for iterations in (1, 3, 5):
            got, got_v = both(img, var, n_t, p_mat, miss, f"NaN and inf pixels, {iterations} levels", iterations=iterations)
            assert_bits(got[bad], img[bad], "the pixels that are not finite")
            assert np.isfinite(got[~bad]).all()
            want_v = np.zeros(4, F32) if var is None else lspec.clean(var)[bad]
            assert_bits(got_v[bad], want_v, "their variance stays")


def test_explicit_plane_with_nan_inf_and_negative_entries(lib, oracle):
    w, h = 33, 17
    rgb, n_t, p_mat, miss = frame(oracle, NIGHT, w, h)
    var = plane(w, h)
    var[3, 4], var[5, 6], var[7, 8], var[9, 10], var[0, 0] = np.nan, np.inf, -np.inf, -2.5, -0.0
    cleaned = lspec.clean(var)
    assert not bits(cleaned[[3, 5, 7, 9, 0], [4, 6, 8, 10, 0]]).any(), "stored as +0"
    for iterations in (1, 2, 5):
        got, got_v = both(rgb, var, n_t, p_mat, miss, f"a dirty plane, {iterations} levels", iterations=iterations)
        same, same_v = restir.denoise_lum_host(rgb, n_t, p_mat, miss, restir.denoise_lum_params(iterations=iterations), var=cleaned)
        assert_bits(got, same, "the cleaned plane gives the same image")
        assert_bits(got_v, same_v, "and the same variance")
        assert np.isfinite(got).all() and np.isfinite(got_v).all()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2)])
def test_smallest_sizes(lib, w, h):
    n_t, p_mat = spec.plane_gbuffer(w, h)
    rgb = noise(w, h)
    for var in (None, plane(w, h)):
        for iterations in (1, 3, 5):
            both(rgb, var, n_t, p_mat, 7, f"{w}x{h}", iterations=iterations)


# ---- 2: it contains the old filter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [(NIGHT, 70, 37), (MONKEY, 130, 70)])
def test_contains_the_geometry_only_filter(lib, oracle, name, w, h):
    """var = 1 and sigma_lum = 1e30: inv_den <= 1e-30 at level 0, r <= 1e6 inv_den, r r underflows far below half an ulp
    of 1, so 1.0f + r r == 1.0f and wl == 1.0f exactly: every weight is restir_denoise_host's.  A level's v = sum w^2 v_q /
    (sum w)^2 is at least min v_q / 25 (Cauchy-Schwarz over at most 25 taps): after four levels v >= 25^-4, sqrt(gv) >=
    1.6e-3, inv_den below 1e-27 and r r below 1e-42."""
    rgb, n_t, p_mat, miss = frame(oracle, name, w, h)
    assert np.isfinite(rgb).all() and np.abs(rgb).max() < 1e6
    ones = np.ones((h, w), F32)
    for iterations in range(1, 6):
        p = restir.denoise_lum_params(iterations=iterations, sigma_lum=1e30)
        got, _ = restir.denoise_lum_host(rgb, n_t, p_mat, miss, p, var=ones)
        assert_bits(got, restir.denoise_host(rgb, n_t, p_mat, miss, restir.denoise_params(iterations=iterations)),
                    f"{name} {w}x{h}, {iterations} levels")


# ---- 3: a lighting edge survives --------------------------------------------------------------------------------------------
def test_a_lighting_edge_survives(lib):
    """One plane, one material, a vertical unit step in luminance, var = 0, two levels: den = 1e-6, r = 1e6 across the edge,
    wl <= 1e-12 -- no pixel moves by more than 1e-6.  restir_denoise_host takes 5/16 of the weight of a pixel next to the
    edge from the other side at level 0 alone: it moves those pixels by more than 0.25."""
    w, h = 24, 12
    n_t, p_mat = spec.plane_gbuffer(w, h)
    rgb = np.zeros((h, w, 3), F32)
    rgb[:, w // 2:] = 1.0
    assert abs(float(lspec.lum(rgb)[0, w // 2]) - 1.0) < 1e-6 and lspec.lum(rgb)[0, 0] == 0
    p = restir.denoise_lum_params(iterations=2)
    got, got_v = both(rgb, np.zeros((h, w), F32), n_t, p_mat, 7, "a step", iterations=2, sigma_lum=p.sigma_lum)
    moved = np.abs(got - rgb).max()
    print(f"the step under restir_denoise_lum_host: max move {moved:.3e}")
    assert moved <= 1e-6
    assert not bits(got_v).any(), "no variance comes from nowhere"
    old = restir.denoise_host(rgb, n_t, p_mat, 7, restir.denoise_params(iterations=2))
    beside = np.abs(old - rgb)[:, [w // 2 - 1, w // 2]]
    print(f"the step under restir_denoise_host: the pixels beside it move by {beside.min():.4f} .. {beside.max():.4f}")
    assert beside.min() >= 0.25


# ---- 4: arguments, defaults, sizes -------------------------------------------------------------------------------------------
def test_defaults_sizes_and_abi_version(lib):
    p = _abi.DenoiseLumParams(_abi.DenoiseParams(9, 9, 9.0, 9), 9, 9.0, 9)
    lib.restir_denoise_lum_params_default(C.byref(p))
    g = restir.denoise_params()
    assert (p.geo.iterations, p.geo.normal_power_log2, p.geo.sigma_plane, p.geo.flags) == \
        (g.iterations, g.normal_power_log2, g.sigma_plane, 0)
    assert (p.variance_source, p.flags) == (_abi.RESTIR_DENOISE_VAR_SPATIAL, 0) and p.sigma_lum > 0
    assert (_abi.RESTIR_DENOISE_VAR_SPATIAL, _abi.RESTIR_DENOISE_VAR_ACCUM) == (0, 1)
    assert C.sizeof(_abi.DenoiseLumParams) == 28 and C.sizeof(_abi.DenoiseParams) == 16
    assert lib.restir_abi_version() == 5 == _abi.RESTIR_ABI_VERSION
    lib.restir_denoise_lum_params_default(None)   # tolerated
    q = restir.denoise_lum_params(3, 4, 0.5, _abi.RESTIR_DENOISE_VAR_ACCUM, 2.0)
    assert (q.geo.iterations, q.geo.normal_power_log2, q.geo.sigma_plane, q.variance_source, q.sigma_lum) == (3, 4, 0.5, 1, 2.0)


def test_invalid_arguments(lib):
    w, h = 4, 3
    n_t, p_mat = spec.plane_gbuffer(w, h)
    rgb, out, out_v = noise(w, h), np.full((h, w, 3), 7.0, F32), np.full((h, w), 7.0, F32)
    var = plane(w, h)
    a = [x.ctypes.data_as(FP) for x in (rgb, var, n_t, p_mat, out, out_v)]
    P = restir.denoise_lum_params

    def lum_with(**kw):
        p = P()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(rgb=a[0], var=a[1], nt=a[2], pm=a[3], w_=w, h_=h, p=P(), o=a[4], ov=a[5]):
        return lib.restir_denoise_lum_host(rgb, var, nt, pm, w_, h_, 7, C.byref(p) if p is not None else None, o, ov)

    assert call() == 0 and call(var=None) == 0 and call(ov=None) == 0
    assert call(p=P(variance_source=_abi.RESTIR_DENOISE_VAR_ACCUM)) == 0   # checked, otherwise ignored on the host
    out[:], out_v[:] = 7.0, 7.0
    geo_flags = P()
    geo_flags.geo.flags = 1
    for kw in ({"rgb": None}, {"nt": None}, {"pm": None}, {"o": None}, {"p": None}, {"w_": 0}, {"h_": 0},
               {"p": P(iterations=0)}, {"p": P(iterations=6)}, {"p": P(normal_power_log2=8)}, {"p": P(sigma_plane=0.0)},
               {"p": P(sigma_plane=float("nan"))}, {"p": geo_flags}, {"p": P(variance_source=2)},
               {"p": P(variance_source=0xFFFFFFFF)}, {"p": P(sigma_lum=0.0)}, {"p": P(sigma_lum=-1.0)},
               {"p": P(sigma_lum=float("nan"))}, {"p": P(sigma_lum=float("inf"))}, {"p": lum_with(flags=1)}):
        assert call(**kw) == INVALID, kw
        assert lib.restir_last_error(), kw
        assert (out == 7.0).all() and (out_v == 7.0).all(), f"{kw}: an output was written"
    with pytest.raises(ValueError):
        restir.denoise_lum_host(rgb, n_t[:-1], p_mat, 7)
    with pytest.raises(ValueError):
        restir.denoise_lum_host(rgb, n_t, p_mat, 7, var=var[:-1])
