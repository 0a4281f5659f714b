"""restir_denoise_host on the CPU (csrc/denoise.h / denoise_host.cpp; no GPU): the edge-avoiding a-trous filter equals its
numpy restatement (tests/denoise_spec.py) bit for bit, no tolerance -- on hand-made G-buffers that isolate one rule each
(the plain B3 filter with its border renormalisation, a material edge, misses, opposed / zero / NaN normals, NaN and inf
colours, the smallest sizes) and on the oracle's nightclub G-buffer with a C2 frame at 70 x 37 for every iteration count
and three normal exponents.  Also every RESTIR_ERR_INVALID case, the defaults and struct sizes, and the stand-alone
program tests/cpp/denoise_host_check.cpp built with -fsanitize=address,undefined over the host unit compiled with the
same flags, run on ragged sizes and compared with the library's answer on the same inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_spec as spec
from romis_amd import _abi, build, restir, scene

F32, U32 = np.float32, np.uint32
FP = C.POINTER(C.c_float)
INVALID = 1
NIGHT = "nightclub_128pt"
# a bound on one level's error on a constant image of at most 1: 25 adds of sw, 25 multiplies and adds of sc, one divide
ROUNDINGS = 76 * 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def assert_bits(got, want, what):
    g, w_ = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w_.shape, f"{what}: shape {g.shape} != {w_.shape}"
    bad = np.flatnonzero(g != w_)
    assert bad.size == 0, f"{what}: {bad.size}/{g.size} words differ; first idx {bad[:4].tolist()} " \
                          f"got {g[bad[:4]].view(F32).tolist()} want {w_[bad[:4]].view(F32).tolist()}"


def c2(**kw):
    """bench.py's C2: N = 1, M = 32, k = 5, r = 10, one biased pass, no temporal reuse"""
    return _abi.default_features(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5,
                                 spatial_resample_radius=10, spatial_reuse=1, temporal_reuse=0,
                                 spatial_resampling_passes=1, **kw)


@pytest.fixture(scope="module")
def lib(abi_lib):
    return abi_lib


def noise(w, h, seed=5, scale=4.0):
    return (np.random.default_rng(seed).random((h, w, 3)) * scale).astype(F32)


def both(rgb, n_t, p_mat, miss, what, iterations=3, npl2=5, sigma=0.01):   # (three levels unless a test says otherwise)
    """the host function's image, asserted equal to the specification's"""
    p = restir.denoise_params(iterations, npl2, sigma)
    got = restir.denoise_host(rgb, n_t, p_mat, miss, p)
    want = spec.denoise(rgb, n_t, p_mat, miss, iterations, npl2, sigma)
    assert_bits(got, want, what)
    return got


# ---- hand-made G-buffers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
def test_one_plane_one_material_is_the_plain_b3_filter(lib, iterations):
    """Every edge weight is h: cn = 1 (the same normal), e = 0 (P in the plane) -- the output is the B3 filter of the
    image renormalised at the border, so a constant image stays constant to a rounding and noise gets smoother."""
    w, h = 23, 11
    n_t, p_mat = spec.plane_gbuffer(w, h)
    rgb = noise(w, h)
    got = both(rgb, n_t, p_mat, 7, f"plane, {iterations} levels", iterations=iterations)
    assert got.var() < rgb.var() and np.isfinite(got).all()
    flat = both(np.full((h, w, 3), 0.75, F32), n_t, p_mat, 7, "constant image", iterations=iterations)
    assert np.abs(flat - F32(0.75)).max() <= ROUNDINGS * iterations
    # level 0 in the interior, by hand: the 5 x 5 B3 mask in double
    if iterations == 1:
        k = np.array([1, 4, 6, 4, 1], np.float64) / 16
        ref = sum(k[a] * k[b] * rgb[3 + a - 2, 5 + b - 2].astype(np.float64) for a in range(5) for b in range(5))
        assert np.allclose(got[3, 5], ref, rtol=1e-5)


def test_two_materials_do_not_mix(lib):
    w, h = 21, 9
    n_t, p_mat = spec.plane_gbuffer(w, h)
    left = np.zeros((h, w), bool)
    left[:, :10] = True
    spec.set_material(p_mat, w, h, ~left, 1)
    rgb = np.zeros((h, w, 3), F32)
    rgb[~left] = 1.0
    got = both(rgb, n_t, p_mat, 7, "two materials", iterations=5)
    assert not bits(got[left]).any(), "the 0 side must stay +0 bits"
    assert np.abs(got[~left] - 1.0).max() <= ROUNDINGS * 5


def test_miss_pixels_mix_only_among_themselves(lib):
    w, h = 19, 10
    n_t, p_mat = spec.plane_gbuffer(w, h, material=2)
    miss = np.zeros((h, w), bool)
    miss[:4] = True
    spec.set_material(p_mat, w, h, miss, 7)
    nt = n_t.reshape(h, w, 4)
    nt[::-1][miss] = (0.0, 0.0, 0.0, -1.0)   # a miss record: no normal, and a t no plane term could use
    rgb = noise(w, h)
    rgb[miss] += 100.0
    got = both(rgb, n_t, p_mat, 7, "misses", iterations=4)
    assert got[miss].min() >= 100.0 and got[~miss].max() <= 4.0 and np.isfinite(got).all()
    assert got[miss].var() < rgb[miss].var()


def test_opposed_normals_do_not_mix(lib):
    w, h = 16, 8
    n_t, p_mat = spec.plane_gbuffer(w, h)
    nt = n_t.reshape(h, w, 4)
    nt[:, 8:, 2] = -2.0
    rgb = np.zeros((h, w, 3), F32)
    rgb[:, 8:] = 1.0
    got = both(rgb, n_t, p_mat, 7, "opposed normals", iterations=3)
    assert not bits(got[:, :8]).any() and np.abs(got[:, 8:] - 1.0).max() <= ROUNDINGS * 5


def test_zero_and_nan_normals_are_flat(lib):
    """A zero-length and a NaN normal make their pixels flat: among surface pixels of their material they exchange
    nothing (exactly one is flat), with each other -- both flat -- they do."""
    w, h = 12, 6
    n_t, p_mat = spec.plane_gbuffer(w, h)
    nt = n_t.reshape(h, w, 4)[::-1]   # image rows
    nt[2, 3, :3] = 0.0
    nt[2, 4, 1] = np.nan
    rgb = np.zeros((h, w, 3), F32)
    rgb[2, 3], rgb[2, 4] = 8.0, 16.0
    got = both(rgb, n_t, p_mat, 7, "zero and NaN normals", iterations=1)
    others = np.ones((h, w), bool)
    others[2, 3] = others[2, 4] = False
    assert not bits(got[others]).any() and np.isfinite(got).all()
    # the two flat pixels: (3/8 . 3/8 . a + 3/8 . 1/4 . b) / (3/8 . 3/8 + 3/8 . 1/4)
    assert np.allclose(got[2, 3], (9 * 8 + 6 * 16) / 15) and np.allclose(got[2, 4], (9 * 16 + 6 * 8) / 15)


def test_nan_and_inf_pixels_pass_through_and_spread_nowhere(lib):
    w, h = 17, 9
    n_t, p_mat = spec.plane_gbuffer(w, h)
    rgb = noise(w, h)
    rgb[4, 8, 1] = np.nan
    rgb[1, 2, 0] = np.inf
    for iterations in (1, 5):
        got = both(rgb, n_t, p_mat, 7, "NaN and inf pixels", iterations=iterations)
        assert_bits(got[4, 8], rgb[4, 8], "the NaN pixel")
        assert_bits(got[1, 2], rgb[1, 2], "the inf pixel")
        rest = np.ones((h, w), bool)
        rest[4, 8] = rest[1, 2] = False
        assert np.isfinite(got[rest]).all()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2)])
def test_smallest_sizes(lib, w, h):
    n_t, p_mat = spec.plane_gbuffer(w, h)
    rgb = noise(w, h)
    for iterations in (1, 3, 5):
        got = both(rgb, n_t, p_mat, 7, f"{w}x{h}", iterations=iterations)
        if (w, h) == (1, 1):
            assert np.allclose(got, rgb, rtol=1e-6)   # the centre tap alone: h c / h


def test_plane_term_cuts_a_depth_step(lib):
    """Two parallel planes one behind the other, one material, one normal: only the plane term tells them apart."""
    w, h = 16, 8
    n_t, p_mat = spec.plane_gbuffer(w, h)
    pm = p_mat.reshape(h, w, 4)
    pm[:, 8:, 2] = 1.0   # 1 unit behind: e = 1 against sigma t = 0.05
    rgb = np.zeros((h, w, 3), F32)
    rgb[:, 8:] = 1.0
    got = both(rgb, n_t, p_mat, 7, "depth step", iterations=3)
    assert not bits(got[:, :8]).any() and np.abs(got[:, 8:] - 1.0).max() <= ROUNDINGS * 5
    wide = both(rgb, n_t, p_mat, 7, "depth step, a support that spans it", iterations=3, sigma=1.0)
    assert (wide[:, 7] > 0).all() and (wide[:, 8] < 1).all()


# ---- the oracle's G-buffer and frame --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def night_frame(oracle):
    sc = scene.bench_scene(NIGHT)
    w, h = 70, 37
    rgb, _, (n_t, p_mat) = oracle.render_frame(oracle.OracleScene(sc), scene.nightclub_camera(w, h),
                                               c2(enable_tone_mapping=0), w, h)
    for a in (rgb, n_t, p_mat):
        a.flags.writeable = False
    return rgb, n_t, p_mat, len(sc.meshes)


@pytest.mark.parametrize("npl2", [0, 5, 7])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
def test_nightclub_c2_frame(lib, night_frame, iterations, npl2):
    rgb, n_t, p_mat, miss = night_frame
    assert (bits(p_mat[:, 3]) == miss).any() and (bits(p_mat[:, 3]) != miss).any(), "the frame sees surface and background"
    got = both(rgb, n_t, p_mat, miss, f"nightclub C2, {iterations} levels, 2^{npl2}", iterations=iterations, npl2=npl2)
    assert np.isfinite(got).all() and got.var() < rgb.var()


# ---- arguments, defaults, sizes -------------------------------------------------------------------------------------------
def test_defaults_sizes_and_abi_version(lib):
    p = _abi.DenoiseParams(9, 9, 9.0, 9)
    lib.restir_denoise_params_default(C.byref(p))
    assert (p.iterations, p.normal_power_log2, p.flags) == (2, 5, 0) and p.sigma_plane == F32(0.01)
    assert C.sizeof(_abi.DenoiseParams) == 16 and _abi.RESTIR_DENOISE_MAX_ITERATIONS == 5
    assert lib.restir_abi_version() == 5 == _abi.RESTIR_ABI_VERSION
    lib.restir_denoise_params_default(None)   # tolerated


def test_invalid_arguments(lib):
    w, h = 4, 3
    n_t, p_mat = spec.plane_gbuffer(w, h)
    rgb, out = noise(w, h), np.full((h, w, 3), 7.0, F32)
    a = [x.ctypes.data_as(FP) for x in (rgb, n_t, p_mat, out)]

    def call(rgb=a[0], nt=a[1], pm=a[2], w_=w, h_=h, p=restir.denoise_params(), o=a[3]):
        return lib.restir_denoise_host(rgb, nt, pm, w_, h_, 7, C.byref(p) if p is not None else None, o)

    assert call() == 0
    out[:] = 7.0
    for kw in ({"rgb": None}, {"nt": None}, {"pm": None}, {"o": None}, {"p": None}, {"w_": 0}, {"h_": 0},
               {"p": restir.denoise_params(iterations=0)}, {"p": restir.denoise_params(iterations=6)},
               {"p": restir.denoise_params(normal_power_log2=8)}, {"p": restir.denoise_params(sigma_plane=0.0)},
               {"p": restir.denoise_params(sigma_plane=-1.0)}, {"p": restir.denoise_params(sigma_plane=float("nan"))},
               {"p": restir.denoise_params(sigma_plane=float("inf"))}, {"p": _abi.DenoiseParams(3, 5, 0.01, 1)}):
        assert call(**kw) == INVALID, kw
        assert lib.restir_last_error(), kw
        assert (out == 7.0).all(), f"{kw}: the output was written"
    with pytest.raises(ValueError):
        restir.denoise_host(rgb, n_t[:-1], p_mat, 7)


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------
def lcg_inputs(w, h):
    """tests/cpp/denoise_host_check.cpp's inputs"""
    state = [(w * 7919 + h) & 0xFFFFFFFF]

    def nxt():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        return F32(state[0] >> 8) * F32(1.0 / 16777216.0)

    npx, miss = w * h, 3
    rgb, n_t, p_mat = np.zeros((npx, 3), F32), np.zeros((npx, 4), F32), np.zeros((npx, 4), F32)
    mat = np.zeros(npx, U32)
    for i in range(npx):
        x, y = F32(i % w), F32(i // w)
        n_t[i] = (nxt() - F32(0.5), nxt() - F32(0.5), F32(1.0) + nxt(), F32(4.0) + nxt())
        p_mat[i, :3] = (F32(0.05) * x, F32(0.05) * y, F32(0.02) * nxt())
        m = nxt()
        mat[i] = miss if m < F32(0.1) else int(x * F32(3.0) / F32(w))
        rgb[i] = [F32(4.0) * nxt() for _ in range(3)]
    p_mat[:, 3] = mat.view(F32)
    if npx > 4:
        n_t[1, :3] = 0.0
        n_t[2, 1] = np.nan
        rgb[3, 1] = np.nan
        rgb[npx - 1, 2] = np.inf
    return rgb.reshape(h, w, 3), n_t, p_mat, miss


def fnv1a(data: bytes) -> int:
    hsh = 1469598103934665603
    for b in data:
        hsh = ((hsh ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return hsh


@pytest.fixture(scope="module")
def san_tool(tmp_path_factory):
    exe = tmp_path_factory.mktemp("denoise_san") / "denoise_host_check_san"
    srcs = [os.path.join(build.ROOT, "tests", "cpp", "denoise_host_check.cpp"),
            os.path.join(build.CSRC, "denoise_host.cpp"), os.path.join(build.CSRC, "abi_error.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{build.CSRC}", f"-I{os.path.join(build.ROOT, 'include')}"] + srcs +
                   ["-o", str(exe)], check=True, timeout=300)
    return str(exe)


@pytest.mark.parametrize("w,h,iterations,npl2", [(1, 1, 5, 5), (3, 2, 5, 0), (37, 5, 3, 5), (33, 17, 5, 7), (70, 37, 4, 5)])
def test_stand_alone_program_under_address_and_undefined_sanitizers(lib, san_tool, w, h, iterations, npl2):
    """The program (its own main) and the host unit, both built with -fsanitize=address,undefined; its answer is the
    library's on the same inputs, and the specification's."""
    r = subprocess.run([san_tool, str(w), str(h), str(iterations), str(npl2)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rgb, n_t, p_mat, miss = lcg_inputs(w, h)
    got = both(rgb, n_t, p_mat, miss, f"LCG inputs {w}x{h}", iterations=iterations, npl2=npl2)
    words = r.stdout.split()
    assert words[0] == "hash" and int(words[1], 16) == fnv1a(got.tobytes()), r.stdout
    assert int(words[3]) == int((~np.isfinite(got)).sum()) == (2 if w * h > 4 else 0)
