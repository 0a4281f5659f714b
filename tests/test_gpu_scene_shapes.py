"""Scene shapes the other GPU tests never render: a BVH past the LDS budget, point-light counts that are no power of
two (up to the handle formats' index limit), light grids that are not square, and light sets of mixed types.

The other files render five kinds of scene -- the 166-triangle nightclub with 128 point lights or 512 parallelograms,
the Cornell box under a 32 x 32 / 64 x 64 light grid or one light, the cube with one segment light.  Four properties of
those scenes keep code from running at all:

A  the BVH fits LDS (route.h: bvh_lds_bytes(s) <= kLdsBudget), so restir_render always takes k_primary_ris and the
   _lds / _sorted kernels.  Monkey (968 triangles, smooth normals, 2 point lights; 89 KB of nodes and triangles at
   bvh.max_leaf = 2) takes k_primary + k_ris, k_final_n{N}, k_spatial1_ntl / k_spatial2_ntl over reservoir planes with
   no tile flags, k_spatial1u, the general k_spatial_n1_unbiased with its shadow rays over the global BVH, a separate
   k_temporal, and initial-visibility rays from global memory.  The knobs primary.lds = 0, final.lds = 0 and
   fuse.primary_ris = 0 force the same kernels on the small scenes, and a larger leaf makes Monkey fit LDS beside the
   light table and the fused last pass's ray phase.
B  the light count is a power of two, so ris_pixel weighs pdf * light_scale.  L = 3, 126, 254, 255 take pdf / (1 / L)
   (the forms differ in float32 on 4 - 70 % of pdfs), __umulhi(d, L) for such L, the two-plane light_c2 table at odd
   offsets and ragged LDS copy loops.  L = 254 is the last count the point-light handles (M | index << 24, index L the
   zero sample) admit, L = 255 the first that falls back to the reservoir planes.
C  the light grid is square.  3 x 4, 24 x 32 and 31 x 32 are regular grids (ny a power of two) with nx != ny, 5 x 3 is
   a grid that is not regular.
D  the light set has one type.  17 lights cycling parallelogram / point / segment diverge sample_rec's type branch
   (0, 1 or 2 extra draws) inside every wave; 5 segment lights; and the mixed set repeated to 585 and 586 lights is
   the last general 112-byte table that is staged in LDS and the first that is read from global memory.

Every test first asserts, through restir_scene_info, the property it exists for.  The bar is the project's: every word
of n_t, p_mat, res_a, res_b, res_dbg, RGB and the returned grid equals the oracle's; no tolerance anywhere.

70 x 37 is 3 x 5 tiles of 32 x 8, ragged on both axes; 33 x 17 is one pixel past a 32 x 16 tile on each axis.  The
oracle's G-buffers, RIS reservoirs and frames are computed once per (scene, camera, size, features), shared between
the tests and never written to.  Every knob is restored in a finally clause.
"""
import contextlib
import copy

import numpy as np
import pytest

from romis_amd import _abi, scene
from test_gpu_fused_final import same_grid, same_rgb
from test_gpu_parity import SEED, assert_bits, assert_grid, get_scene, key, oracle_ris, origin

pytestmark = pytest.mark.gpu

W, H = 70, 37
W2, H2 = 33, 17
LDS_BUDGET = 65536
NIGHT, CORNELL = "nightclub_128pt", "cornell_1024"

KNOB_DEFAULTS = {"spatial.th": 0, "spatial.gather": 1, "spatial.handles": 1, "spatial.n2h": 1, "final.fuse": 1,
                 "primary.lds": 1, "final.lds": 1, "fuse.primary_ris": 1, "ris.compact": 1, "ris.lds": 1,
                 "bvh.max_leaf": 2, "primary.tl": 1, "final.qbvh": 2, "final.sort": 1}


@pytest.fixture(scope="module")
def gpu():
    from romis_amd import build, restir
    build.build()
    r = restir.Renderer(0)
    yield r
    r.close()


@contextlib.contextmanager
def knobs(gpu, **kw):
    """Tuning knobs ("spatial_th" for "spatial.th") for the block, the library's defaults after it."""
    kw = {k.replace("_", ".", 1): v for k, v in kw.items()}
    try:
        for k, v in kw.items():
            gpu.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            gpu.set_tuning(k, KNOB_DEFAULTS[k])


# ---- scenes -------------------------------------------------------------------------------------------------
def _points(counts, n=None):
    pts = scene.parallelogram_centre_points(scene.nightclub_wall_grids(counts))
    return pts if n is None else pts[:n]


def _segment(l, diagonal, i):
    """A segment light from a wall parallelogram's corner along its first edge (or its diagonal), the wall's colour at
    one end and a keyed colour at the other."""
    f32 = np.float32
    p0, e1, e2 = (np.asarray(list(getattr(l, k)), f32) for k in ("p0", "p1", "p2"))
    s = _abi.Light(type=_abi.LIGHT_SEGMENT)
    s.p0[:] = p0.tolist()
    s.p1[:] = ((p0 + e1) + e2 if diagonal else p0 + e1).tolist()
    s.c0[:] = list(l.c0)
    s.c1[:] = scene._keyed_colour(1000 + i)
    return s


def _mixed_lights(n):
    """n lights cycling parallelogram (four keyed corner colours) / point (at the centre) / segment (p0 to p0 + edge01)
    over the 18 wall parallelograms of nightclub_wall_grids((3, 3)), repeated past 18."""
    walls = scene.nightclub_wall_grids((3, 3))
    out = []
    for i in range(n):
        l = walls[i % len(walls)]
        if i % 3 == 0:
            p = copy.copy(l)
            for c, name in enumerate(("c1", "c2", "c3")):
                getattr(p, name)[:] = scene._keyed_colour(2000 + 3 * i + c)
            out.append(p)
        elif i % 3 == 1:
            out.append(scene.parallelogram_centre_points([l])[0])
        else:
            out.append(_segment(l, False, i))
    return out


def _build_scene(name):
    night = get_scene(NIGHT)
    if name == "Monkey":
        return scene.load_prebuilt("Monkey")
    if name == "pt3":
        return scene.Scene(night.meshes, _points((8, 8), 3), name)
    if name == "pt126":
        return scene.Scene(night.meshes, _points((9, 7)), name)
    if name == "pt254":
        return scene.Scene(night.meshes, _points((127, 1)), name)
    if name == "pt255":
        return scene.Scene(night.meshes, _points((128, 1), 255), name)
    if name.startswith("grid"):
        nx, ny = (int(v) for v in name[4:].split("x"))
        return scene.cornell_ceiling_grid((nx, ny))
    if name.startswith("mixed"):
        return scene.Scene(night.meshes, _mixed_lights(int(name[5:])), name)
    if name == "seg5":
        walls = scene.nightclub_wall_grids((3, 3))
        return scene.Scene(night.meshes, [_segment(walls[j], i % 2 == 1, i) for i, j in enumerate((0, 4, 8, 9, 13))], name)
    return get_scene(name)


_built = {}


def shape_scene(name):
    if name not in _built:
        _built[name] = _build_scene(name)
    return _built[name]


def camera(name, cam, w, h):
    """cam: "framed" (cornell_framed_camera), "toml" (cornell_camera), None (the scene's own: the nightclub's for the
    nightclub meshes), or (fov_deg, dist, look_at, rot_deg) for scene.make_camera."""
    if isinstance(cam, tuple):
        return scene.make_camera(*cam, w, h)
    if cam == "framed":
        return scene.cornell_framed_camera(w, h)
    if cam == "toml":
        return scene.cornell_camera(w, h)
    return scene.camera_for(name, w, h) if name in (NIGHT, CORNELL) else scene.nightclub_camera(w, h)


def use_scene(gpu, name):
    """Uploads the scene; returns (scene, restir_scene_info)."""
    s = shape_scene(name)
    gpu.set_scene(s)
    info = gpu.scene_info()
    assert info.num_lights == len(s.lights) and info.num_tris == s.num_triangles
    assert info.bvh_lds_bytes == (2 * info.num_nodes + 3 * info.num_tris) * 16
    return s, info


def assert_over_budget(info):
    assert info.bvh_lds_bytes > LDS_BUDGET, f"the BVH takes {info.bvh_lds_bytes} bytes: it fits LDS"


def assert_point_count(info, L):
    assert info.num_lights == L and info.light_types == 1 and info.light_scale == (L if L & (L - 1) == 0 else 0.0)


# ---- the oracle's side, computed once and shared ------------------------------------------------------------
def feats(N=1, passes=2, unbiased=0, vis=0, temporal=0, **kw):
    return _abi.default_features(num_samples_in_reservoir=N, spatial_resampling_passes=passes,
                                 spatial_reuse=1 if passes else 0, unbiased_combination=unbiased,
                                 spatial_reuse_visibility_check=vis, temporal_reuse=temporal, **kw)


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


_oscenes, _inputs, _ris, _frames = {}, {}, {}, {}


def oscene(oracle, name):
    if name not in _oscenes:
        _oscenes[name] = oracle.OracleScene(shape_scene(name))
    return _oscenes[name]


def inputs(oracle, name, cam, w=W, h=H):
    """(oracle scene, camera, n_t, p_mat) of the oracle's primary rays."""
    k = (name, cam, w, h)
    if k not in _inputs:
        osc, c = oscene(oracle, name), camera(name, cam, w, h)
        _inputs[k] = (osc, c) + frozen(*oracle.gbuffer(osc, c, w, h))
    return _inputs[k]


def ris_of(oracle, name, cam, f, w=W, h=H, frame=0):
    """The oracle's RIS reservoirs (res_a, res_b, res_dbg) over its own G-buffer."""
    k = (name, cam, w, h, bytes(f), frame)
    if k not in _ris:
        osc, c, n_t, p_mat = inputs(oracle, name, cam, w, h)
        _ris[k] = frozen(*oracle_ris(oracle, osc, f, c, n_t, p_mat, frame=frame, w=w, h=h))
    return _ris[k]


def frames_of(oracle, name, cam, f, w=W, h=H, count=1):
    """[(rgb, (res_a, res_b))] of oracle.render_frame for frames 0 .. count - 1; with f.temporal_reuse each frame's
    grid is the next one's predecessor."""
    k = (name, cam, w, h, bytes(f))
    have = _frames.setdefault(k, [])
    osc, c = oscene(oracle, name), camera(name, cam, w, h)
    while len(have) < count:
        prev = have[-1][1] if (have and f.temporal_reuse) else None
        rgb, res, _ = oracle.render_frame(osc, c, f, w, h, SEED, len(have), prev=prev)
        have.append((frozen(rgb)[0], frozen(*res)))
    return have[:count]


def lit_share(oracle, name, cam, N=1, w=W, h=H):
    """The share of pixels with any light in the oracle's two-pass frame."""
    return float((frames_of(oracle, name, cam, feats(N, 2), w, h)[0][0].max(axis=-1) > 0).mean())


def hit_share(oracle, name, cam, w=W, h=H):
    return float((inputs(oracle, name, cam, w, h)[2][:, 3] < 1e30).mean())   # t = FLT_MAX on a miss


# ---- the device's side --------------------------------------------------------------------------------------
def upload_inputs(gpu, oracle, name, cam, N, w=W, h=H):
    osc, c, n_t, p_mat = inputs(oracle, name, cam, w, h)
    gpu.stage_configure(w, h, N)
    gpu.upload(_abi.BUF_GBUF_N_T, n_t)
    gpu.upload(_abi.BUF_GBUF_P_MAT, p_mat)
    return osc, c, n_t, p_mat


def check_reservoirs(gpu, want, what, dbg=True):
    a, b, d = want
    assert_bits(gpu.download(_abi.BUF_RES_A), a, f"{what} res_a")
    assert_bits(gpu.download(_abi.BUF_RES_B), b, f"{what} res_b")
    if dbg:
        assert_bits(gpu.download(_abi.BUF_RES_DBG), d, f"{what} wSum/chosen")


def check_stage_ris(gpu, oracle, name, cam, f, what, w=W, h=H):
    _, c, _, _ = upload_inputs(gpu, oracle, name, cam, f.num_samples_in_reservoir, w, h)
    gpu.stage_ris(c, f, key(_abi.RESTIR_STAGE_RIS))
    check_reservoirs(gpu, ris_of(oracle, name, cam, f, w, h), what)


def check_stage_spatial(gpu, oracle, name, cam, f, what, w=W, h=H, passes=2):
    """`passes` chained stage passes from the oracle's RIS reservoirs, each from the oracle's input."""
    osc, c, n_t, p_mat = upload_inputs(gpu, oracle, name, cam, f.num_samples_in_reservoir, w, h)
    a, b, _ = ris_of(oracle, name, cam, f, w, h)
    for p in range(passes):
        kp = key(_abi.RESTIR_STAGE_SPATIAL, p)
        gpu.upload(_abi.BUF_RES_A, a)
        gpu.upload(_abi.BUF_RES_B, b)
        gpu.stage_spatial(c, f, kp)
        a, b, d = oracle.spatial_pass(osc, f, kp, origin(oracle, c), w, h, n_t, p_mat, (a, b))
        check_reservoirs(gpu, (a, b, d), f"{what} pass {p}")


def check_stage_final(gpu, oracle, name, cam, f, what, w=W, h=H):
    osc, c, n_t, p_mat = upload_inputs(gpu, oracle, name, cam, f.num_samples_in_reservoir, w, h)
    a, b, _ = ris_of(oracle, name, cam, f, w, h)
    gpu.upload(_abi.BUF_RES_A, a)
    gpu.upload(_abi.BUF_RES_B, b)
    gpu.stage_final(c, f)
    assert_bits(gpu.download(_abi.BUF_RGB), oracle.final(osc, f, origin(oracle, c), w, h, n_t, p_mat, (a, b)), f"{what} rgb")


def render(gpu, c, w, h, f, tile=None, want_grid=True, prev=None, frame=0):
    if prev is None:
        gpu.set_seed(SEED, frame)
    return gpu.render_restir(prev, c, w, h, f, tile=tile, want_grid=want_grid)


@contextlib.contextmanager
def counted(gpu):
    """Every kernel of the block bracketed; yields a dict that holds {kernel: launches} after the block."""
    n = {}
    gpu.enable_timing(True)
    try:
        gpu.set_tuning("timing.mask", -1)
        gpu.reset_timings()
        yield n
        n.update({k: v[1] for k, v in gpu.timings().items()})
    finally:
        gpu.enable_timing(False)


def check_frame(gpu, oracle, name, cam, f, what, w=W, h=H):
    """One frame with a returned grid and one without against the oracle's; returns the downloaded grid planes."""
    c = camera(name, cam, w, h)
    want, res = frames_of(oracle, name, cam, f, w, h)[0]
    rgb, grid = render(gpu, c, w, h, f)
    rgb_ng, _ = render(gpu, c, w, h, f, want_grid=False)
    assert_bits(rgb, want, f"{what} rgb")
    assert_grid(grid, res, what)
    assert_bits(rgb_ng, want, f"{what} rgb without a grid")
    same_rgb(rgb_ng, rgb, f"{what} rgb without a grid against the grid frame's")
    return [np.asarray(a) for a in grid.download()]


def check_sequence(gpu, oracle, name, cam, f, what, w=W, h=H, count=4):
    """`count` frames of one view, the grid threaded through when f.temporal_reuse."""
    c = camera(name, cam, w, h)
    want = frames_of(oracle, name, cam, f, w, h, count)
    gpu.set_seed(SEED, 0)
    prev = None
    for frame in range(count):
        rgb, grid = gpu.render_restir(prev if f.temporal_reuse else None, c, w, h, f)
        assert_bits(rgb, want[frame][0], f"{what} frame {frame} rgb")
        assert_grid(grid, want[frame][1], f"{what} frame {frame}")
        prev = grid


def assert_unfused(n, what):
    assert n["primary"] >= 1 and n["ris"] >= 1 and n["primary_ris"] == 0, f"{what}: launches {n}"


# ---- A. a BVH past the LDS budget ---------------------------------------------------------------------------
MONKEY = "Monkey"
# (N, passes, unbiased, visibility reuse)
MONKEY_FRAMES = [(1, 0, 0, 0), (1, 1, 0, 0), (1, 2, 0, 0), (2, 2, 0, 0), (1, 1, 1, 1), (2, 1, 1, 0), (3, 1, 0, 0)]


def test_monkey_views_are_what_the_tests_assume(oracle):
    """From the oracle alone: the framed camera fills the frame with lit geometry, the TOML camera leaves most tiles
    background."""
    assert hit_share(oracle, MONKEY, "framed") >= 0.88 and lit_share(oracle, MONKEY, "framed") >= 0.8
    assert 0.03 <= hit_share(oracle, MONKEY, "toml") <= 0.2
    assert shape_scene(MONKEY).num_triangles == 968 and len(shape_scene(MONKEY).lights) == 2


@pytest.mark.parametrize("cam", ["framed", "toml"])
@pytest.mark.parametrize("w,h", [(W, H), (W2, H2)])
def test_monkey_primary(gpu, oracle, cam, w, h):
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    _, c, n_t, p_mat = inputs(oracle, MONKEY, cam, w, h)
    gpu.stage_configure(w, h, 1)
    gpu.stage_primary(c)
    assert_bits(gpu.download(_abi.BUF_GBUF_N_T), n_t, "n_t")
    assert_bits(gpu.download(_abi.BUF_GBUF_P_MAT), p_mat, "p_mat")


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("initial_vis", [0, 1])
def test_monkey_ris(gpu, oracle, N, initial_vis):
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    f = feats(N, initial_samples_visibility_check=initial_vis)
    for cam in ("framed", "toml"):
        check_stage_ris(gpu, oracle, MONKEY, cam, f, f"N={N} vis={initial_vis} {cam}")


@pytest.mark.parametrize("N", [1, 2])
def test_monkey_temporal(gpu, oracle, N):
    """k_temporal over the oracle's inputs: the predecessor is frame 0 after one spatial pass, the current grid frame 1's RIS."""
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    f = feats(N, temporal=1)
    osc, c, n_t, p_mat = upload_inputs(gpu, oracle, MONKEY, "framed", N)
    a0, b0, _ = ris_of(oracle, MONKEY, "framed", f)
    pa, pb, _ = oracle.spatial_pass(osc, f, key(_abi.RESTIR_STAGE_SPATIAL, 0, 0), origin(oracle, c), W, H, n_t, p_mat, (a0, b0))
    ca, cb, _ = ris_of(oracle, MONKEY, "framed", f, frame=1)
    for which, arr in [(_abi.BUF_RES_A, ca), (_abi.BUF_RES_B, cb), (_abi.BUF_PREV_A, pa), (_abi.BUF_PREV_B, pb)]:
        gpu.upload(which, arr)
    kt = key(_abi.RESTIR_STAGE_TEMPORAL, 0, 1)
    gpu.stage_temporal(c, f, kt)
    check_reservoirs(gpu, oracle.temporal(osc, f, kt, origin(oracle, c), W, H, n_t, p_mat, (ca, cb), (pa, pb)), f"N={N}")


# k_spatial1_ntl[_t2], k_spatial2_ntl, k_spatial1u, the general unbiased kernel with rays over the global BVH (the lean
# k_spatial1u_vis needs the BVH in LDS), the general kernels at N = 3
MONKEY_SPATIAL = {"biased_n1": (1, 0, 0, {}), "biased_n1_t2": (1, 0, 0, dict(spatial_th=2)), "biased_n2": (2, 0, 0, {}),
                  "unbiased_n1": (1, 1, 0, {}), "unbiased_vis_n1": (1, 1, 1, {}), "general_n3": (3, 0, 0, {}),
                  "general_n3_unbiased_vis": (3, 1, 1, {})}


@pytest.mark.parametrize("case", sorted(MONKEY_SPATIAL))
def test_monkey_spatial(gpu, oracle, case):
    N, unbiased, vis, tune = MONKEY_SPATIAL[case]
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    with knobs(gpu, **tune):
        check_stage_spatial(gpu, oracle, MONKEY, "framed", feats(N, 2, unbiased, vis), case)
        if tune:
            check_stage_spatial(gpu, oracle, MONKEY, "framed", feats(N, 2, unbiased, vis), case, W2, H2)


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("tonemap", [1, 0])
def test_monkey_final(gpu, oracle, N, tonemap):
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    f = feats(N, enable_tone_mapping=tonemap, gamma=2.2)
    for cam in ("framed", "toml"):
        check_stage_final(gpu, oracle, MONKEY, cam, f, f"N={N} tonemap={tonemap} {cam}")


# every row through the framed view; the background-tile view through the routes that treat background tiles apart
@pytest.mark.parametrize("cam,N,passes,unbiased,vis", [("framed",) + r for r in MONKEY_FRAMES] +
                         [("toml",) + r for r in MONKEY_FRAMES if r in ((1, 2, 0, 0), (2, 2, 0, 0), (1, 1, 1, 1))])
def test_monkey_frames(gpu, oracle, cam, N, passes, unbiased, vis):
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    what = f"{cam} N={N} passes={passes} unbiased={unbiased} vis={vis}"
    with counted(gpu) as n:
        check_frame(gpu, oracle, MONKEY, cam, feats(N, passes, unbiased, vis), what)
    assert_unfused(n, what)
    assert n["spatial"] == 2 * passes and n["final"] == 2 and n["temporal"] == 0, f"{what}: launches {n}"
    assert gpu.background_pixels()[0] == 0   # no tile flags without the fused kernel


def test_monkey_static_view_sequence(gpu, oracle):
    """Four frames of one view: nothing is kept between them (the G-buffer reuse belongs to the fused kernel)."""
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    before = gpu.gbuf_reuses()
    with counted(gpu) as n:
        check_sequence(gpu, oracle, MONKEY, "framed", feats(1, 2), "static")
    assert_unfused(n, "static")
    assert n["primary"] == 4 and n["ris"] == 4
    assert gpu.gbuf_reuses() == before, "a frame read a kept G-buffer"


@pytest.mark.parametrize("N", [1, 2])
def test_monkey_temporal_sequence(gpu, oracle, N):
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    with counted(gpu) as n:
        check_sequence(gpu, oracle, MONKEY, "framed", feats(N, 2, temporal=1), f"temporal N={N}")
    assert_unfused(n, f"temporal N={N}")
    assert n["temporal"] == 3, f"launches {n}"


def test_monkey_ghost_zoned_tile(gpu, oracle):
    from romis_amd import restir
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    N, passes = 1, 2
    f = feats(N, passes)
    tile = restir.tile_plan(W, H, 2, 1, 1, passes * f.spatial_resample_radius)
    assert tile.gwidth - tile.width == passes * f.spatial_resample_radius
    want, (wa, wb) = frames_of(oracle, MONKEY, "framed", f)[0]
    with counted(gpu) as n:
        rgb, grid = render(gpu, camera(MONKEY, "framed", W, H), W, H, f, tile=tile)
    assert_unfused(n, "tile")
    r0 = H - (tile.y0 + tile.height)
    assert_bits(rgb, np.ascontiguousarray(want[r0:r0 + tile.height, tile.x0:tile.x0 + tile.width]), "tile rgb")
    pos, col, gw, gm = grid.download()
    own = (slice(None), slice(tile.y0 - tile.gy0, tile.y0 - tile.gy0 + tile.height),
           slice(tile.x0 - tile.gx0, tile.x0 - tile.gx0 + tile.width))
    ref = (slice(None), slice(tile.y0, tile.y0 + tile.height), slice(tile.x0, tile.x0 + tile.width))
    wa, wb = wa.reshape(N, H, W, 4)[ref], wb.reshape(N, H, W, 4)[ref]
    assert_bits(pos[own], wa[..., :3], "tile grid position")
    assert_bits(gw[own], wa[..., 3], "tile grid W")
    assert_bits(col[own], wb[..., :3], "tile grid colour")
    assert np.array_equal(gm[own], np.ascontiguousarray(wb[..., 3]).view(np.uint32)), "tile grid M"


def assert_image_carries_light(rgb, case):
    """R-MIS images are finite.  After two iterations R-OMIS's least-squares system is singular at a pixel or two, in
    the oracle as on the device (the existing nightclub scene has one such pixel as well): the words are compared with
    the oracle's all the same, and the rest of the image must be finite."""
    finite = np.isfinite(rgb)
    assert finite.all() if case.startswith("rmis") else finite.mean() >= 0.995, f"{case}: {(~finite).sum()} words not finite"
    assert rgb[finite].max() > 0.0


@pytest.mark.parametrize("case", ["rmis_equal", "romis_direct"])
def test_monkey_render_mis(gpu, oracle, case):
    from test_gpu_mis import MIS_CASES, bits_equal
    assert_over_budget(use_scene(gpu, MONKEY)[1])
    f = _abi.default_features(**MIS_CASES[case])
    f.max_iterations_mis = 2
    c = camera(MONKEY, "framed", W, H)
    gpu.set_seed(SEED, 0)
    got = gpu.render_mis(c, W, H, f)
    bits_equal(got, oracle.render_mis(oscene(oracle, MONKEY), c, f, W, H, SEED, 0), f"Monkey {case}")
    assert_image_carries_light(got, case)


# The smallest bvh.max_leaf at which Monkey's BVH fits LDS (63,904 bytes).  The test below searches for it
# and fails if it moves.
MONKEY_FIT_LEAF = 5


def test_monkey_with_a_larger_leaf_fits_lds(gpu, oracle):
    """A larger leaf shrinks the node array until the BVH fits: the frame takes k_primary_ris with 62 KB of BVH beside
    the light table, the tile flags and the fused last pass's ray phase.  The oracle does not depend on the leaf size."""
    try:
        fit = None
        for leaf in range(2, 17):
            gpu.set_tuning("bvh.max_leaf", leaf)
            _, info = use_scene(gpu, MONKEY)
            if info.bvh_lds_bytes <= LDS_BUDGET:
                fit = leaf
                break
        assert fit == MONKEY_FIT_LEAF, f"Monkey fits LDS from bvh.max_leaf = {fit} ({info.bvh_lds_bytes} bytes)"
        for cam in ("framed", "toml"):
            for N, passes, unbiased, vis in [(1, 2, 0, 0), (2, 2, 0, 0), (1, 1, 1, 1)]:
                what = f"leaf {fit} {cam} N={N} passes={passes} unbiased={unbiased}"
                with counted(gpu) as n:
                    check_frame(gpu, oracle, MONKEY, cam, feats(N, passes, unbiased, vis), what)
                assert n["primary_ris"] == 2 and n["primary"] == 0 and n["ris"] == 0, f"{what}: launches {n}"
        check_sequence(gpu, oracle, MONKEY, "framed", feats(1, 2, temporal=1), f"leaf {fit} temporal")
    finally:
        gpu.set_tuning("bvh.max_leaf", KNOB_DEFAULTS["bvh.max_leaf"])
        gpu.set_scene(shape_scene(MONKEY))
    assert_over_budget(gpu.scene_info())


UNFUSED_KNOBS = {"primary_lds": dict(primary_lds=0), "final_lds": dict(final_lds=0), "unfused": dict(fuse_primary_ris=0),
                 "all": dict(primary_lds=0, final_lds=0, fuse_primary_ris=0)}


@pytest.mark.parametrize("tune", sorted(UNFUSED_KNOBS))
@pytest.mark.parametrize("name,cam", [(NIGHT, None), (CORNELL, "framed"), (CORNELL, None)])
def test_small_scenes_through_the_unstaged_kernels(gpu, oracle, name, cam, tune):
    """The kernels of an over-budget BVH forced on scenes whose BVH fits: N = 1 and 2, two passes, the default frame
    first so that the knobbed frame's grid can be compared with it too."""
    _, info = use_scene(gpu, name)
    assert info.bvh_lds_bytes <= LDS_BUDGET
    for N in (1, 2):
        f = feats(N, 2)
        ref = check_frame(gpu, oracle, name, cam, f, f"{name} N={N} defaults")
        with knobs(gpu, **UNFUSED_KNOBS[tune]):
            with counted(gpu) as n:
                got = check_frame(gpu, oracle, name, cam, f, f"{name} N={N} {tune}")
        same_grid(got, ref, f"{name} N={N} {tune} against the default frame")
        if "fuse_primary_ris" in UNFUSED_KNOBS[tune]:
            assert_unfused(n, f"{name} {tune}")
        else:
            assert n["primary_ris"] == 2 and n["primary"] == 0, f"{name} {tune}: launches {n}"
    with knobs(gpu, **UNFUSED_KNOBS[tune]):
        check_sequence(gpu, oracle, name, cam, feats(1, 2, temporal=1), f"{name} {tune} temporal", count=2)


# ---- B. point-light counts that are no power of two ---------------------------------------------------------
POINT_SETS = {"pt3": 3, "pt126": 126, "pt254": 254, "pt255": 255}


def held_index(res, lights):
    """Per pixel of sub-reservoir 0 the index of the light whose position the held sample has (bit for bit); L for the
    zero sample (position and colour 0), -1 for anything else."""
    a, b = res
    pos = np.ascontiguousarray(a[0, :, :3]).view(np.uint32)
    table = np.array([list(l.p0) for l in lights], np.float32).view(np.uint32)
    idx = np.full(pos.shape[0], -1, np.int64)
    for i in range(len(lights) - 1, -1, -1):
        idx[(pos == table[i]).all(axis=1)] = i
    zero = (a[0, :, :3] == 0).all(axis=1) & (b[0, :, :3] == 0).all(axis=1) & (idx < 0)
    idx[zero] = len(lights)
    return idx


@pytest.mark.parametrize("name", sorted(POINT_SETS))
def test_point_sets_hold_their_highest_indices(oracle, name):
    """From the oracle alone: after RIS and after two passes (N = 1) pixels hold the light of index L - 1, the zero
    sample, and (L >= 254) lights whose index needs the handle's top bits."""
    L = POINT_SETS[name]
    lights = shape_scene(name).lights
    assert len(lights) == L and len({tuple(l.p0) for l in lights}) == L
    f = feats(1, 2)
    for what, res in [("RIS", ris_of(oracle, name, None, f)[:2]), ("two passes", frames_of(oracle, name, None, f)[0][1])]:
        idx = held_index(res, lights)
        assert (idx >= 0).all(), f"{what}: a held position is no light's"
        assert (idx == L).sum() >= 100, f"{what}: {(idx == L).sum()} pixels hold the zero sample"
        assert (idx == L - 1).sum() >= 1, f"{what}: no pixel holds light {L - 1}"
        if L >= 254:
            high = ((idx >= 250) & (idx < L)).sum()
            assert high >= 5, f"{what}: {high} pixels hold a light of index >= 250"


@pytest.mark.parametrize("name", sorted(POINT_SETS))
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("lds", [0, 1])
def test_point_sets_ris(gpu, oracle, name, compact, lds):
    assert_point_count(use_scene(gpu, name)[1], POINT_SETS[name])
    with knobs(gpu, ris_compact=compact, ris_lds=lds):
        for N in (1, 2, 3):
            check_stage_ris(gpu, oracle, name, None, feats(N), f"{name} N={N} compact={compact} lds={lds}")
        check_stage_ris(gpu, oracle, name, None, feats(1, initial_samples_visibility_check=1), f"{name} vis compact={compact}")


# the handle routes of test_gpu_spatial_sweep.FRAME_ROUTES, and the default route with and without the fused final
POINT_ROUTES = {"hg_t2": (1, {}), "hg_t2_unfused_final": (1, dict(final_fuse=0)),
                "h_t2": (1, dict(spatial_gather=0, spatial_th=2)), "h": (1, dict(spatial_th=1)),
                "nohandles": (1, dict(spatial_handles=0)), "n2_th1": (2, dict(spatial_th=1)),
                "n2_th2": (2, dict(spatial_th=2))}


@pytest.mark.parametrize("name", sorted(POINT_SETS))
@pytest.mark.parametrize("route", sorted(POINT_ROUTES))
def test_point_sets_handle_routes(gpu, oracle, name, route):
    """Two-pass frames through each handle route.  Up to L = 254 the default N = 1 route fuses final shading into the
    last handle pass (no RESTIR_K_FINAL launch); at L = 255 the index field is full and the reservoir planes are read."""
    L = POINT_SETS[name]
    assert_point_count(use_scene(gpu, name)[1], L)
    N, tune = POINT_ROUTES[route]
    with knobs(gpu, **tune):
        with counted(gpu) as n:
            check_frame(gpu, oracle, name, None, feats(N, 2), f"{name} {route}")
        if N == 2:
            with knobs(gpu, spatial_n2h=0):
                check_frame(gpu, oracle, name, None, feats(N, 2), f"{name} {route} spatial.n2h=0")
    assert n["spatial"] == 4 and n["primary_ris"] == 2
    if route == "hg_t2":
        assert n["final"] == (0 if L <= 254 else 2), f"{name}: {n['final']} final launches"
    if route == "hg_t2_unfused_final":
        assert n["final"] == 2


@pytest.mark.parametrize("name", sorted(POINT_SETS))
@pytest.mark.parametrize("N", [1, 2])
def test_point_sets_temporal_sequence(gpu, oracle, name, N):
    """Four frames threading the grid: the fused temporal kernel rebuilds the predecessor from the frame handles
    (hv >> 24 up to L = 254)."""
    assert_point_count(use_scene(gpu, name)[1], POINT_SETS[name])
    check_sequence(gpu, oracle, name, None, feats(N, 2, temporal=1), f"{name} temporal N={N}")


def test_point_set_render_mis(gpu, oracle):
    """mis.hip divides by 1 / L on its own."""
    from test_gpu_mis import MIS_CASES, bits_equal
    assert_point_count(use_scene(gpu, "pt126")[1], 126)
    c = camera("pt126", None, W, H)
    for case in ("rmis_balance", "romis_direct"):
        f = _abi.default_features(**MIS_CASES[case])
        f.max_iterations_mis = 2
        gpu.set_seed(SEED, 0)
        got = gpu.render_mis(c, W, H, f)
        bits_equal(got, oracle.render_mis(oscene(oracle, "pt126"), c, f, W, H, SEED, 0), f"pt126 {case}")
        assert_image_carries_light(got, case)


# ---- C. light grids that are not square ---------------------------------------------------------------------
# name: (L, lights_regular, grid_ny_log2)
GRIDS = {"grid3x4": (12, 1, 2), "grid24x32": (768, 1, 5), "grid31x32": (992, 1, 5), "grid5x3": (15, 0, 0)}


def assert_grid_form(info, name):
    L, regular, ny_log2 = GRIDS[name]
    assert (info.num_lights, info.light_types, info.lights_pgram, info.lights_grid) == (L, 4, 1, 1)
    assert (info.lights_regular, info.grid_ny_log2) == (regular, ny_log2), \
        f"{name}: regular {info.lights_regular}, ny_log2 {info.grid_ny_log2}"
    assert info.light_scale == 0.0


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_light_grids_light_the_frame(oracle, name):
    assert hit_share(oracle, name, "framed") >= 0.95
    assert 0.88 <= lit_share(oracle, name, "framed") <= 0.94


@pytest.mark.parametrize("name", sorted(GRIDS))
@pytest.mark.parametrize("compact", [0, 1, 2])
def test_light_grids_ris(gpu, oracle, name, compact):
    assert_grid_form(use_scene(gpu, name)[1], name)
    for lds in (1, 0):
        with knobs(gpu, ris_compact=compact, ris_lds=lds):
            for N in (1, 2):
                check_stage_ris(gpu, oracle, name, "framed", feats(N), f"{name} N={N} compact={compact} lds={lds}")


@pytest.mark.parametrize("name", sorted(GRIDS))
@pytest.mark.parametrize("N,th", [(1, 0), (1, 1), (2, 0)])
def test_light_grids_frames(gpu, oracle, name, N, th):
    """Two passes: the regular grids' N = 1 frames read grid handles (k_spatial1g_t2; spatial.th = 1: the n_t-window pass)."""
    assert_grid_form(use_scene(gpu, name)[1], name)
    with knobs(gpu, spatial_th=th):
        check_frame(gpu, oracle, name, "framed", feats(N, 2), f"{name} N={N} th={th}")
        check_frame(gpu, oracle, name, "framed", feats(N, 2), f"{name} N={N} th={th} {W2}x{H2}", W2, H2)


# ---- D. mixed and multi-light sets --------------------------------------------------------------------------
MIXED_SETS = {"mixed17": (17, 7), "seg5": (5, 2)}


def assert_light_types(info, name):
    L, types = MIXED_SETS[name]
    assert (info.num_lights, info.light_types) == (L, types)
    assert (info.lights_pgram, info.lights_grid, info.lights_regular, info.light_scale) == (0, 0, 0, 0.0)


def test_mixed_set_cycles_the_types_and_lights_the_frame(oracle):
    assert [l.type for l in shape_scene("mixed17").lights][:6] == [2, 0, 1, 2, 0, 1]
    seg = [l for l in shape_scene("mixed17").lights if l.type == _abi.LIGHT_SEGMENT]
    assert all(list(l.c0) != list(l.c1) and list(l.p0) != list(l.p1) for l in seg)
    for N in (1, 2, 3):
        assert 0.58 <= lit_share(oracle, "mixed17", None, N) <= 0.72
    assert lit_share(oracle, "seg5", None) >= 0.55


@pytest.mark.parametrize("name", sorted(MIXED_SETS))
@pytest.mark.parametrize("lds", [0, 1])
def test_mixed_sets_ris(gpu, oracle, name, lds):
    assert_light_types(use_scene(gpu, name)[1], name)
    with knobs(gpu, ris_lds=lds):
        for N in (1, 2, 3):
            check_stage_ris(gpu, oracle, name, None, feats(N), f"{name} N={N} lds={lds}")
        check_stage_ris(gpu, oracle, name, None, feats(2, initial_samples_visibility_check=1), f"{name} vis lds={lds}")


@pytest.mark.parametrize("name", sorted(MIXED_SETS))
@pytest.mark.parametrize("N,unbiased,vis", [(1, 0, 0), (2, 0, 0), (1, 1, 0), (1, 1, 1), (3, 1, 0)])
def test_mixed_sets_spatial(gpu, oracle, name, N, unbiased, vis):
    assert_light_types(use_scene(gpu, name)[1], name)
    check_stage_spatial(gpu, oracle, name, None, feats(N, 2, unbiased, vis), f"{name} N={N} unbiased={unbiased} vis={vis}")


@pytest.mark.parametrize("name", sorted(MIXED_SETS))
def test_mixed_sets_final_and_frame(gpu, oracle, name):
    assert_light_types(use_scene(gpu, name)[1], name)
    for N in (1, 2):
        check_stage_final(gpu, oracle, name, None, feats(N), f"{name} N={N}")
        check_frame(gpu, oracle, name, None, feats(N, 2), f"{name} N={N} frame")
    check_sequence(gpu, oracle, name, None, feats(1, 2, temporal=1), f"{name} temporal", count=2)


@pytest.mark.parametrize("L,staged", [(585, True), (586, False)])
def test_general_light_table_staging_boundary(gpu, oracle, L, staged):
    """The 7-float4 records of L lights take 112 L bytes: 65,520 at L = 585 (staged in LDS), 65,632 at 586 (global memory)."""
    name = f"mixed{L}"
    _, info = use_scene(gpu, name)
    assert (info.num_lights, info.light_types, info.light_scale) == (L, 7, 0.0)
    assert (112 * L <= LDS_BUDGET) == staged
    for N in (1, 3):
        check_stage_ris(gpu, oracle, name, None, feats(N), f"{name} N={N}")
