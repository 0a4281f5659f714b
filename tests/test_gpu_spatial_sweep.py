"""numNeighboursToSample (K) and spatialResampleRadius (R) swept through every spatial-reuse kernel.

The lean kernels of kernels.hip unroll their neighbour loops to kLeanK = 5 masked by n < K, and size their LDS window
(32 + 2R) x (8 TH + 2R), its row width AW and the reciprocal behind LeanWindow::row() from R.  The host takes them for
K <= 5 and R <= 10 and the general kernels one step outside.  Here K and R run over the interior of that domain, its
edges (K = 0, R = 0, K = 5, R = 10) and the first values outside (K = 6, R = 11), through each kernel in turn.  The
bar is the project's: every word of res_a, res_b, (res_dbg), RGB and the returned grid equals the oracle's
(oracle.spatial_pass on the oracle's own inputs for the stage routes, oracle.render_frame for whole frames).  No
tolerance is involved.

Sizes: 65 x 35 has three tile columns, the last one pixel wide, so AW takes 1 + R, 32 + R and 32 + 2R across them
(AW = 1 at R = 0, where row() once returned 0 for every entry), and a ragged bottom tile row (3 rows) at both tile
heights; 97 x 41 of the nightclub and 65 x 35 of cornell_1024's default camera have all-background, mixed and
all-geometry tiles.

Routes, by the condition of route_spatial / spatial_handle_kind (csrc/route.h) that selects the kernel (lean: spatial.lean, N = 1,
K <= 5, SoA planes; lean2: the same at N = 2; hin: the pass reads handles, spatial_handle_kind >= 0):

stage API (no handles, no background flags; debug on: the _dbg instantiation, off: the shipped one)
  ntl          lean, biased, R <= 10, th = 1 (spatial.th = 1)                      k_spatial1_ntl
  ntl_t2       lean, biased, R <= 10, th >= 2 (spatial.th = 2)                     k_spatial1_ntl_t2
  n2_ntl       lean2, biased, R <= 10, no hin                                      k_spatial2_ntl
  u            lean, unbiased, no visibility reuse (any R)                         k_spatial1u
  u_vis        lean, unbiased, visibility reuse, the BVH fits LDS (any R)          k_spatial1u_vis
  general_*    N = 3: neither lean nor lean2                                       k_spatial_n0_biased / _unbiased
  K = 6, or R = 11 on a biased route: the general k_spatial_n1 / n2 kernels

whole frames (restir_render, two passes: the first writes handles only)
  hg_t2        hin kind 0 (point lights, N = 1), spatial.gather, spatial.th != 1   k_spatial1hg_t2, and the last pass
               with final.fuse               k_spatial1hg_t2_final (no RESTIR_K_FINAL launch; one for K = 6 or R = 11)
  h_t2         hin kind 0, spatial.gather = 0, spatial.th = 2                      k_spatial1h_t2
  h            hin kind 0, spatial.th = 1                                          k_spatial1h
  nohandles    spatial.handles = 0: no hin, th by width = 1, RIS's pdf cache       k_spatial1_ntl (not _dbg)
  g_t2         hin kind 1 (cornell_1024, a regular light grid, <= 1024 lights)     k_spatial1g_t2
  n2_th1/2     hin kind 2 (point lights, N = 2, spatial.n2h), spatial.th           k_spatial2hg / k_spatial2hg_t2
               and spatial.n2h = 0: no hin                                         k_spatial2_ntl
  spatial_handle_kind's M bound (M0 (K + 1)^passes <= kHandleM = 2^24 - 1, kHandleMG = 2^19 - 1) at its last value
  inside and first outside, reached exactly at R = 0 where every neighbour is the pixel itself.

Every knob is restored in a finally clause.  The oracle's inputs and frames are computed once per (scene, size, features),
shared between the routes and never written to.
"""
import contextlib

import numpy as np
import pytest

from romis_amd import _abi, scene
from test_gpu_parity import SEED, assert_bits, assert_grid, get_scene, key, oracle_ris, origin

pytestmark = pytest.mark.gpu

NIGHT, CORNELL = "nightclub_128pt", "cornell_1024"
W, H = 65, 35

R_SWEEP = [(5, r) for r in (0, 1, 2, 3, 4, 6, 8, 9, 10, 11)]
K_SWEEP = [(k, 10) for k in (0, 1, 2, 3, 4, 6)]
MIXED = [(0, 0), (1, 0), (3, 4), (2, 7), (4, 5), (6, 11)]
PAIRS = R_SWEEP + K_SWEEP + MIXED
GENERAL_PAIRS = [(5, 0), (3, 4), (6, 11)]
BACKGROUND_PAIRS = [(5, 0), (2, 7), (5, 10), (6, 10), (5, 11)]
GHOST_PAIRS = [(5, 0), (3, 4), (5, 7)]

KNOB_DEFAULTS = {"spatial.th": 0, "spatial.gather": 1, "spatial.handles": 1, "spatial.n2h": 1, "final.fuse": 1,
                 "miss.tiles": 1, "miss.gbuf": 2}


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


def feats(K, R, N=1, passes=2, M=32, mode="biased"):
    return _abi.default_features(num_samples_in_reservoir=N, num_neighbours_to_sample=K, spatial_resample_radius=R,
                                 spatial_resampling_passes=passes, initial_light_samples=M, temporal_reuse=0,
                                 unbiased_combination=int(mode != "biased"),
                                 spatial_reuse_visibility_check=int(mode == "unbiased_vis"))


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


# ---- the oracle's side, computed once and shared ------------------------------------------------------------
_inputs, _chains, _frames = {}, {}, {}


def inputs(oracle, name, framing, w, h):
    """(scene, oracle scene, camera, n_t, p_mat, hit mask) of the oracle's primary rays."""
    k = (name, framing, w, h)
    if k not in _inputs:
        s = get_scene(name)
        osc = oracle.OracleScene(s)
        cam = scene.camera_for(name, w, h, framing)
        n_t, p_mat = frozen(*oracle.gbuffer(osc, cam, w, h))
        _inputs[k] = (s, osc, cam, n_t, p_mat, n_t[:, 3] < 1e30)   # t = FLT_MAX on a miss
    return _inputs[k]


def chain(oracle, name, framing, w, h, N, mode, K, R, passes=2):
    """The oracle's RIS reservoirs and `passes` chained spatial passes over them: [(a, b, dbg)], entry 0 = RIS."""
    k = (name, framing, w, h, N, mode, K, R, passes)
    if k not in _chains:
        _, osc, cam, n_t, p_mat, _ = inputs(oracle, name, framing, w, h)
        f = feats(K, R, N, passes, mode=mode)
        out = [frozen(*oracle_ris(oracle, osc, f, cam, n_t, p_mat, w=w, h=h))]
        for p in range(passes):
            out.append(frozen(*oracle.spatial_pass(osc, f, key(_abi.RESTIR_STAGE_SPATIAL, p), origin(oracle, cam), w, h,
                                                   n_t, p_mat, out[-1][:2])))
        _chains[k] = out
    return _chains[k]


def oracle_frame(oracle, name, framing, w, h, K, R, N=1, passes=2, M=32):
    """(rgb, (res_a, res_b)) of oracle.render_frame, biased passes."""
    k = (name, framing, w, h, K, R, N, passes, M)
    if k not in _frames:
        _, osc, cam, _, _, _ = inputs(oracle, name, framing, w, h)
        rgb, res, _ = oracle.render_frame(osc, cam, feats(K, R, N, passes, M), w, h, SEED, 0)
        _frames[k] = (frozen(rgb)[0], frozen(*res))
    return _frames[k]


def M_of(b):
    return b[..., 3].view(np.uint32)


def assert_not_vacuous(oracle, name, framing, w, h, N, mode, K, R, min_share):
    """From the oracle alone: the camera sees geometry, and (K >= 1) the first pass grows M on >= 10 % of it -- the
    smallest share over every route and pair here is 24 % (K = 1, R = 10, N = 2)."""
    hit = inputs(oracle, name, framing, w, h)[5]
    assert hit.mean() >= min_share, f"geometry share {hit.mean():.3f}"
    if K >= 1:
        c = chain(oracle, name, framing, w, h, N, mode, K, R)
        grew = (M_of(c[1][1]) > M_of(c[0][1])).any(axis=0)
        assert grew[hit].mean() >= 0.1, f"M grows on {grew[hit].mean():.3f} of the geometry pixels"


def tile_census(hit, w, h, tw=32, th=8):
    """(all-background, mixed, all-geometry) tw x th tiles of the frame."""
    m = hit.reshape(h, w)
    n = [0, 0, 0]
    for y in range(0, h, th):
        for x in range(0, w, tw):
            t = m[y:y + th, x:x + tw]
            n[0 if not t.any() else (2 if t.all() else 1)] += 1
    return tuple(n)


# ---- stage API ----------------------------------------------------------------------------------------------
STAGE_ROUTES = {"ntl": (1, "biased", dict(spatial_th=1)), "ntl_t2": (1, "biased", dict(spatial_th=2)),
                "n2_ntl": (2, "biased", {}), "u": (1, "unbiased", {}), "u_vis": (1, "unbiased_vis", {}),
                "general_biased": (3, "biased", {}), "general_unbiased": (3, "unbiased", {})}
STAGE_CASES = [(r, k, rad) for r in STAGE_ROUTES for k, rad in (GENERAL_PAIRS if r.startswith("general") else PAIRS)]


def run_stage_chain(gpu, oracle, name, w, h, N, mode, K, R):
    """Two chained passes, each from the oracle's input reservoirs, with the debug plane (res_a, res_b, res_dbg) and
    without (res_a, res_b).  The second run's output slot holds the pass's input before it, not the first run's output."""
    s, _, cam, n_t, p_mat, _ = inputs(oracle, name, None, w, h)
    c = chain(oracle, name, None, w, h, N, mode, K, R)
    f = feats(K, R, N, mode=mode)
    gpu.set_scene(s)
    gpu.stage_configure(w, h, N)
    gpu.upload(_abi.BUF_GBUF_N_T, n_t)
    gpu.upload(_abi.BUF_GBUF_P_MAT, p_mat)
    for p in range(2):
        (a, b, _), (a2, b2, d2) = c[p], c[p + 1]
        for debug in (True, False):
            gpu.upload(_abi.BUF_RES_A, a)
            gpu.upload(_abi.BUF_RES_B, b)
            gpu.stage_spatial(cam, f, key(_abi.RESTIR_STAGE_SPATIAL, p), debug=debug)
            what = f"K={K} R={R} pass {p} debug={debug}"
            assert_bits(gpu.download(_abi.BUF_RES_A), a2, f"{what} res_a")
            assert_bits(gpu.download(_abi.BUF_RES_B), b2, f"{what} res_b")
            if debug:
                assert_bits(gpu.download(_abi.BUF_RES_DBG), d2, f"{what} wSum/chosen")


@pytest.mark.parametrize("route,K,R", STAGE_CASES)
def test_stage_pass_sweep(gpu, oracle, route, K, R):
    N, mode, tune = STAGE_ROUTES[route]
    assert_not_vacuous(oracle, NIGHT, None, W, H, N, mode, K, R, 0.5)
    with knobs(gpu, **tune):
        run_stage_chain(gpu, oracle, NIGHT, W, H, N, mode, K, R)


# ---- whole frames -------------------------------------------------------------------------------------------
def render(gpu, cam, w, h, f, tile=None, want_grid=True):
    gpu.set_seed(SEED, 0)
    return gpu.render_restir(None, cam, w, h, f, tile=tile, want_grid=want_grid)


def render_counted(gpu, cam, w, h, f):
    """(rgb, grid, RESTIR_K_FINAL launches, RESTIR_K_SPATIAL launches) of one frame with every kernel bracketed."""
    gpu.enable_timing(True)
    try:
        gpu.set_tuning("timing.mask", -1)
        gpu.reset_timings()
        rgb, grid = render(gpu, cam, w, h, f)
        t = gpu.timings()
    finally:
        gpu.enable_timing(False)
    return rgb, grid, t["final"][1], t["spatial"][1]


def in_domain(K, R):
    return K <= 5 and R <= 10


# route: (scene, framing, N, knobs)
FRAME_ROUTES = {"h_t2": (NIGHT, None, 1, dict(spatial_gather=0, spatial_th=2)),
                "h": (NIGHT, None, 1, dict(spatial_th=1)),
                "nohandles": (NIGHT, None, 1, dict(spatial_handles=0)),
                "g_t2": (CORNELL, "framed", 1, {}),
                "n2_th1": (NIGHT, None, 2, dict(spatial_th=1)),
                "n2_th2": (NIGHT, None, 2, dict(spatial_th=2))}


@pytest.mark.parametrize("K,R", PAIRS)
def test_frame_sweep_gathered_handles_fused_and_not(gpu, oracle, K, R):
    """The default N = 1 route, k_spatial1hg_t2 twice (final.fuse = 0) and k_spatial1hg_t2 + k_spatial1hg_t2_final.  The
    fused kernel replaces final shading's launch exactly inside the handle path's documented limits."""
    assert_not_vacuous(oracle, NIGHT, None, W, H, 1, "biased", K, R, 0.5)
    s, _, cam, _, _, _ = inputs(oracle, NIGHT, None, W, H)
    want, res = oracle_frame(oracle, NIGHT, None, W, H, K, R)
    gpu.set_scene(s)
    f = feats(K, R)
    for fuse in (1, 0):
        with knobs(gpu, final_fuse=fuse):
            rgb, grid, n_final, n_spatial = render_counted(gpu, cam, W, H, f)
        what = f"K={K} R={R} final.fuse={fuse}"
        assert_bits(rgb, want, f"{what} rgb")
        assert_grid(grid, res, what)
        assert n_spatial == 2, f"{what}: {n_spatial} spatial launches"
        assert n_final == (0 if fuse and in_domain(K, R) else 1), f"{what}: {n_final} final launches"


@pytest.mark.parametrize("route,K,R", [(r, k, rad) for r in FRAME_ROUTES for k, rad in PAIRS])
def test_frame_sweep(gpu, oracle, route, K, R):
    name, framing, N, tune = FRAME_ROUTES[route]
    assert_not_vacuous(oracle, name, framing, W, H, N, "biased", K, R, 0.9 if framing else 0.5)
    s, _, cam, _, _, _ = inputs(oracle, name, framing, W, H)
    want, res = oracle_frame(oracle, name, framing, W, H, K, R, N)
    gpu.set_scene(s)
    f = feats(K, R, N)
    with knobs(gpu, **tune):
        rgb, grid = render(gpu, cam, W, H, f)
        if N == 2:
            with knobs(gpu, spatial_n2h=0):   # the reservoir form, k_spatial2_ntl, against the same oracle frame
                rgb_off, grid_off = render(gpu, cam, W, H, f)
    what = f"{route} K={K} R={R}"
    assert_bits(rgb, want, f"{what} rgb")
    assert_grid(grid, res, what)
    if N == 2:
        assert_bits(rgb_off, want, f"{what} spatial.n2h=0 rgb")
        assert_grid(grid_off, res, f"{what} spatial.n2h=0")


# ---- background tiles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,R", BACKGROUND_PAIRS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("name,w,h", [(NIGHT, 97, 41), (CORNELL, 65, 35)])
def test_background_tiles_sweep(gpu, oracle, name, w, h, N, K, R):
    """Frames with all-background, mixed and all-geometry tiles, the flags (miss.tiles) on and off, RIS's G-buffer skip
    forced (miss.gbuf = 1: the window fix-up of lean_window_ready, whose flag lookups go through row()) and at its default,
    both tile heights.  (6,10) and (5,11) are the fallback: the pass route's bg_known turns false, so RIS must store the
    reservoirs of its background tiles for the general kernels."""
    s, _, cam, _, _, hit = inputs(oracle, name, None, w, h)
    bg, mixed, _ = tile_census(hit, w, h)
    assert bg >= 5 and mixed >= 3, f"{bg} all-background and {mixed} mixed 32 x 8 tiles"
    want, res = oracle_frame(oracle, name, None, w, h, K, R, N)
    gpu.set_scene(s)
    f = feats(K, R, N)
    for th in (0, 2):
        for gbuf in (1, KNOB_DEFAULTS["miss.gbuf"]):
            out = {}
            for tiles in (1, 0):
                with knobs(gpu, miss_tiles=tiles, miss_gbuf=gbuf, spatial_th=th):
                    rgb, grid = render(gpu, cam, w, h, f)
                what = f"K={K} R={R} N={N} th={th} miss.gbuf={gbuf} miss.tiles={tiles}"
                assert_bits(rgb, want, f"{what} rgb")
                assert_grid(grid, res, what)
                out[tiles] = (rgb, [np.asarray(a) for a in grid.download()])
            assert_bits(out[1][0], out[0][0], f"K={K} R={R} th={th} miss.gbuf={gbuf} rgb flags on / off")
            for p, q in zip(out[1][1], out[0][1]):
                assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), "grid flags on / off"


# ---- a ghost-zoned tile -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,R", GHOST_PAIRS)
@pytest.mark.parametrize("N", [1, 2])
def test_ghost_zoned_tile_sweep(gpu, oracle, N, K, R):
    """97 x 41 split 2 x 2, rank 3, ghost zone passes x R (none at R = 0, which must be accepted): the fused N = 1 route
    and the N = 2 handle route on a view whose origin, rect and RGB origin differ.  RGB and the grid on the owned rect
    against the oracle's whole frame."""
    from romis_amd import restir
    w, h, passes = 97, 41, 2
    s, _, cam, _, _, _ = inputs(oracle, NIGHT, None, w, h)
    want, (wa, wb) = oracle_frame(oracle, NIGHT, None, w, h, K, R, N)
    tile = restir.tile_plan(w, h, 2, 2, 3, passes * R)
    assert (tile.gwidth - tile.width, tile.gheight - tile.height) == (passes * R, passes * R)
    gpu.set_scene(s)
    rgb, grid = render(gpu, cam, w, h, feats(K, R, N), tile=tile)
    r0 = h - (tile.y0 + tile.height)
    what = f"tile N={N} K={K} R={R}"
    assert_bits(rgb, np.ascontiguousarray(want[r0:r0 + tile.height, tile.x0:tile.x0 + tile.width]), f"{what} rgb")
    pos, col, gw, gm = grid.download()
    own = (slice(None), slice(tile.y0 - tile.gy0, tile.y0 - tile.gy0 + tile.height),
           slice(tile.x0 - tile.gx0, tile.x0 - tile.gx0 + tile.width))
    ref = (slice(None), slice(tile.y0, tile.y0 + tile.height), slice(tile.x0, tile.x0 + tile.width))
    wa, wb = wa.reshape(N, h, w, 4)[ref], wb.reshape(N, h, w, 4)[ref]
    assert_bits(pos[own], wa[..., :3], f"{what} grid position")
    assert_bits(gw[own], wa[..., 3], f"{what} grid W")
    assert_bits(col[own], wb[..., :3], f"{what} grid colour")
    assert np.array_equal(gm[own], np.ascontiguousarray(wb[..., 3]).view(np.uint32)), f"{what} grid M"


# ---- narrow views: AW = the image width ---------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 3, 7, 13, 21, 31])
def test_narrow_views(gpu, oracle, w):
    """Images narrower than a tile at K = 5, R = 10: the window's rows are the image's (AW = w), through the stage
    k_spatial1_ntl and the default whole-frame route."""
    h, K, R = 19, 5, 10
    with knobs(gpu, spatial_th=1):
        run_stage_chain(gpu, oracle, NIGHT, w, h, 1, "biased", K, R)
    s, _, cam, _, _, _ = inputs(oracle, NIGHT, None, w, h)
    want, res = oracle_frame(oracle, NIGHT, None, w, h, K, R)
    rgb, grid = render(gpu, cam, w, h, feats(K, R))
    assert_bits(rgb, want, f"{w}x{h} rgb")
    assert_grid(grid, res, f"{w}x{h}")


# ---- the largest M the handle formats admit -----------------------------------------------------------------
# At R = 0 every neighbour is the pixel itself, accepted on geometry: M reaches M0 (K + 1)^passes exactly.
# (scene, framing, N, M0, K, passes, the M reached, inside the handle's bound)
M_BOUND_CASES = {"point_in": (NIGHT, None, 1, 59, 5, 7, 16516224, True),      # <= kHandleM = 2^24 - 1
                 "point_out": (NIGHT, None, 1, 60, 5, 7, 16796160, False),
                 "grid_in": (CORNELL, "framed", 1, 33, 4, 6, 515625, True),   # <= kHandleMG = 2^19 - 1
                 "grid_out": (CORNELL, "framed", 1, 32, 3, 7, 524288, False),
                 "grid_in_6": (CORNELL, "framed", 1, 32, 3, 6, 131072, True),
                 "point_n2_in": (NIGHT, None, 2, 59, 5, 7, 16516224, True),
                 "point_n2_out": (NIGHT, None, 2, 60, 5, 7, 16796160, False)}


@pytest.mark.parametrize("case", sorted(M_BOUND_CASES))
def test_largest_m_of_the_handle_formats(gpu, oracle, case):
    """spatial_handle_kind admits handles while M0 (K + 1)^passes fits their M field and sends the first frame past it to
    the reservoir planes; both are bit-exact.  At N = 1 the oracle's grid must reach the stated M (on every geometry pixel
    of the nightclub), or a changed default made the case empty; at N = 2 only a handful of pixels reach it, so parity
    alone.  On the point-light route the fused last pass shows which form ran: no final launch with handles, one without."""
    name, framing, N, M0, K, passes, m_max, inside = M_BOUND_CASES[case]
    assert (M0 * (K + 1) ** passes == m_max) and (m_max <= ((1 << 24) - 1 if name == NIGHT else (1 << 19) - 1)) == inside
    s, _, cam, _, _, hit = inputs(oracle, name, framing, W, H)
    want, res = oracle_frame(oracle, name, framing, W, H, K, 0, N, passes, M0)
    if N == 1:
        m = M_of(res[1])[0]
        assert m.max() == m_max, f"{case}: the oracle's largest M is {m.max()}"
        assert hit.mean() >= (0.9 if framing else 0.5)
        if name == NIGHT:
            assert (m[hit] == m_max).all()
    gpu.set_scene(s)
    rgb, grid, n_final, n_spatial = render_counted(gpu, cam, W, H, feats(K, 0, N, passes, M0))
    assert_bits(rgb, want, f"{case} rgb")
    assert_grid(grid, res, case)
    assert n_spatial == passes
    if name == NIGHT and N == 1:
        assert n_final == (0 if inside else 1), f"{case}: {n_final} final launches"
