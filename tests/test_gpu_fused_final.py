"""final.fuse (the default): restir_render's last N = 1 biased pass over point-light handles shades its own 32 x 16
tiles (k_spatial1hg_t2_final) instead of handing its grid to k_final_n1_sorted.  The fused kernel applies final
shading's operations to the reservoir the pass holds in registers, so every frame must equal the two-kernel frame
(final.fuse = 0) bit for bit -- RGB and, where a grid is returned, the grid -- and the oracle's frame.  Where either
kernel's conditions fail the host keeps the two kernels; RESTIR_K_FINAL's launch count shows which path ran.
"""
import numpy as np
import pytest

from romis_amd import _abi, scene
from test_gpu_parity import SEED, _extreme_scene, assert_bits, assert_grid, get_scene

pytestmark = pytest.mark.gpu

NAME = "nightclub_128pt"


@pytest.fixture(scope="module")
def gpu():
    from romis_amd import build, restir
    build.build()
    r = restir.Renderer(0)
    yield r
    r.close()


def features(passes=1, M=32, **kw):
    kw.setdefault("num_samples_in_reservoir", 1)
    kw.setdefault("temporal_reuse", 0)
    return _abi.default_features(spatial_resampling_passes=passes, initial_light_samples=M, **kw)


def render(gpu, fuse, cam, w, h, f, tile=None, want_grid=True, prev=None, frame=0):
    """One seeded frame with final.fuse = fuse: (rgb, downloaded grid planes or None, ReservoirGrid or None)."""
    gpu.set_tuning("final.fuse", fuse)
    try:
        if prev is None:
            gpu.set_seed(SEED, frame)
        rgb, grid = gpu.render_restir(prev, cam, w, h, f, tile=tile, want_grid=want_grid)
    finally:
        gpu.set_tuning("final.fuse", 1)
    planes = [np.asarray(a) for a in grid.download()] if grid is not None else None
    return rgb, planes, grid


def same_rgb(a, b, what):
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    bad = np.flatnonzero(a.view(np.uint32).reshape(-1) != b.view(np.uint32).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size}/{a.size} rgb words differ, first {bad[:4].tolist()}"


def same_grid(a, b, what, tile=None):
    # a tiled frame's grid is defined on the owned rect (the ghost ring holds intermediate values, include/restir_c.h)
    own = (slice(None), slice(tile.y0 - tile.gy0, tile.y0 - tile.gy0 + tile.height),
           slice(tile.x0 - tile.gx0, tile.x0 - tile.gx0 + tile.width)) if tile is not None else (slice(None),)
    for plane, (p, q) in zip(("pos", "col", "W", "M"), zip(a, b)):
        assert np.array_equal(p[own].view(np.uint32), q[own].view(np.uint32)), f"{what}: grid {plane}"


def fused_equals_unfused(gpu, cam, w, h, f, what, tile=None):
    """RGB with and without a returned grid, and the grid, fused against unfused; returns the fused (rgb, no-grid rgb,
    ReservoirGrid)."""
    rgb1, g1, grid1 = render(gpu, 1, cam, w, h, f, tile)
    rgb0, g0, _ = render(gpu, 0, cam, w, h, f, tile)
    same_rgb(rgb1, rgb0, f"{what} rgb")
    same_grid(g1, g0, what, tile)
    ng1, _, _ = render(gpu, 1, cam, w, h, f, tile, want_grid=False)
    ng0, _, _ = render(gpu, 0, cam, w, h, f, tile, want_grid=False)
    same_rgb(ng1, ng0, f"{what} rgb without a grid")
    same_rgb(ng1, rgb0, f"{what} rgb without a grid against the grid frame's")
    return rgb1, ng1, grid1


def final_launches(gpu, fuse, cam, w, h, f, want_grid=False):
    """RESTIR_K_FINAL launches of one frame (timing on, every kernel bracketed), and the frame's rgb."""
    gpu.enable_timing(True)
    try:
        gpu.set_tuning("timing.mask", -1)
        gpu.reset_timings()
        rgb, _, _ = render(gpu, fuse, cam, w, h, f, want_grid=want_grid)
        t = gpu.timings()
    finally:
        gpu.enable_timing(False)
    return t["final"][1], t["spatial"][1], rgb


# 1 x 1: a single lane live in a 512-thread block; 33 x 17: one pixel past a 32 x 16 tile on each axis (dead lanes at
# every barrier); 64 x 1: one row; 37 x 23 with two passes: only the last fuses, the first writes handles only;
# 70 x 150: several tile rows, ragged bottom; 96 x 64: whole tiles only
SHAPES = [(1, 1, 1), (33, 17, 1), (64, 1, 1), (37, 23, 2), (70, 150, 1), (96, 64, 1)]


@pytest.mark.parametrize("M", [32, 1])
@pytest.mark.parametrize("w,h,passes", SHAPES)
def test_fused_equals_unfused(gpu, w, h, passes, M):
    gpu.set_scene(get_scene(NAME))
    fused_equals_unfused(gpu, scene.camera_for(NAME, w, h), w, h, features(passes, M), f"{w}x{h} passes={passes} M={M}")


@pytest.mark.parametrize("passes", [1, 2])
def test_fused_equals_unfused_on_a_ghost_zoned_tile(gpu, passes):
    """333 x 190 split 2 x 2, rank 3: the owned rect, the view and the RGB origin all differ; the grid on the owned rect."""
    from romis_amd import restir
    w, h = 333, 190
    gpu.set_scene(get_scene(NAME))
    f = features(passes)
    tile = restir.tile_plan(w, h, 2, 2, 3, passes * f.spatial_resample_radius)
    fused_equals_unfused(gpu, scene.camera_for(NAME, w, h), w, h, f, f"tile passes={passes}", tile)


@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("miss_tiles", [1, 0])
def test_fused_equals_unfused_with_background_tiles(gpu, tiled, miss_tiles):
    """640 x 360 through camera_for("nightclub_128pt", 640, 360), whole and as rank 3 of a 2 x 2 plan, with the
    background-tile flags on and off.  On the CPU (the oracle's primary rays) 24.5 % of this frame's pixels miss the
    scene: of its 20 x 23 tiles of 32 x 16 pixels 97 are all background (the block-uniform exit that writes the tile's
    RGB), 56 mixed and 307 all geometry, and 16 have exactly one all-background 32 x 8 half (lanes of a background RIS
    tile inside a shading block); rank 3's owned rect has 10 / 10 / 100."""
    from romis_amd import restir
    w, h = 640, 360
    gpu.set_scene(get_scene(NAME))
    f = features(1)
    tile = restir.tile_plan(w, h, 2, 2, 3, f.spatial_resample_radius) if tiled else None
    gpu.set_tuning("miss.tiles", miss_tiles)
    try:
        fused_equals_unfused(gpu, scene.camera_for(NAME, w, h), w, h, f, f"background tiled={tiled} flags={miss_tiles}", tile)
    finally:
        gpu.set_tuning("miss.tiles", 1)


@pytest.mark.parametrize("w,h,passes", SHAPES[:4])
def test_fused_matches_oracle(gpu, oracle, w, h, passes):
    s = get_scene(NAME)
    gpu.set_scene(s)
    cam = scene.camera_for(NAME, w, h)
    f = features(passes)
    rgb, _, grid = render(gpu, 1, cam, w, h, f)
    rgb_ng, _, _ = render(gpu, 1, cam, w, h, f, want_grid=False)
    want, res, _ = oracle.render_frame(oracle.OracleScene(s), cam, f, w, h, SEED, 0)
    assert_bits(rgb, want, f"{w}x{h} passes={passes} rgb")
    assert_grid(grid, res, f"{w}x{h} passes={passes}")
    assert_bits(rgb_ng, want, f"no grid {w}x{h} passes={passes} rgb")


@pytest.mark.parametrize("variant", ["huge_colour", "far_lights", "mixed_shininess"])
def test_fused_extreme_scenes(gpu, oracle, variant):
    """The need test, the miss path's finiteness checks and the specular power inside the fused epilogue: colour x
    reflectance products past 2^120, lights whose squared distance overflows, mixed integer / general exponents."""
    w, h = 96, 64
    s = _extreme_scene(variant)
    gpu.set_scene(s)
    cam = scene.nightclub_camera(w, h)
    f = features(1)
    rgb, _, grid = fused_equals_unfused(gpu, cam, w, h, f, variant)
    want, res, _ = oracle.render_frame(oracle.OracleScene(s), cam, f, w, h, SEED, 0)
    assert_bits(rgb, want, f"{variant} rgb")
    assert_grid(grid, res, variant)


FALLBACKS = {
    "N2": (NAME, dict(num_samples_in_reservoir=2), {}),
    "light_grid": ("cornell_1024", {}, {}),
    "qbvh": (NAME, {}, {"final.qbvh": 1}),
    "unsorted": (NAME, {}, {"final.sort": 0}),
    "unbiased_vis": (NAME, dict(unbiased_combination=1, spatial_reuse_visibility_check=1), {}),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallbacks_keep_two_kernels(gpu, case):
    """Where the pass is not k_spatial1hg_t2 or final shading not k_final_n1_sorted the host launches both kernels:
    the frame equals the final.fuse = 0 frame and RESTIR_K_FINAL counts a launch."""
    name, feat, tune = FALLBACKS[case]
    w, h = 96, 64
    gpu.set_scene(get_scene(name))
    cam = scene.camera_for(name, w, h)
    f = features(1, **feat)
    try:
        for k, v in tune.items():
            gpu.set_tuning(k, v)
        n1, _, rgb1 = final_launches(gpu, 1, cam, w, h, f)
        n0, _, rgb0 = final_launches(gpu, 0, cam, w, h, f)
    finally:
        gpu.set_tuning("final.qbvh", 2)
        gpu.set_tuning("final.sort", 1)
    assert n1 == 1 and n0 == 1, f"{case}: final launches {n1} (fuse on) / {n0} (off)"
    same_rgb(rgb1, rgb0, case)


@pytest.mark.parametrize("want_grid", [False, True])
def test_fused_frame_has_no_final_launch(gpu, want_grid):
    w, h = 96, 64
    gpu.set_scene(get_scene(NAME))
    cam = scene.camera_for(NAME, w, h)
    f = features(2)
    n1, s1, rgb1 = final_launches(gpu, 1, cam, w, h, f, want_grid)
    n0, s0, rgb0 = final_launches(gpu, 0, cam, w, h, f, want_grid)
    assert (n1, s1) == (0, 2), f"fused: {n1} final launches, {s1} spatial"
    assert (n0, s0) == (1, 2), f"unfused: {n0} final launches, {s0} spatial"
    same_rgb(rgb1, rgb0, "timed frame")


def test_fused_temporal_sequence(gpu):
    """Three frames of C3's features (two passes, temporal reuse, the grid threaded through): the fused kernel writes
    the grid and the frame handles the next frame's temporal reuse reads."""
    w, h = 96, 64
    gpu.set_scene(get_scene(NAME))
    cam = scene.camera_for(NAME, w, h)
    f = features(2, temporal_reuse=1)
    out = {}
    for fuse in (1, 0):
        prev, frames = None, []
        for frame in range(3):
            rgb, planes, prev = render(gpu, fuse, cam, w, h, f, prev=prev)
            frames.append((rgb, planes))
        out[fuse] = frames
    for frame in range(3):
        same_rgb(out[1][frame][0], out[0][frame][0], f"frame {frame} rgb")
        same_grid(out[1][frame][1], out[0][frame][1], f"frame {frame}")
