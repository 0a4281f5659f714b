"""R-MIS / R-OMIS on screen tiles (restir_render_mis_tile, restir_render_mis_tiles, distributed.MisTiles): a tile that
computes a ghost ring of the resample radius reproduces its owned pixels of the whole image bit for bit -- against the
oracle's whole-image render (the oracle has no tile form) and the GPU's own.  Every comparison is of 32-bit words, after
set_seed(SEED, 0)."""
import functools
import os
import socket

import numpy as np
import pytest

from romis_amd import _abi, scene

W, H = 48, 32
SEED = _abi.RESTIR_DEFAULT_SEED
NIGHTCLUB, CORNELL, TEX = "nightclub_128pt", "cornell_parallelogram", "CubeTextured"

# tests/test_gpu_mis.py's MIS_CASES, and one with the EqualSimilarDissimilar strategy
MIS_CASES = {
    "rmis_equal": dict(ray_trace_mode=_abi.MODE_RMIS, num_samples_in_reservoir=2),
    "rmis_balance": dict(ray_trace_mode=_abi.MODE_RMIS, num_samples_in_reservoir=2, mis_weight_rmis=_abi.MIS_BALANCE),
    "rmis_dissimilar": dict(ray_trace_mode=_abi.MODE_RMIS, num_samples_in_reservoir=1, spatial_resample_radius=2,
                            neighbour_selection_strategy=_abi.NEIGHBOURS_DISSIMILAR),
    "romis_direct": dict(ray_trace_mode=_abi.MODE_ROMIS, num_samples_in_reservoir=2),
    "romis_random_k2": dict(ray_trace_mode=_abi.MODE_ROMIS, num_samples_in_reservoir=1, num_neighbours_to_sample=2,
                            neighbour_selection_strategy=_abi.NEIGHBOURS_RANDOM),
    "romis_k7": dict(ray_trace_mode=_abi.MODE_ROMIS, num_samples_in_reservoir=1, num_neighbours_to_sample=7),
    "romis_progressive": dict(ray_trace_mode=_abi.MODE_ROMIS, num_samples_in_reservoir=6, use_progressive_romis=1),
    "romis_progressive_mod2": dict(ray_trace_mode=_abi.MODE_ROMIS, num_samples_in_reservoir=6,
                                   use_progressive_romis=1, progressive_update_mod=2),
    "romis_esd": dict(ray_trace_mode=_abi.MODE_ROMIS, num_samples_in_reservoir=1,
                      neighbour_selection_strategy=3),   # RESTIR_NEIGHBOURS_EQUAL_SIMILAR_DISSIMILAR
}
SCENE_CASES = [(NIGHTCLUB, c) for c in sorted(MIS_CASES)] + [(CORNELL, "rmis_balance"), (CORNELL, "romis_progressive")]

# 2 x 2 even; 4 x 1: tiles 12 wide with r = 10, so a tile's view covers three tiles or all four; an uneven layout whose
# cuts fall off multiples of 32 and 8
UNEVEN_CUTS = {"x": [0, 19, 48], "y": [[0, 13, 32], [0, 13, 32]]}
SPLITS = ["2x2", "4x1", "uneven"]


def features(case, **over):
    f = _abi.default_features(**MIS_CASES[case])
    for k, v in over.items():
        setattr(f, k, v)
    return f


def get_scene(name):
    return scene.load_prebuilt(name) if name == TEX else scene.bench_scene(name)


def split_tiles(split, width, height, radius):
    """The tiles of a split, ghost = radius."""
    from romis_amd import restir
    if split == "uneven":
        L = _abi.TileLayout.from_cuts(width, height, UNEVEN_CUTS)
        return [restir.tile_plan(width, height, 2, 2, q, radius, layout=L) for q in range(4)]
    tx, ty = (int(v) for v in split.split("x"))
    return [restir.tile_plan(width, height, tx, ty, q, radius) for q in range(tx * ty)]


def assert_bits(got, want, what):
    g = np.ascontiguousarray(got, np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)}/{g.size} words differ, first at (row, col, ch) {bad[0].tolist()}: "
                           f"{g[tuple(bad[0])]:#010x} != {w[tuple(bad[0])]:#010x}")


def crop(full, t):
    r0 = full.shape[0] - (t.y0 + t.height)   # tile rows count from the bottom, image rows from the top
    return full[r0:r0 + t.height, t.x0:t.x0 + t.width]


def stitch(gpu, cam, f, tiles, width, height):
    """Every tile rendered alone, each after set_seed(SEED, 0), placed into the whole image."""
    out = np.full((height, width, 3), np.nan, np.float32)
    for t in tiles:
        gpu.set_seed(SEED, 0)
        rgb = gpu.render_mis(cam, width, height, f, tile=t)
        assert rgb.shape == (t.height, t.width, 3)
        crop(out, t)[...] = rgb
    return out


@pytest.fixture(scope="module")
def gpu():
    from romis_amd import build, restir
    build.build()
    r = restir.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def whole(gpu, oracle):
    """(scene name, case) -> (oracle whole frame, GPU whole frame, oracle neighbourhood grid), computed once."""
    @functools.lru_cache(maxsize=None)
    def get(name, case):
        f = features(case)
        sc = get_scene(name)
        osc = oracle.OracleScene(sc)
        cam = scene.camera_for(name, W, H)
        want = oracle.render_mis(osc, cam, f, W, H, SEED, 0)
        gpu.set_scene(sc)
        gpu.set_seed(SEED, 0)
        mine = gpu.render_mis(cam, W, H, f)
        n_t, p_mat = oracle.gbuffer(osc, cam, W, H)
        ol = oracle.lib()
        nbr = oracle.neighbours(osc, f, ol.or_rng_key(SEED, 0, _abi.RESTIR_STAGE_NEIGHBOURS, 0),
                                ol.or_rng_key(SEED, 0, _abi.RESTIR_STAGE_NEIGHBOURS, 1), W, H, n_t, p_mat)
        for a in (want, mine, nbr):
            a.setflags(write=False)
        return want, mine, nbr
    return get


def reads_ghost_ring(nbr, t, width):
    """Some owned pixel of t has an oracle neighbourhood entry outside t's owned rectangle."""
    ys, xs = np.mgrid[t.y0:t.y0 + t.height, t.x0:t.x0 + t.width]
    p = (ys * width + xs).reshape(-1)
    cnt = nbr[0, p]
    ent = nbr[1:, p].astype(np.int64)
    valid = np.arange(ent.shape[0])[:, None] < cnt[None, :]
    ex, ey = ent % width, ent // width
    outside = (ex < t.x0) | (ex >= t.x0 + t.width) | (ey < t.y0) | (ey >= t.y0 + t.height)
    return bool((outside & valid).any())


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name,case", SCENE_CASES)
def test_tiles_stitch_to_whole_frame_and_oracle(gpu, oracle, whole, name, case, split):
    want, mine, nbr = whole(name, case)
    f = features(case)
    tiles = split_tiles(split, W, H, f.spatial_resample_radius)
    for q, t in enumerate(tiles):   # otherwise the test could pass without ever reading the ghost ring
        assert reads_ghost_ring(nbr, t, W), f"{split} tile {q}: no owned pixel's neighbourhood leaves the tile"
    gpu.set_scene(get_scene(name))
    got = stitch(gpu, scene.camera_for(name, W, H), f, tiles, W, H)
    assert_bits(mine, want, f"{name} {case}: the GPU's whole frame vs the oracle")
    assert_bits(got, mine, f"{name} {case} {split}: stitched tiles vs the GPU's whole frame")
    assert_bits(got, want, f"{name} {case} {split}: stitched tiles vs the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rmis_balance", "romis_direct"])
def test_textured_scene_tiles(gpu, oracle, whole, case):
    """Texture mapping on: the target pdfs read the texCoord plane, by view index on a tile."""
    want, mine, _ = whole(TEX, case)
    f = features(case)
    assert f.enable_texture_mapping == 1
    gpu.set_scene(get_scene(TEX))
    got = stitch(gpu, scene.camera_for(TEX, W, H), f, split_tiles("2x2", W, H, f.spatial_resample_radius), W, H)
    assert_bits(mine, want, f"{case}: the GPU's whole textured frame vs the oracle")
    assert_bits(got, want, f"{case}: stitched textured tiles vs the oracle")
    f0 = features(case, enable_texture_mapping=0)
    gpu.set_seed(SEED, 0)
    assert not np.array_equal(gpu.render_mis(scene.camera_for(TEX, W, H), W, H, f0), mine)   # the texture matters


@pytest.mark.gpu
def test_ragged_tiles(gpu, oracle):
    """61 x 37 in 3 x 2: tiles that are multiples of neither 64 lanes nor 256-pixel blocks, one of an odd size (the even
    split gives the remainders to the first column and row: tile 0 is 21 x 19, the last 20 x 18)."""
    w, h = 61, 37
    f = features("romis_direct")
    sc = get_scene(NIGHTCLUB)
    cam = scene.camera_for(NIGHTCLUB, w, h)
    tiles = split_tiles("3x2", w, h, f.spatial_resample_radius)
    assert len(tiles) == 6 and (tiles[0].width * tiles[0].height) % 2 == 1
    assert all((t.width * t.height) % 64 for t in tiles)
    want = oracle.render_mis(oracle.OracleScene(sc), cam, f, w, h, SEED, 0)
    gpu.set_scene(sc)
    assert_bits(stitch(gpu, cam, f, tiles, w, h), want, "ragged tiles vs the oracle")
    # the same cuts mirrored, so that the last tile is the odd 21 x 19 one
    from romis_amd import restir
    L = _abi.TileLayout.from_cuts(w, h, {"x": [0, 20, 40, 61], "y": [[0, 18, 37]] * 3})
    tiles = [restir.tile_plan(w, h, 3, 2, q, f.spatial_resample_radius, layout=L) for q in range(6)]
    assert (tiles[-1].width * tiles[-1].height) % 2 == 1 and all((t.width * t.height) % 64 for t in tiles)
    assert_bits(stitch(gpu, cam, f, tiles, w, h), want, "ragged tiles, the last one odd, vs the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 5])
def test_chunked_romis_scratch_on_tiles(gpu, oracle, whole, chunk):
    """mis.chunk: the T x N samples in several k_romis_samples / k_romis_accum pairs, counted over owned pixels."""
    want, _, _ = whole(NIGHTCLUB, "romis_progressive")
    f = features("romis_progressive")
    gpu.set_scene(get_scene(NIGHTCLUB))
    gpu.set_tuning("mis.chunk", chunk)
    try:
        got = stitch(gpu, scene.camera_for(NIGHTCLUB, W, H), f, split_tiles("2x2", W, H, f.spatial_resample_radius), W, H)
    finally:
        gpu.set_tuning("mis.chunk", 0)
    assert_bits(got, want, f"chunk {chunk}: stitched tiles vs the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rmis_equal", "romis_direct"])
def test_render_mis_tiled(gpu, oracle, whole, case):
    """restir_render_mis_tiles: the whole image, one frame index consumed whatever the number of tiles."""
    want, _, _ = whole(NIGHTCLUB, case)
    f = features(case)
    sc = get_scene(NIGHTCLUB)
    cam = scene.camera_for(NIGHTCLUB, W, H)
    gpu.set_scene(sc)
    gpu.set_seed(SEED, 0)
    assert_bits(gpu.render_mis_tiled(cam, W, H, f, tiles=(2, 2)), want, f"{case}: render_mis_tiled 2x2")
    assert_bits(gpu.render_mis(cam, W, H, f), oracle.render_mis(oracle.OracleScene(sc), cam, f, W, H, SEED, 1),
                f"{case}: the render after render_mis_tiled is frame 1")
    gpu.set_seed(SEED, 0)
    L = _abi.TileLayout.from_cuts(W, H, UNEVEN_CUTS)
    assert_bits(gpu.render_mis_tiled(cam, W, H, f, layout=L), want, f"{case}: render_mis_tiled over an uneven layout")
    gpu.set_seed(SEED, 0)
    assert_bits(gpu.render_mis_tiled(cam, W, H, f, tiles=(1, 1)), want, f"{case}: render_mis_tiled 1x1")
    assert gpu.download_rgb(W, H).shape == (H, W, 3)


@pytest.mark.gpu
def test_tile_leaves_its_image_for_download(gpu, whole):
    want, _, _ = whole(NIGHTCLUB, "rmis_equal")
    f = features("rmis_equal")
    gpu.set_scene(get_scene(NIGHTCLUB))
    t = split_tiles("2x2", W, H, f.spatial_resample_radius)[3]
    gpu.set_seed(SEED, 0)
    gpu.render_mis(scene.camera_for(NIGHTCLUB, W, H), W, H, f, tile=t)
    assert_bits(gpu.download_rgb(t.width, t.height), crop(want, t), "restir_download_rgb after a tile")


@pytest.mark.gpu
def test_contract_errors(gpu, tmp_path):
    from romis_amd import restir
    gpu.set_scene(get_scene(NIGHTCLUB))
    cam = scene.camera_for(NIGHTCLUB, W, H)
    f = features("romis_direct")
    r = f.spatial_resample_radius
    good = restir.tile_plan(W, H, 2, 2, 1, r)

    def raises(status, feats, tile, match=None):
        with pytest.raises(_abi.RestirError, match=status) as e:
            gpu.render_mis(cam, W, H, feats, tile=tile)
        if match:
            assert match in str(e.value)

    raises("INVALID", f, restir.tile_plan(W, H, 2, 2, 1, r - 1), "radius")          # ghost narrower than r
    raises("INVALID", features("rmis_equal"), restir.tile_plan(W, H, 2, 2, 1, r - 1), "radius")
    raises("INVALID", _abi.default_features(), restir.tile_plan(W, H, 2, 2, 1, 2 * r))   # ReSTIR mode
    bad = restir.tile_plan(W, H, 2, 2, 1, r)
    bad.width += 1                                                                   # past the image
    raises("INVALID", f, bad, "inconsistent")
    bad = restir.tile_plan(W, H, 2, 2, 1, r)
    bad.global_width += 1
    raises("INVALID", f, bad)
    raises("UNSUPPORTED", features("romis_direct", num_neighbours_to_sample=8), good)
    # the corner rule is the image's: a 2 x 2 corner window holds fewer than k = 5 candidates, whatever tile is asked for
    fr1 = features("romis_direct", spatial_resample_radius=1)
    raises("INVALID", fr1, restir.tile_plan(W, H, 3, 3, 4, 1), "corner")
    fv = features("romis_direct", save_alphas_visualisation=1)
    gpu.set_renders_dir(tmp_path)
    try:
        raises("UNSUPPORTED", fv, good, "whole-image")
    finally:
        gpu.set_renders_dir(None)
    assert list(tmp_path.iterdir()) == []
    gpu.set_seed(SEED, 0)
    assert gpu.render_mis(cam, W, H, fv, tile=good).shape == (good.height, good.width, 3)   # no dir: flag ignored
    with pytest.raises(_abi.RestirError, match="UNSUPPORTED"):                        # restir_render keeps refusing
        gpu.render_restir(None, cam, W, H, f, tile=good, want_grid=False)


# ---- distributed.MisTiles over gloo: every rank its own process and context on the one GPU ---------------------------
MT_CASES = ["rmis_balance", "romis_direct"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, tiles, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from romis_amd import distributed, restir
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    r = restir.Renderer(0)
    r.set_scene(get_scene(NIGHTCLUB))
    cam = scene.camera_for(NIGHTCLUB, W, H)
    for case in MT_CASES:
        mt = distributed.MisTiles(r, W, H, tiles, rank, features(case))
        r.set_seed(SEED, 0)
        full = mt.render(cam, gather=True)
        r.set_seed(SEED, 0)
        own = mt.render(cam, gather=False)
        assert own.shape == (mt.tile.height, mt.tile.width, 3)
        # the gather alone on tiles of -0.0: a float sum of zero-padded images would return +0.0
        probe = mt.gather(np.full((mt.tile.height, mt.tile.width, 3), -0.0, np.float32))
        assert (full is None) == (rank != 0) and (probe is None) == (rank != 0)
        if rank == 0:
            np.save(os.path.join(out_dir, f"{case}.npy"), full)
            np.save(os.path.join(out_dir, f"{case}_own.npy"), own)
            np.save(os.path.join(out_dir, f"{case}_probe.npy"), probe)
    dist.barrier()
    r.close()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,tiles", [(2, (2, 1)), (4, (2, 2))])
def test_mis_tiles_over_gloo(tmp_path, world, tiles):
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    from romis_amd import restir
    mp.spawn(_worker, args=(world, _free_port(), tiles, str(tmp_path)), nprocs=world, join=True)
    r = restir.Renderer(0)
    try:
        r.set_scene(get_scene(NIGHTCLUB))
        cam = scene.camera_for(NIGHTCLUB, W, H)
        for case in MT_CASES:
            f = features(case)
            r.set_seed(SEED, 0)
            want = r.render_mis(cam, W, H, f)
            assert_bits(np.load(str(tmp_path / f"{case}.npy")), want, f"{case}: rank 0's gathered image")
            t0 = restir.tile_plan(W, H, tiles[0], tiles[1], 0, f.spatial_resample_radius)
            assert_bits(np.load(str(tmp_path / f"{case}_own.npy")), crop(want, t0), f"{case}: rank 0's own tile")
            probe = np.load(str(tmp_path / f"{case}_probe.npy"))
            assert probe.shape == (H, W, 3) and (probe.view(np.uint32) == 0x80000000).all(), "the gather changed a -0.0"
    finally:
        r.close()
