"""Dynamic scenes on the GPU: restir_update_meshes (vertices moved, the BVH refitted on the device) and restir_set_lights
(another light list over the same geometry), every comparison bit for bit.

Arrays: after each deformation of test_bvh_refit the device's nodes and quantized words equal the host's refit_bvh and
quantize_nodes (tools/refit_check --dump over the same original and moved triangles), the triangle records equal numpy's
float32 v1 - v0, the normals the supplied ones, and a second update back restores the upload's arrays.  Cube at
bvh.max_leaf 1 (23 nodes, several levels in one workgroup), the nightclub at the default leaf, Monkey at leaf 2 (too
large for LDS: the two-launch path) and at leaf 5 (fits).

Frames: the tree only prunes, so a frame after an update equals the oracle's frame of the moved scene (its brute-force
rays take any triangle list) and the frame of a fresh context's set_scene(moved scene).  Every sequence asserts that the
oracle's G-buffer changed on >= 16 pixels from one frame to the next, so a stale tree or a stale kept G-buffer cannot
pass.  Frames are 70 x 37 and 33 x 17.
"""
import ctypes as C
import dataclasses
import subprocess

import numpy as np
import pytest

from romis_amd import _abi, scene
from test_bvh_refit import bounds, deform, refit_tool, triangles_of, write_tri, DEFORMATIONS, _hash_unit
from test_gpu_parity import SEED, assert_bits, assert_grid, get_scene
from test_gpu_scene_shapes import _mixed_lights, counted, feats

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 70, 37
W2, H2 = 33, 17
NIGHT, CORNELL, MONKEY, CUBE = "nightclub_128pt", "cornell_1024", "Monkey", "Cube"
NIGHT_BOX = 9       # a box on the nightclub's floor, 92 of the 70 x 37 default view's pixels
CORNELL_BOX = 5     # the Cornell box's short block


@pytest.fixture()
def gpu():
    """A context of its own per test: what it keeps across an update is the subject."""
    from romis_amd import build, restir
    build.build()
    r = restir.Renderer(0)
    yield r
    r.close()


def the_scene(name):
    return scene.load_prebuilt(name) if name in (MONKEY, CUBE) else get_scene(name)


def positions_of(s):
    return [np.ascontiguousarray(m.positions, f32) for m in s.meshes]


def with_positions(s, positions, normals=None, lights=None):
    meshes = [dataclasses.replace(m, positions=p, normals=m.normals if normals is None else normals[i])
              for i, (m, p) in enumerate(zip(s.meshes, positions))]
    return scene.Scene(meshes, s.lights if lights is None else lights, s.name)


def camera_of(name, w, h):
    if name == NIGHT:
        return scene.nightclub_camera(w, h)
    return scene.cornell_framed_camera(w, h)


def changed(a, b):
    """{mesh: (positions, None)} of the meshes whose positions differ."""
    return {i: (q, None) for i, (p, q) in enumerate(zip(a, b)) if not np.array_equal(p.view(np.uint32), q.view(np.uint32))}


def gbuf_pixels_changed(g0, g1):
    return int(np.count_nonzero((g0[0].view(np.uint32) != g1[0].view(np.uint32)).any(axis=1) |
                                (g0[1].view(np.uint32) != g1[1].view(np.uint32)).any(axis=1)))


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} / {b.shape}"
    bad = np.flatnonzero(a.view(np.uint32).reshape(-1) != b.view(np.uint32).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} words differ, first at {bad[0]}: {a.reshape(-1)[bad[0]]} / {b.reshape(-1)[bad[0]]}"


# ---- arrays ------------------------------------------------------------------------------------------------------
ARRAY_SCENES = {"cube_leaf1": (CUBE, 1), "nightclub": (NIGHT, 2), "monkey_leaf2": (MONKEY, 2), "monkey_leaf5": (MONKEY, 5)}
_refits = {}


def host_refit(tmp, name, leaf, kind, tris0, tris1):
    """refit_bvh(build_bvh(tris0, leaf), tris1) and its quantize_nodes, from tools/refit_check --dump."""
    if (name, leaf, kind) not in _refits:
        a, b, out = (str(tmp / f"{name}.{leaf}.{kind}.{x}") for x in ("orig.tri", "moved.tri", "bin"))
        write_tri(a, tris0)
        write_tri(b, tris1)
        subprocess.run([refit_tool(), "--dump", str(leaf), a, b, out], check=True)
        raw = np.fromfile(out, np.uint32)
        n, t, q_ok = (int(v) for v in raw[:3])
        nq = 4 * n if q_ok else 4
        nodes = raw[3:3 + 8 * n].view(f32).reshape(n, 8)
        words = raw[3 + 8 * n:3 + 8 * n + nq].reshape(-1, 4)
        order = raw[3 + 8 * n + nq:3 + 8 * n + nq + t]
        _refits[(name, leaf, kind)] = (nodes, words if q_ok else None, order)
    return _refits[(name, leaf, kind)]


def assert_scene_arrays(got, nodes, words, order, tris, normals_by_tri, mesh_of_tri, what):
    same_bits(got["nodes"], nodes, f"{what} nodes")
    assert (got["nodes_q"] is None) == (words is None), f"{what}: quantized nodes"
    if words is not None:
        same_bits(got["nodes_q"], words, f"{what} nodes_q")
    t = tris[order]
    same_bits(got["tri_v0"][:, :3], t[:, 0], f"{what} v0")
    assert np.array_equal(got["tri_v0"][:, 3].view(np.uint32), order), f"{what} v0.w"
    same_bits(got["tri_e1"][:, :3], t[:, 1] - t[:, 0], f"{what} e1")
    same_bits(got["tri_e2"][:, :3], t[:, 2] - t[:, 0], f"{what} e2")
    for k, key in enumerate(("tri_n0", "tri_n1", "tri_n2")):
        same_bits(got[key][:, :3], normals_by_tri[:, k], f"{what} {key}")
    assert np.array_equal(got["tri_n0"][:, 3].view(np.uint32), mesh_of_tri), f"{what} n0.w"


@pytest.mark.parametrize("kind", DEFORMATIONS)
@pytest.mark.parametrize("case", sorted(ARRAY_SCENES))
def test_refitted_arrays_equal_the_host_refit(gpu, tmp_path, case, kind):
    name, leaf = ARRAY_SCENES[case]
    s = the_scene(name)
    tri = [np.asarray(m.triangles, np.int64) for m in s.meshes]
    mesh_of_tri = np.concatenate([np.full(len(t), i, np.uint32) for i, t in enumerate(tri)])
    p0 = positions_of(s)
    n0 = [np.ascontiguousarray(m.normals, f32) for m in s.meshes]
    p1 = deform(p0, kind)
    # the jitter also carries new normals (hashed, not unit: the arrays are compared, nothing is shaded)
    n1 = [_hash_unit(len(n), 77 + i) for i, n in enumerate(n0)] if kind == "jitter" else n0
    gpu.set_tuning("bvh.max_leaf", leaf)
    gpu.set_scene(s)
    info = gpu.scene_info()
    fits = info.bvh_lds_bytes <= 65536
    assert fits == (case != "monkey_leaf2") and (case != "cube_leaf1" or info.num_nodes == 23)
    upload = gpu.debug_scene()
    nodes, words, order = host_refit(tmp_path, name, leaf, "identity", triangles_of(p0, tri), triangles_of(p0, tri))
    assert_scene_arrays(upload, nodes, words, order, triangles_of(p0, tri), triangles_of(n0, tri), mesh_of_tri, f"{case} upload")

    ups = changed(p0, p1) if kind != "identity" else {0: (p0[0], None)}
    if kind == "jitter":
        ups = {i: (p1[i], n1[i]) for i in range(len(p1))}
    if kind in ("grow", "collapse") and len(p0) > 1:
        assert len(ups) == 1   # one mesh of several: the others' vertices stay where the upload put them
    gpu.update_meshes(ups)
    nodes, words, order = host_refit(tmp_path, name, leaf, kind, triangles_of(p0, tri), triangles_of(p1, tri))
    assert_scene_arrays(gpu.debug_scene(), nodes, words, order, triangles_of(p1, tri), triangles_of(n1, tri), mesh_of_tri,
                        f"{case} {kind}")
    after = gpu.scene_info()
    assert (after.num_nodes, after.num_tris, after.nodes_q_ok) == (info.num_nodes, info.num_tris, info.nodes_q_ok)

    gpu.update_meshes({i: (p0[i], n0[i]) for i in range(len(p0))})
    back = gpu.debug_scene()
    for key, a in upload.items():
        if a is not None:
            same_bits(back[key], a, f"{case} {kind} and back: {key}")


# ---- frames against the oracle -----------------------------------------------------------------------------------
def moving_sequence(gpu, oracle, name, mesh, step, f, w, h, what, leaf=None, frames=4):
    """`frames` frames of one camera; before each but the first `mesh` moves by `step`.  Each equals the oracle's frame
    of the scene as it then stands (prev threaded on both sides when f.temporal_reuse); a last still frame reuses."""
    s = the_scene(name)
    if leaf is not None:
        gpu.set_tuning("bvh.max_leaf", leaf)
    gpu.set_scene(s)
    gpu.set_seed(SEED, 0)
    cam = camera_of(name, w, h)
    p0 = positions_of(s)
    prev, oprev, gb_prev, osc = None, None, None, None
    reuses = []
    for frame in range(frames + 1):
        still = frame == frames
        if not still:
            p = [q.copy() for q in p0]
            p[mesh] = (p0[mesh] + np.asarray(step, f32) * f32(frame)).astype(f32)
            if frame:
                gpu.update_meshes({mesh: (p[mesh], None)})
            osc = oracle.OracleScene(with_positions(s, p))
        rgb, grid = gpu.render_restir(prev if f.temporal_reuse else None, cam, w, h, f)
        want, res, gb = oracle.render_frame(osc, cam, f, w, h, SEED, frame, prev=oprev if f.temporal_reuse else None)
        assert_bits(rgb, want, f"{what} frame {frame} rgb")
        assert_grid(grid, res, f"{what} frame {frame}")
        if frame and not still:
            assert gbuf_pixels_changed(gb_prev, gb) >= 16, f"{what} frame {frame}: the move is invisible"
        prev, oprev, gb_prev = grid, res, gb
        reuses.append(gpu.gbuf_reuses())
    return reuses


@pytest.mark.parametrize("passes", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 2])
def test_nightclub_box_moves(gpu, oracle, N, passes):
    what = f"nightclub N={N} passes={passes}"
    reuses = moving_sequence(gpu, oracle, NIGHT, NIGHT_BOX, (0.0, 0.4, 0.3), feats(N, passes, temporal=1), W, H, what)
    info = gpu.scene_info()
    assert info.num_lights == 128 and info.bvh_lds_bytes <= 65536
    # no frame after an update reads the kept G-buffer; the still frame after them does
    assert reuses[:4] == [0, 0, 0, 0] and reuses[4] == 1, f"{what}: gbuf_reuses {reuses}"


def test_nightclub_box_moves_small_frame(gpu, oracle):
    reuses = moving_sequence(gpu, oracle, NIGHT, NIGHT_BOX, (0.0, 0.8, 0.6), feats(1, 2, temporal=1), W2, H2, "nightclub 33x17")
    assert reuses == [0, 0, 0, 0, 1]


def test_cornell_grid_unbiased_block_moves(gpu, oracle):
    f = feats(1, 1, unbiased=1, vis=1)
    reuses = moving_sequence(gpu, oracle, CORNELL, CORNELL_BOX, (0.05, 0.06, 0.0), f, W, H, "cornell 32x32 unbiased")
    assert gpu.scene_info().lights_grid == 1 and reuses == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("N", [1, 2])
def test_monkey_leaf2_moves(gpu, oracle, N):
    """Too large for LDS: the two-launch refit, then the general (unfused, unstaged) frame kernels."""
    reuses = moving_sequence(gpu, oracle, MONKEY, 0, (0.04, -0.03, 0.02), feats(N, 2, temporal=1), W2, H2, f"Monkey N={N}", leaf=2)
    assert gpu.scene_info().bvh_lds_bytes > 65536 and reuses == [0] * 5


def toward_camera(oracle, s, cam, mesh, t):
    """positions with `mesh` moved a fraction t of the way from its centroid to the camera."""
    origin = np.asarray(list(oracle.camera_frame(cam).origin), f32)
    p = positions_of(s)
    p[mesh] = (p[mesh] + (origin - p[mesh].mean(axis=0).astype(f32)) * f32(t)).astype(f32)
    return p


@pytest.mark.parametrize("w,h", [(W, H), (W2, H2)])
def test_update_equals_a_fresh_upload_and_leaves_the_old_root_box(gpu, oracle, w, h):
    """The box moves 35 % of the way to the camera: out of the uploaded scene's bounds and still in view.  A tree whose
    root did not grow loses those hits.  The frame equals the oracle's and a fresh context's set_scene(moved scene)."""
    from romis_amd import restir
    s = the_scene(NIGHT)
    cam = camera_of(NIGHT, w, h)
    p1 = toward_camera(oracle, s, cam, NIGHT_BOX, 0.35)
    lo, hi = bounds(positions_of(s))
    moved = with_positions(s, p1)
    f = feats(1, 2)
    want, res, gb = oracle.render_frame(oracle.OracleScene(moved), cam, f, w, h, SEED, 3)
    hit = gb[1][:, 3].view(np.uint32) == NIGHT_BOX
    outside = hit & ((gb[1][:, :3] < lo - f32(0.01)).any(axis=1) | (gb[1][:, :3] > hi + f32(0.01)).any(axis=1))
    assert outside.sum() >= 16, f"{outside.sum()} pixels see the box outside the old bounds"

    gpu.set_scene(s)
    gpu.set_seed(SEED, 2)
    gpu.render_restir(None, cam, w, h, f)
    gpu.update_meshes({NIGHT_BOX: (p1[NIGHT_BOX], None)})
    rgb, grid = gpu.render_restir(None, cam, w, h, f)
    assert_bits(rgb, want, "updated rgb")
    assert_grid(grid, res, "updated")
    other = restir.Renderer(0)
    try:
        other.set_scene(moved)
        other.set_seed(SEED, 3)
        rgb2, grid2 = other.render_restir(None, cam, w, h, f)
        same_bits(rgb, rgb2, "update against a fresh upload: rgb")
        for a, b in zip(grid.download(), grid2.download()):
            same_bits(a, b, "update against a fresh upload: grid")
    finally:
        other.close()


def test_rmis_frame_after_an_update(gpu, oracle):
    from test_gpu_mis import MIS_CASES, bits_equal
    s = the_scene(NIGHT)
    cam = camera_of(NIGHT, W2, H2)
    f = _abi.default_features(**MIS_CASES["rmis_equal"])
    f.max_iterations_mis = 2
    p1 = toward_camera(oracle, s, cam, NIGHT_BOX, 0.2)
    gpu.set_scene(s)
    gpu.set_seed(SEED, 0)
    before = gpu.render_mis(cam, W2, H2, f)
    gpu.update_meshes({NIGHT_BOX: (p1[NIGHT_BOX], None)})
    gpu.set_seed(SEED, 0)
    got = gpu.render_mis(cam, W2, H2, f)
    bits_equal(got, oracle.render_mis(oracle.OracleScene(with_positions(s, p1)), cam, f, W2, H2, SEED, 0), "R-MIS after an update")
    assert np.count_nonzero((got.view(np.uint32) != before.view(np.uint32)).any(axis=2)) >= 16


def test_ghost_zoned_tile_after_an_update(gpu, oracle):
    from romis_amd import restir
    s = the_scene(NIGHT)
    cam = camera_of(NIGHT, W, H)
    f = feats(1, 2)
    tile = restir.tile_plan(W, H, 2, 1, 1, 2 * f.spatial_resample_radius)
    assert tile.gwidth - tile.width == 2 * f.spatial_resample_radius
    p1 = toward_camera(oracle, s, cam, NIGHT_BOX, 0.35)
    gpu.set_scene(s)
    gpu.set_seed(SEED, 0)
    before, _ = gpu.render_restir(None, cam, W, H, f, tile=tile)
    gpu.update_meshes({NIGHT_BOX: (p1[NIGHT_BOX], None)})
    gpu.set_seed(SEED, 0)
    rgb, grid = gpu.render_restir(None, cam, W, H, f, tile=tile)
    other = restir.Renderer(0)
    try:
        other.set_scene(with_positions(s, p1))
        other.set_seed(SEED, 0)
        rgb2, grid2 = other.render_restir(None, cam, W, H, f, tile=tile)
        same_bits(rgb, rgb2, "tile rgb")
        # the owned rectangle of the returned grid (the ghost ring holds passes' intermediate state, which no caller reads)
        own = (slice(None), slice(tile.y0 - tile.gy0, tile.y0 - tile.gy0 + tile.height),
               slice(tile.x0 - tile.gx0, tile.x0 - tile.gx0 + tile.width))
        for a, b in zip(grid.download(), grid2.download()):
            same_bits(a[own], b[own], "tile grid")
    finally:
        other.close()
    want, _, _ = oracle.render_frame(oracle.OracleScene(with_positions(s, p1)), cam, f, W, H, SEED, 0)
    r0 = H - (tile.y0 + tile.height)
    assert_bits(rgb, np.ascontiguousarray(want[r0:r0 + tile.height, tile.x0:tile.x0 + tile.width]), "tile rgb against the oracle")
    assert np.count_nonzero((rgb.view(np.uint32) != before.view(np.uint32)).any(axis=2)) >= 16


# ---- lights ------------------------------------------------------------------------------------------------------
def moved_lights(lights, k):
    """Every light shifted by k * (0.11, -0.07, 0.05) and its colours scaled by 1 - 0.15 k (float32)."""
    out = []
    d = np.array([0.11, -0.07, 0.05], f32) * f32(k)
    g = f32(1.0) - f32(0.15) * f32(k)
    for l in lights:
        m = _abi.Light.from_buffer_copy(l)
        m.p0[:] = (np.asarray(list(l.p0), f32) + d).tolist()
        for c in ("c0", "c1", "c2", "c3"):
            getattr(m, c)[:] = (np.asarray(list(getattr(l, c)), f32) * g).tolist()
        out.append(m)
    return out


@pytest.mark.parametrize("N", [1, 2])
def test_lights_move_under_a_still_camera(gpu, oracle, N):
    s = the_scene(NIGHT)
    cam = camera_of(NIGHT, W, H)
    f = feats(N, 1, temporal=1)
    gpu.set_scene(s)
    gpu.set_seed(SEED, 0)
    prev, oprev, last = None, None, None
    for frame in range(4):
        lights = moved_lights(s.lights, frame)
        if frame:
            gpu.set_lights(lights)
        rgb, grid = gpu.render_restir(prev, cam, W, H, f)
        want, res, _ = oracle.render_frame(oracle.OracleScene(with_positions(s, positions_of(s), lights=lights)), cam, f, W, H,
                                           SEED, frame, prev=oprev)
        assert_bits(rgb, want, f"lights N={N} frame {frame} rgb")
        assert_grid(grid, res, f"lights N={N} frame {frame}")
        assert gpu.gbuf_reuses() == frame, f"frame {frame}: {gpu.gbuf_reuses()} reusing frames"   # the geometry stands
        if last is not None:
            assert np.count_nonzero((want.view(np.uint32) != last.view(np.uint32)).any(axis=2)) >= 16
        prev, oprev, last = grid, res, want


def light_lists():
    night, cornell = the_scene(NIGHT), the_scene(CORNELL)
    odd = _abi.Light.from_buffer_copy(cornell.lights[700])   # one light with another first edge: parallelograms, no grid
    odd.p1[:] = (np.asarray(list(odd.p1), f32) * f32(0.5)).tolist()
    return {"128_to_126": (NIGHT, night.lights[:126]), "points_to_mixed17": (NIGHT, _mixed_lights(17)),
            "grid_to_non_grid": (CORNELL, cornell.lights[:700] + [odd] + cornell.lights[701:]),
            "to_none": (NIGHT, [])}


INFO_FIELDS = [n for n, _ in _abi.SceneInfo._fields_]


@pytest.mark.parametrize("case", ["128_to_126", "points_to_mixed17", "grid_to_non_grid", "to_none"])
def test_another_light_list(gpu, oracle, case):
    from romis_amd import restir
    name, lights = light_lists()[case]
    s = the_scene(name)
    cam = camera_of(name, W, H)
    f = feats(1, 2)
    gpu.set_scene(s)
    gpu.set_seed(SEED, 0)
    gpu.render_restir(None, cam, W, H, f)
    gpu.set_lights(lights)
    s2 = with_positions(s, positions_of(s), lights=lights)
    other = restir.Renderer(0)
    try:
        other.set_scene(s2)
        want_info = {k: getattr(other.scene_info(), k) for k in INFO_FIELDS}
    finally:
        other.close()
    info = {k: getattr(gpu.scene_info(), k) for k in INFO_FIELDS}
    assert info == want_info
    assert info["num_lights"] == len(lights)
    if case == "128_to_126":
        assert info["light_scale"] == 0.0
    if case == "grid_to_non_grid":
        assert info["lights_grid"] == 0 and info["lights_pgram"] == 1
    if case == "points_to_mixed17":
        assert info["light_types"] == 7
    osc = oracle.OracleScene(s2)
    for frame in (1, 2):
        rgb, grid = gpu.render_restir(None, cam, W, H, f)
        want, res, _ = oracle.render_frame(osc, cam, f, W, H, SEED, frame)
        assert_bits(rgb, want, f"{case} frame {frame} rgb")
        assert_grid(grid, res, f"{case} frame {frame}")
    assert gpu.gbuf_reuses() >= 1   # the kept G-buffer outlived the light list wherever the new frames can read it


# ---- kernel choice -----------------------------------------------------------------------------------------------
def test_handles_survive_a_geometry_update_and_not_a_light_update(gpu, oracle):
    """N = 1, two biased passes, 128 point lights, temporal reuse: with the predecessor's frame handles the passes read
    handles and the last one shades (no RESTIR_K_FINAL launch); without them they read the reservoir planes and final
    shading is a launch of its own."""
    s = the_scene(NIGHT)
    cam = camera_of(NIGHT, W, H)
    f = feats(1, 2, temporal=1)
    gpu.set_scene(s)
    gpu.set_seed(SEED, 0)
    p = positions_of(s)
    lights = s.lights
    finals, prev, oprev = [], None, None
    for frame, event in enumerate(["none", "none", "geometry", "lights", "none"]):
        if event == "geometry":
            p[NIGHT_BOX] = (p[NIGHT_BOX] + np.array([0.0, 0.5, 0.0], f32)).astype(f32)
            gpu.update_meshes({NIGHT_BOX: (p[NIGHT_BOX], None)})
        if event == "lights":
            lights = moved_lights(s.lights, 1)
            gpu.set_lights(lights)
        with counted(gpu) as n:
            rgb, grid = gpu.render_restir(prev, cam, W, H, f)
        want, res, _ = oracle.render_frame(oracle.OracleScene(with_positions(s, p, lights=lights)), cam, f, W, H, SEED, frame,
                                           prev=oprev)
        assert_bits(rgb, want, f"frame {frame} ({event}) rgb")
        assert_grid(grid, res, f"frame {frame} ({event})")
        finals.append(n["final"])
        prev, oprev = grid, res
    # (the frame after that one has a predecessor without frame handles -- only a handle frame writes them -- so what it
    # takes is not asserted; its image and grid are, above)
    assert finals[:4] == [0, 0, 0, 1], f"RESTIR_K_FINAL launches per frame: {finals}"


# ---- errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_as_it_was(gpu, oracle):
    lib = gpu.lib
    FP = C.POINTER(C.c_float)
    s = the_scene(NIGHT)
    pos = positions_of(s)

    def update(*ups):
        arr = (_abi.MeshUpdate * max(1, len(ups)))()
        for i, (m, p, nv) in enumerate(ups):
            arr[i].mesh, arr[i].num_vertices = m, nv
            arr[i].positions = p.ctypes.data_as(FP) if p is not None else None
        return lib.restir_update_meshes(gpu.ctx, arr, len(ups))

    INVALID, STATE = 1, 4
    assert update((0, pos[0], len(pos[0]))) == STATE
    assert lib.restir_set_lights(gpu.ctx, None, 0) == STATE
    assert lib.restir_debug_scene_download(gpu.ctx, *([None] * 8)) == STATE
    assert lib.restir_update_meshes(None, None, 0) == INVALID and lib.restir_set_lights(None, None, 0) == INVALID

    gpu.set_scene(s)
    upload = gpu.debug_scene()
    bad = pos[NIGHT_BOX].copy()
    bad[3, 1] = np.inf
    nan = pos[NIGHT_BOX].copy()
    nan[0, 0] = np.nan
    moved = (pos[NIGHT_BOX] + f32(1.0)).astype(f32)
    assert update((len(pos), pos[0], len(pos[0]))) == INVALID                       # mesh index
    assert update((NIGHT_BOX, moved, len(moved) - 1)) == INVALID                    # vertex count
    assert update((NIGHT_BOX, None, len(moved))) == INVALID                         # null positions
    assert update((NIGHT_BOX, moved, len(moved)), (NIGHT_BOX, moved, len(moved))) == INVALID   # named twice
    assert update((0, pos[0], len(pos[0])), (NIGHT_BOX, bad, len(bad))) == INVALID  # not finite, after a valid entry
    assert update((NIGHT_BOX, nan, len(nan))) == INVALID
    assert b"non-finite" in lib.restir_last_error()
    assert lib.restir_update_meshes(gpu.ctx, None, 1) == INVALID
    badlight = _abi.Light.from_buffer_copy(s.lights[0])
    badlight.type = 3
    assert lib.restir_set_lights(gpu.ctx, (_abi.Light * 1)(badlight), 1) == INVALID
    assert lib.restir_set_lights(gpu.ctx, None, 2) == INVALID
    for key, a in upload.items():   # nothing moved
        same_bits(gpu.debug_scene()[key], a, f"after the refused calls: {key}")

    cam, f = camera_of(NIGHT, W, H), feats(1, 2)
    osc = oracle.OracleScene(s)
    gpu.set_seed(SEED, 0)
    for frame in range(2):
        rgb, grid = gpu.render_restir(None, cam, W, H, f)
        want, res, _ = oracle.render_frame(osc, cam, f, W, H, SEED, frame)
        assert_bits(rgb, want, f"after the refused calls: frame {frame} rgb")
        assert_grid(grid, res, f"after the refused calls: frame {frame}")
        if frame == 0:
            assert lib.restir_update_meshes(gpu.ctx, None, 0) == 0   # count 0: a no-op that keeps the kept G-buffer
    assert gpu.gbuf_reuses() == 1
