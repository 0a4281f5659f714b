"""Rays the other GPU tests never trace: axis-parallel, tied, grazing and degenerate ones.

The oracle finds hits by brute force over every triangle; the device prunes -- the threaded float BVH (box_hit over
safe_inv's 1e-30 stand-in for a zero direction component, widen(t_best)), the 16-byte quantized nodes (occluded_q), the
per-tile candidate lists (tile_triangles) and the binned shadow rays (target_bin).  The other files' five cameras have
generic Euler angles, stand outside the geometry and hit faces well away from an edge, and their shadow rays run from a
surface to a light in free space.  Here:

A  cameras (all through scene.make_camera) whose rays have exact zero direction components, components below 1e-6,
   ties between triangles at the closest t, an origin inside the mesh or in a face's plane, a 170 and a 0.05 degree
   field of view, 3-pixel-wide frames, and no hit at all;
B  shadow rays designed through uploaded reservoirs (W = 1, M = 1, colour 1), the sample position y computed in numpy
   float32 from the pixel's own P so that the intended zero or equality is exact: plumb (two exact zeros), coincident
   (y = P: a NaN direction), ending on a surface, at a triangle's vertex and inside it, a subnormal component (1 / d
   infinite, NaN slabs), 5e-4 and 1e19 long;
C  bvh.max_leaf 1, 3, 4, 15, 16, 17: odd leaves through the two-at-a-time loops, and the quantized nodes' limit.

Every test first asserts, from the oracle's G-buffer or numpy float32 arithmetic on the camera frame, that its rays are
the ones it was written for; then every word of n_t, p_mat, reservoirs, RGB and returned grids equals the oracle's --
non-finite words included, no tolerance, no pixel left out.  Oracle results are computed once per module and shared.

Counts the property assertions see (oracle only).  Axis views: 95 rays with a zero component (32 with d.x == 0, 64 with
d.y == 0); ties 13 (cube from outside) and 45 (from its centre).  Designed rays, (visible, occluded) pixels at N = 1:

               cube (169 px)  cube_inside (2048)  night (1887)   monkey (2356)
  plumb        88, 81         1024, 1024          943, 944       1178, 1178
  surface      168, 1         1057, 991           817, 1070      1126, 1230
  vertex       84, 85         1024, 1024          713, 1174      897, 1459
  subnormal    6, 7 (13 px)   16, 16 (32 px)      no P.x = +-0   no P.x = +-0
  near         169, 0         2048, 0             1878, 9        2323, 33
  far          84, 85         1024, 1024          898, 989       1178, 1178

(coincident rays have a NaN direction and hit nothing: all visible.)  RIS towards 254 plumb lights: 21650 / 8352 / 254
(pixel, light) pairs with an exact zero component on the cube / nightclub / Monkey.

Why a NaN ray is safe to trace: in occluded, occluded_q and closest the node index only ever moves to i + 1 or to the
node's miss link, and every miss link is greater than its node's index (tests/test_bvh_invariants.py), so a ray whose
every comparison is false walks at most num_nodes nodes and ends; target_bin's fminf(fmaxf(t, 0), cells - 1) turns a
NaN coordinate into cell 0, so its bin is < 256.
"""
import numpy as np
import pytest

from romis_amd import _abi, scene
from test_gpu_parity import assert_bits, key, origin
from test_gpu_scene_shapes import (CORNELL, H, NIGHT, W, W2, H2, assert_over_budget, assert_unfused, camera, check_frame,
                                   check_reservoirs, counted, feats, frames_of, frozen, gpu, inputs, knobs, oscene,
                                   shape_scene, upload_inputs, use_scene)

pytestmark = pytest.mark.gpu

f32 = np.float32
CUBE, MONKEY = "CubeTextured", "Monkey"
WA, HA = 64, 32   # even: pixel (W / 2, H / 2) has nx = ny = 0
LDS_TRIS = 256    # kernels.hip kTlMaxTris: the fused kernel builds candidate lists up to this many triangles


def centre(name):
    """The centre of the mesh bounds, as Python floats (a camera's look_at)."""
    pos = np.concatenate([np.asarray(m.positions, f32) for m in shape_scene(name).meshes])
    return tuple(float(v) for v in (pos.min(axis=0) + pos.max(axis=0)) * f32(0.5))


AXIS = (50.0, 3.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
NIGHT_LOOK, NIGHT_ROT = (2.57, 1.23, -1.35), (10.3, 30.0, 0.0)


def views():
    """id: (scene, (fov, dist, look_at, rot), w, h, class)."""
    inside = (35.0, 140.0, 10.0)
    return {
        "axis_cube": (CUBE, AXIS, WA, HA, "axis"),
        "axis_cornell": (CORNELL, AXIS, WA, HA, "axis"),
        "axis_night": (NIGHT, AXIS, WA, HA, "axis"),
        "axis_monkey": (MONKEY, AXIS, WA, HA, "axis"),
        "near_axis_y90": (CUBE, (50.0, 3.0, (0.0, 0.0, 0.0), (0.0, 90.0, 0.0)), WA, HA, "near_axis"),
        "near_axis_xyz": (NIGHT, (50.0, 3.0, (0.0, 0.0, 0.0), (90.0, 180.0, 270.0)), WA, HA, "near_axis"),
        "inside_cube": (CUBE, (120.0, 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), WA, HA, "inside"),
        "inside_night": (NIGHT, (90.0, 0.05, centre(NIGHT), inside), W, H, "inside"),
        "inside_monkey": (MONKEY, (90.0, 0.05, centre(MONKEY), inside), W, H, "inside"),
        # the origin (0, 0, -0.5) lies in the plane of the face z = -0.5 and looks into the cube: that face's triangles
        # are met at t = 0 or its rounding error, on the boundary of t > 0.  (From (0, 0, 0.5) under rot (0, 90, 0) the
        # origin rounds to 0.49999997, not the face's 0.5, and a camera in a face's plane that looks along it loses the
        # half of its rays that leave through the face.)
        "grazing_cube": (CUBE, (60.0, 0.5, (0.0, 0.0, 0.0), (0.0, 0.0, 30.0)), W2, H2, "grazing"),
        "wide_night": (NIGHT, (170.0, 0.6, NIGHT_LOOK, (-95.0, 400.0, 12.5)), W, H, "wide"),
        "wide_cornell": (CORNELL, (170.0, 0.6, (0.0, 0.0, 0.0), (-95.0, 400.0, 12.5)), W2, H2, "wide"),
        "narrow_night": (NIGHT, (0.05, 25.0, NIGHT_LOOK, NIGHT_ROT), W, H, "narrow"),
        "narrow_cornell": (CORNELL, (0.05, 3.0, (0.0, 0.0, 0.0), (20.0, 20.0, 0.0)), W2, H2, "narrow"),
        "sliver_tall": (NIGHT, (30.0, 25.0, NIGHT_LOOK, NIGHT_ROT), 3, 97, "sliver"),
        "sliver_flat": (NIGHT, (30.0, 25.0, NIGHT_LOOK, NIGHT_ROT), 97, 3, "sliver"),
        "miss_night": (NIGHT, (30.0, 3000.0, NIGHT_LOOK, NIGHT_ROT), W2, H2, "miss"),
        "miss_monkey": (MONKEY, (30.0, 3000.0, NIGHT_LOOK, NIGHT_ROT), W2, H2, "miss"),
    }


VIEWS = views()
_rays, _uv = {}, {}


def triangles(name):
    """[T][3][3] float32 vertex positions, mesh order."""
    return np.concatenate([np.asarray(m.positions, f32)[np.asarray(m.triangles, np.int64)] for m in shape_scene(name).meshes])


def view_inputs(oracle, v):
    """inputs() of a view; a textured scene's texCoord plane is kept per view and bound again (the oracle scene holds
    the plane of the last G-buffer it traced)."""
    name, cam, w, h, _ = VIEWS[v]
    got = inputs(oracle, name, cam, w, h)
    osc = got[0]
    if osc.num_textures:
        if v not in _uv:
            _uv[v] = frozen(osc.uv.copy())[0]
        osc.bind_uv(_uv[v])
    return got


def view_rays(oracle, v):
    """(ties [h][w], directions [h][w][3], camera frame) of a view's primary rays, from the oracle."""
    if v not in _rays:
        name, cam, w, h, _ = VIEWS[v]
        c = camera(name, cam, w, h)
        ties, dirs = oracle.primary_ties(oscene(oracle, name), c, w, h)
        _rays[v] = frozen(ties.reshape(h, w), dirs.reshape(h, w, 3)) + (oracle.camera_frame(c),)
    return _rays[v]


def tile_list_sizes(name, cf, w, h):
    """tile_triangles in numpy float32: per 32 x 8 tile the number of triangles not wholly beyond one of the four planes
    of the tile's ray pyramid (widened by two pixels, margin 1e-5)."""
    tri = triangles(name)
    qx, qy, qz, qw = (f32(v) for v in cf.quat)
    one, two = f32(1.0), f32(2.0)
    rx = np.array([one - two * (qy * qy + qz * qz), two * (qx * qy + qw * qz), two * (qx * qz - qw * qy)], f32)
    ry = np.array([two * (qx * qy - qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz + qw * qx)], f32)
    rz = np.array([two * (qx * qz + qw * qy), two * (qy * qz - qw * qx), one - two * (qx * qx + qy * qy)], f32)
    p = tri - np.asarray(list(cf.origin), f32)
    l1 = np.abs(p).sum(axis=-1)
    hw, hh = f32(cf.half_w), f32(cf.half_h)
    sizes = []
    for y0 in range(0, h, 8):
        for x0 in range(0, w, 32):
            x1, y1 = min(x0 + 32, w) - 1, min(y0 + 8, h) - 1
            nxl, nxh = f32(x0 - 2) / f32(w) * two - one, f32(x1 + 2) / f32(w) * two - one
            nyl, nyh = f32(y0 - 2) / f32(h) * two - one, f32(y1 + 2) / f32(h) * two - one
            a0, a1 = min(-nxl * hw, -nxh * hw), max(-nxl * hw, -nxh * hw)
            b0, b1 = min(nyl * hh, nyh * hh), max(nyl * hh, nyh * hh)
            out = np.zeros(len(tri), bool)
            for pn in (rx - rz * a0, rz * a1 - rx, ry - rz * b0, rz * b1 - ry):
                m = f32(1e-5) * np.abs(pn).sum()
                out |= ((p @ pn) < -m * l1).all(axis=-1)
            sizes.append(int((~out).sum()))
    return sizes


def ray_facts(oracle, v):
    """What a view's class asserts, from the oracle and the camera frame alone."""
    name, cam, w, h, _ = VIEWS[v]
    ties, dirs, cf = view_rays(oracle, v)
    _, _, n_t, p_mat = view_inputs(oracle, v)
    hit = (n_t[:, 3] < 1e30).reshape(h, w)
    small = (dirs != 0) & (np.abs(dirs) < 1e-6)
    tri = triangles(name)
    o = np.asarray(list(cf.origin), f32)
    # the camera plane: through the origin, normal = the view axis R (0, 0, 1) (the centre pixel's direction at even sizes)
    qx, qy, qz, qw = (f32(x) for x in cf.quat)
    axis = np.array([2 * (qx * qz + qw * qy), 2 * (qy * qz - qw * qx), 1 - 2 * (qx * qx + qy * qy)], f32)
    side = (tri - o) @ axis
    return dict(hit_share=float(hit.mean()), zero_rays=int((dirs == 0).any(axis=-1).sum()),
                zero_x=int((dirs[..., 0] == 0).sum()), zero_y=int((dirs[..., 1] == 0).sum()), small=int(small.any(axis=-1).sum()),
                tied=int((ties > 1).sum()), straddle=int(((side > 0).any(axis=1) & (side < 0).any(axis=1)).sum()),
                origin_on_vertex_coord=bool((tri.reshape(-1, 3).view(np.uint32) == o.view(np.uint32)).any()),
                list_max=max(tile_list_sizes(name, cf, w, h)), tris=len(tri))


# ---- B. designed shadow rays: the oracle's side -------------------------------------------------------------
# view: (scene, camera, w, h); the G-buffers of the nightclub and Monkey are the ones test_gpu_scene_shapes shares
RAY_VIEWS = {"cube": "axis_cube", "cube_inside": "inside_cube", "night": (NIGHT, None, W, H), "monkey": (MONKEY, "framed", W, H)}
AXES = np.eye(3, dtype=f32)
DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1],
                 [3, 1, 2], [-2, 3, 1], [1, -2, -3], [-1, -3, 2]], f32)
DIRS /= np.sqrt((DIRS * DIRS).sum(axis=1, keepdims=True)).astype(f32)
_designed = {}


def ray_view(oracle, rv):
    """(scene name, oracle scene, camera, w, h, n_t, p_mat) of a designed-ray view."""
    spec = RAY_VIEWS[rv]
    if isinstance(spec, str):
        name, cam, w, h, _ = VIEWS[spec]
        osc, c, n_t, p_mat = view_inputs(oracle, spec)
    else:
        name, cam, w, h = spec
        osc, c, n_t, p_mat = inputs(oracle, name, cam, w, h)
    return name, cam, osc, c, w, h, n_t, p_mat


def family_variants(family, name, P, hit):
    """[variant][pixel][3] float32: the candidate sample positions of every hit pixel (rows of P[hit]), each computed in
    float32 from the pixel's own P.  Pixels a family does not apply to hold NaN in every variant."""
    Ph = P[hit]
    n = len(Ph)
    scale = f32(np.abs(triangles(name)).max())
    if family == "plumb":      # P + k e_axis: two exact zeros in y - P
        ks = [f32(s * m) * scale for m in (2.0, 0.6, 0.15, 0.03) for s in (1, -1)]
        return np.stack([Ph + k * AXES[a] for k in ks for a in range(3)])
    if family == "coincident":
        return Ph[None].copy()
    if family == "surface":    # another pixel's P: the ray ends on a surface
        return np.stack([Ph[(np.arange(n) + s) % n] for s in (1, 5, 17, 97, n // 2, n // 3 + 1)])
    if family == "vertex":     # a triangle's v0 (u = v = 0) and v0 + (e1 + e2) / 4
        tri = triangles(name)
        out = []
        for j in range(6):
            t = tri[(np.arange(n) * 7 + j * 13) % len(tri)]
            out += [t[:, 0], t[:, 0] + ((t[:, 1] - t[:, 0]) + (t[:, 2] - t[:, 0])) / f32(4)]
        return np.stack(out).astype(f32)
    if family == "subnormal":  # P + (1e-40, k, 0) where P.x is +-0: 1 / d.x is infinite
        ks = [f32(s * m) * scale for m in (4.0, 1.4, 0.6, 0.1) for s in (1, -1)]
        out = np.stack([Ph + np.array([1e-40, k, 0], f32) for k in ks])
        out[:, Ph[:, 0] != 0] = np.nan
        return out
    if family == "near":       # 5e-4 long: P2 = P + 1e-3 dir lies beyond y; occluded only next to a crease: many directions
        more = np.random.default_rng(5).normal(size=(114, 3)).astype(f32)
        more /= np.sqrt((more * more).sum(axis=1, keepdims=True)).astype(f32)
        return np.stack([Ph + f32(5e-4) * d for d in np.concatenate([DIRS, more])])
    if family == "far":
        return np.stack([Ph + f32(1e19) * d for d in DIRS])
    raise KeyError(family)


FAMILIES = ["plumb", "coincident", "surface", "vertex", "subnormal", "near", "far"]


def designed(oracle, rv, family):
    """Reservoirs (res_a, res_b) for N = 2 whose hit pixels hold a designed sample (W = 1, M = 1, colour 1); N = 1 uses
    sub-reservoir 0.  The other pixels keep the oracle's RIS result.  Per pixel and sub-reservoir the variant is chosen
    here, from the oracle's visible() alone, so that occluded and visible rays alternate wherever a pixel's variants offer
    both: pixel i of sub-reservoir j wants outcome (i + j) % 2.  Returns (res_a, res_b, chosen y [2][hits][3],
    visible [2][hits], applies [hits])."""
    k = (rv, family)
    if k in _designed:
        return _designed[k]
    name, cam, osc, c, w, h, n_t, p_mat = ray_view(oracle, rv)
    P = np.ascontiguousarray(p_mat[:, :3])
    hit = n_t[:, 3] < 1e30
    Ph = P[hit]
    var = family_variants(family, name, P, hit)
    applies = ~np.isnan(var).all(axis=(0, 2)) if family == "subnormal" else np.ones(len(Ph), bool)
    vis = np.stack([oracle.visible(osc, Ph, np.where(np.isnan(v), Ph, v).astype(f32)) for v in var])   # [variant][pixel]
    rows = np.flatnonzero(applies)
    order = np.zeros(len(Ph), np.int64)
    order[rows] = np.arange(len(rows))
    ys, seen = [], []
    for j in range(2):
        want = ((order + j) % 2).astype(bool)                      # True: visible
        rot = (np.arange(len(var))[:, None] + j) % len(var)         # sub-reservoir 1 starts one variant later
        ok = vis[rot[:, 0]] == want[None]
        pick = rot[np.where(ok.any(axis=0), ok.argmax(axis=0), 0), 0]
        ys.append(var[pick, np.arange(len(Ph))])
        seen.append(vis[pick, np.arange(len(Ph))])
    f = feats(2, enable_texture_mapping=0)
    a, b, _ = (x.copy() for x in _ris_base(oracle, rv, f))
    put = np.flatnonzero(hit)[applies]
    for j in range(2):
        a[j, put, :3] = ys[j][applies]
        a[j, put, 3] = 1.0
        b[j, put, :3] = 1.0
        b[j, put, 3] = np.array([1], np.uint32).view(f32)[0]
    _designed[k] = frozen(a, b, np.stack(ys), np.stack(seen), applies)
    return _designed[k]


_base = {}


def _ris_base(oracle, rv, f):
    if rv not in _base:
        name, cam, osc, c, w, h, n_t, p_mat = ray_view(oracle, rv)
        _base[rv] = frozen(*oracle.ris(osc, f, key(_abi.RESTIR_STAGE_RIS), origin(oracle, c), w, h, n_t, p_mat))
    return _base[rv]


def outcome_counts(oracle, rv, family, N):
    """(visible, occluded) pixels of the family's rays in sub-reservoirs 0 .. N - 1 (a pixel counts once per outcome)."""
    _, _, _, seen, applies = designed(oracle, rv, family)
    s = seen[:N][:, applies]
    return int(s.any(axis=0).sum()), int((~s).any(axis=0).sum())


# per view, the designed families whose rays the oracle finds both visible and occluded on >= 16 pixels (N = 1).  Not
# there: "surface" and "near" from outside the convex cube (no second surface in the way; 1 and 0 occluded pixels),
# "near" inside the cube and in the nightclub (a 5e-4 ray is stopped only within 1.5e-3 of a crease: 0 and 9 pixels), and
# "subnormal" on the axis view, whose centre column holds 13 hit pixels -- each family meets the condition on the other
# views it runs on, and over all its views together.
BOTH_OUTCOMES = {"cube": ["plumb", "vertex", "far"], "cube_inside": ["plumb", "surface", "vertex", "subnormal", "far"],
                 "night": ["plumb", "surface", "vertex", "far"], "monkey": ["plumb", "surface", "vertex", "near", "far"]}
FAMILY_VIEWS = {f: [rv for rv in RAY_VIEWS if f != "subnormal" or rv.startswith("cube")] for f in FAMILIES}


def assert_family_reaches_its_rays(oracle, rv, family):
    """From numpy and the oracle alone: the exact zeros / equalities the family exists for, and both outcomes."""
    name, cam, osc, c, w, h, n_t, p_mat = ray_view(oracle, rv)
    a, b, ys, seen, applies = designed(oracle, rv, family)
    Ph = p_mat[n_t[:, 3] < 1e30, :3]
    d = (ys - Ph[None])[:, applies]
    n = int(applies.sum())
    if family == "plumb":
        assert ((d == 0).sum(axis=-1) == 2).all() and n >= 160
    elif family == "coincident":
        assert (d == 0).all()
    elif family == "surface":
        own = {r.tobytes() for r in Ph}
        assert all(r.tobytes() in own for r in ys[0]) and (d != 0).any(axis=-1).mean() > 0.99
    elif family == "vertex":
        v0 = {r.tobytes() for r in triangles(name)[:, 0]}
        assert sum(r.tobytes() in v0 for r in ys[0]) >= n // 4
    elif family == "subnormal":
        assert n >= 13 and (Ph[applies][:, 0] == 0).all()
        assert (np.abs(d[..., 0]) < np.finfo(f32).tiny).all() and (d[..., 0] > 0).all() and (d[..., 1] != 0).all() and (d[..., 2] == 0).all()
    elif family == "near":
        assert (np.abs(d).max(axis=-1) <= 5.1e-4).all()      # (P + 5e-4 dir) - P, rounded at P's magnitude
    elif family == "far":
        assert (np.abs(d).max(axis=-1) >= 2e18).all()
    counts = {N: outcome_counts(oracle, rv, family, N) for N in (1, 2)}
    print(f"rays {rv} {family}: pixels {n}, (visible, occluded) N=1 {counts[1]} N=2 {counts[2]}")
    if family in BOTH_OUTCOMES[rv]:
        assert min(counts[1]) >= 16, f"{rv} {family}: visible / occluded pixels {counts[1]}"
    if family != "coincident":
        total = np.sum([outcome_counts(oracle, v, family, 1) for v in FAMILY_VIEWS[family]], axis=0)
        assert total.min() >= 16, f"{family}: visible / occluded pixels over its views {total.tolist()}"
    return counts


# ---- the device's side --------------------------------------------------------------------------------------
def put_scene(gpu, name):
    s, info = use_scene(gpu, name)
    if name == MONKEY:
        assert_over_budget(info)
    else:
        assert info.bvh_lds_bytes <= 65536 and info.nodes_q_ok == 1
    return info


def final_against_oracle(gpu, oracle, rv, res, N, what, tunes):
    """stage_final over the view's G-buffer and `res` under each knob set of `tunes`, against oracle.final."""
    name, cam, osc, c, w, h, n_t, p_mat = ray_view(oracle, rv)
    f = feats(N, enable_texture_mapping=0)
    res = tuple(np.ascontiguousarray(x[:N]) for x in res)
    want = oracle.final(osc, f, origin(oracle, c), w, h, n_t, p_mat, res)
    for tune in tunes:
        with knobs(gpu, **tune):
            upload_inputs(gpu, oracle, name, cam, N, w, h)
            gpu.upload(_abi.BUF_RES_A, res[0])
            gpu.upload(_abi.BUF_RES_B, res[1])
            gpu.stage_final(c, f)
            assert_bits(gpu.download(_abi.BUF_RGB), want, f"{what} N={N} {tune} rgb")
    return want


FINAL_TUNES = [dict(final_qbvh=q, final_sort=s, final_lds=l) for q in (0, 1) for s in (0, 1) for l in (0, 1)]


# ---- A. cameras ---------------------------------------------------------------------------------------------
def assert_view_class(oracle, v):
    """The property a camera class exists for, before anything is compared."""
    name, cam, w, h, cls = VIEWS[v]
    ft = ray_facts(oracle, v)
    print(f"view {v} ({cls}, {name} {w}x{h}): {ft}")
    _, dirs, cf = view_rays(oracle, v)
    _, _, n_t, p_mat = view_inputs(oracle, v)
    if cls == "axis":
        assert (w, h) == (WA, HA) and ft["zero_rays"] == 95 and ft["zero_x"] == 32 and ft["zero_y"] == 64
        assert (dirs[:, w // 2, 0] == 0).all() and (dirs[h // 2, :, 1] == 0).all()
        if name == CUBE:
            col = np.arange(h) * w + w // 2
            on = n_t[col, 3] < 1e30
            assert on.sum() >= 8 and (p_mat[col[on], 0].view(np.uint32) == np.array(cf.origin[0], f32).view(np.uint32)).all()
            assert ft["tied"] == 13
    elif cls == "near_axis":
        assert ft["small"] > 0
    elif cls == "inside":
        assert ft["straddle"] > 0
        lo, hi = (triangles(name).reshape(-1, 3).min(axis=0), triangles(name).reshape(-1, 3).max(axis=0))
        o = np.asarray(list(cf.origin), f32)
        assert ((o > lo) & (o < hi)).all()
        if name == CUBE:
            assert ft["hit_share"] == 1.0 and ft["tied"] == 45
    elif cls == "grazing":
        assert ft["origin_on_vertex_coord"] and ft["hit_share"] > 0.9
    elif cls == "wide":
        assert ft["hit_share"] > 0.05
    elif cls == "narrow":
        assert ft["hit_share"] == 1.0 and ft["list_max"] < ft["tris"] <= LDS_TRIS
    elif cls == "sliver":
        assert ft["hit_share"] > 0 and min(w, h) == 3
    elif cls == "miss":
        assert ft["hit_share"] == 0.0
    return ft


@pytest.mark.parametrize("v", sorted(VIEWS))
def test_view_primary(gpu, oracle, v):
    """k_primary_lds / k_primary (Monkey: the global BVH either way) against the oracle's G-buffer."""
    name, cam, w, h, _ = VIEWS[v]
    assert_view_class(oracle, v)
    put_scene(gpu, name)
    osc, c, n_t, p_mat = view_inputs(oracle, v)
    for lds in (1, 0):
        with knobs(gpu, primary_lds=lds):
            gpu.stage_configure(w, h, 1)
            gpu.stage_primary(c)
            assert_bits(gpu.download(_abi.BUF_GBUF_N_T), n_t, f"{v} lds={lds} n_t")
            assert_bits(gpu.download(_abi.BUF_GBUF_P_MAT), p_mat, f"{v} lds={lds} p_mat")
            if osc.num_textures:
                assert_bits(gpu.download(_abi.BUF_GBUF_UV), _uv[v], f"{v} lds={lds} texCoord")


@pytest.mark.parametrize("v", sorted(VIEWS))
def test_view_frames(gpu, oracle, v):
    """restir_render: primary.tl = 1 / 0 (the fused kernel's candidate lists against its BVH walk), N = 1 / 2, one and
    two passes, each frame traced (a knob set drops the kept G-buffer) and then rendered again from the kept G-buffer;
    one unbiased frame with visibility reuse."""
    name, cam, w, h, cls = VIEWS[v]
    assert_view_class(oracle, v)
    fused = name != MONKEY
    put_scene(gpu, name)
    seen = {}
    for N, passes, unbiased, vis in [(1, 1, 0, 0), (1, 2, 0, 0), (2, 1, 0, 0), (2, 2, 0, 0), (1, 1, 1, 1)]:
        f = feats(N, passes, unbiased, vis)
        for tl in (1, 0):
            what = f"{v} N={N} passes={passes} unbiased={unbiased} tl={tl}"
            with knobs(gpu, primary_tl=tl):
                with counted(gpu) as n:
                    before = gpu.gbuf_reuses()
                    check_frame(gpu, oracle, name, cam, f, what, w, h)
                    reused = gpu.gbuf_reuses() - before
            if fused:
                assert n["primary_ris"] == 2 and n["primary"] == 0 and n["ris"] == 0, f"{what}: launches {n}"
                assert reused == 1, f"{what}: {reused} of the two frames read the kept G-buffer"
            else:
                assert_unfused(n, what)
                assert reused == 0
            seen[(N, passes, unbiased)] = {k_: n_ for k_, n_ in n.items() if n_}
    print(f"launches {v}: {seen}")
    if cls == "miss":
        want = frames_of(oracle, name, cam, feats(1, 2), w, h)[0][0]
        assert not want.view(np.uint32).any(), "an all-miss image is +0"


# ---- B. designed shadow rays --------------------------------------------------------------------------------
RAY_CASES = [(rv, f) for f in FAMILIES for rv in FAMILY_VIEWS[f]]


@pytest.mark.parametrize("rv,family", RAY_CASES)
def test_designed_rays_final(gpu, oracle, rv, family):
    """stage_final: k_final / k_final_lds / k_final_n{1,2}_sorted[_q] (Monkey: the global BVH whatever the knobs say)."""
    assert_family_reaches_its_rays(oracle, rv, family)
    put_scene(gpu, ray_view(oracle, rv)[0])
    a, b = designed(oracle, rv, family)[:2]
    for N in (1, 2):
        final_against_oracle(gpu, oracle, rv, (a, b), N, f"{rv} {family}", FINAL_TUNES)


@pytest.mark.parametrize("rv,family", RAY_CASES)
def test_designed_rays_unbiased_spatial(gpu, oracle, rv, family):
    """One unbiased pass with visibility reuse over the designed reservoirs: k_spatial1u_vis (N = 1, the BVH in LDS) and
    the general unbiased kernel (N = 2; Monkey: shadow rays over the global BVH)."""
    assert_family_reaches_its_rays(oracle, rv, family)
    name, cam, osc, c, w, h, n_t, p_mat = ray_view(oracle, rv)
    put_scene(gpu, name)
    a, b = designed(oracle, rv, family)[:2]
    kp = key(_abi.RESTIR_STAGE_SPATIAL, 0)
    for N in (1, 2):
        f = feats(N, 1, 1, 1, enable_texture_mapping=0)
        res = (np.ascontiguousarray(a[:N]), np.ascontiguousarray(b[:N]))
        upload_inputs(gpu, oracle, name, cam, N, w, h)
        gpu.upload(_abi.BUF_RES_A, res[0])
        gpu.upload(_abi.BUF_RES_B, res[1])
        gpu.stage_spatial(c, f, kp)
        check_reservoirs(gpu, oracle.spatial_pass(osc, f, kp, origin(oracle, c), w, h, n_t, p_mat, res), f"{rv} {family} N={N}")


@pytest.mark.parametrize("rv", ["cube", "night", "monkey"])
@pytest.mark.parametrize("N", [1, 2])
def test_plumb_point_lights_ris(gpu, oracle, rv, N):
    """RIS with initial-visibility rays towards 254 point lights, each plumb over a distinct pixel's P (two exact zero
    direction components from that pixel, one from every pixel that shares a coordinate with it)."""
    name, cam, _, c, w, h, n_t, p_mat = ray_view(oracle, rv)
    hit = np.flatnonzero(n_t[:, 3] < 1e30)
    pix = hit[(np.arange(254) * len(hit)) // 254]
    assert len(hit) >= 160   # the cube's 169 hit pixels carry two lights each, on different axes
    P = p_mat[:, :3]
    scale = f32(np.abs(triangles(name)).max())
    lights, pos = [], []
    for i, p in enumerate(pix):
        y = P[p] + (f32(0.6) if i & 1 else f32(-0.6)) * scale * AXES[i % 3]
        l = _abi.Light(type=_abi.LIGHT_POINT)
        l.p0[:] = [float(x) for x in y]
        l.c0[:] = [1.0, 1.0, 1.0]
        lights.append(l)
        pos.append(y)
    assert len({y.tobytes() for y in pos}) == 254
    d = np.stack(pos)[None, :, :] - P[hit][:, None, :]
    zero_pairs = int((d == 0).any(axis=-1).sum())
    print(f"ris {rv}: {zero_pairs} (pixel, light) pairs with an exact zero component, {int(((d == 0).sum(axis=-1) == 2).sum())} with two")
    assert zero_pairs >= 254
    sc = scene.Scene(shape_scene(name).meshes, lights, f"{name}_plumb254")
    osc = oracle.OracleScene(sc)
    n_t2, p_mat2 = oracle.gbuffer(osc, c, w, h)     # the same meshes: the same G-buffer (binds this scene's texCoords)
    assert_bits(n_t2, n_t, "n_t")
    assert_bits(p_mat2, p_mat, "p_mat")
    gpu.set_scene(sc)
    info = gpu.scene_info()
    assert info.num_lights == 254 and info.light_types == 1 << _abi.LIGHT_POINT
    f = feats(N, initial_samples_visibility_check=1, enable_texture_mapping=0)
    kr = key(_abi.RESTIR_STAGE_RIS)
    want = oracle.ris(osc, f, kr, origin(oracle, c), w, h, n_t, p_mat)
    dark = int((want[0][0, hit, 3] == 0).sum())
    print(f"ris {rv} N={N}: {dark} of {len(hit)} hit pixels end with W = 0")
    gpu.stage_configure(w, h, N)
    gpu.upload(_abi.BUF_GBUF_N_T, n_t)
    gpu.upload(_abi.BUF_GBUF_P_MAT, p_mat)
    gpu.stage_ris(c, f, kr)
    check_reservoirs(gpu, want, f"{rv} plumb lights N={N}")


# ---- C. leaf sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rv", ["night", "cube"])
def test_leaf_sizes(gpu, oracle, rv):
    """bvh.max_leaf 1, 3, 4, 15, 16, 17: occluded / occluded_q step through a leaf two triangles at a time (k + 1 < cnt),
    and a leaf of 16 does not fit the quantized node's 4-bit count -- the route then takes the float nodes.  The oracle does
    not depend on the leaf size.  (The cube's 12 triangles never fill a leaf of 16: its quantized nodes stay.)"""
    name, cam, osc, c, w, h, n_t, p_mat = ray_view(oracle, rv)
    a, b = designed(oracle, rv, "plumb")[:2]
    assert_family_reaches_its_rays(oracle, rv, "plumb")
    nodes = []
    try:
        for leaf in (1, 3, 4, 15, 16, 17):
            gpu.set_tuning("bvh.max_leaf", leaf)
            _, info = use_scene(gpu, name)
            nodes.append(info.num_nodes)
            want_q = 1 if (leaf < 16 or info.num_tris < 16) else 0
            assert info.nodes_q_ok == want_q, f"{name} max_leaf {leaf}: nodes_q_ok {info.nodes_q_ok}"
            check_frame(gpu, oracle, name, cam, feats(2, 2), f"{rv} leaf {leaf} N=2 frame", w, h)
            for N in (1, 2):
                final_against_oracle(gpu, oracle, rv, (a, b), N, f"{rv} leaf {leaf}", [dict(final_qbvh=1), dict(final_qbvh=0, final_sort=0)])
    finally:
        gpu.set_tuning("bvh.max_leaf", 2)
        gpu.set_scene(shape_scene(name))
    print(f"leaf sizes {rv}: nodes {nodes}")
    assert nodes == sorted(nodes, reverse=True) and nodes[0] > nodes[-1]
    if rv == "night":
        assert all(x > y for x, y in zip(nodes[:5], nodes[1:5])), nodes
