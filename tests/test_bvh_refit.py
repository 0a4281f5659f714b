"""csrc/bvh.cpp refit_bvh on the CPU: a tree built over a scene and refitted to the scene moved keeps every invariant a
built tree has, prunes no hit, and reproduces build_bvh's nodes bit for bit when nothing moved.

tools/refit_check (tests/cpp/refit_check.cpp, which includes bvh_check.cpp for the invariants, the restated device walks
and the hashed rays) builds the tree of the original triangles for bvh.max_leaf in {1, 2, 3, 5, 15, 16}, refits it to the
moved ones and checks

  - unchanged topology: tri_order, every miss link and leaf word;
  - every node's box contains its subtree's moved vertices with the new pad, lies inside its parent's, and the root's is
    exactly the moved scene's padded bounds (so a refit that only grew boxes fails on a scene that shrank);
  - quantize_nodes of the refitted tree contains the float boxes;
  - over 10^5 hashed rays of bvh_check's families, on the trees of max_leaf 2, 3, 15 and 16: the walks accept every
    leaf that holds an exact hit and closest() equals brute force.

Inputs: Cube, CornellNightClub, Monkey, and test_bvh_invariants' sheet and identical300.  Deformations (each asserted
here to be what it claims): (a) one part translated out of the original bounds, (b) everything scaled by 0.25 about
the bounds' low corner, (c) a translation by (2e4, 3e4, -1e4), (d) one part collapsed to a point -- zero-area triangles,
the invariants alone, as test_bvh_invariants treats them --, (e) a per-vertex jitter of 5 % of the extent, (f) nothing.
A "part" is one mesh of a scene with several, else the first half of the vertices.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from romis_amd import build, scene
from test_bvh_invariants import synthetic_inputs

f32 = np.float32
LEAVES = [1, 2, 3, 5, 15, 16]
DEFORMATIONS = ["grow", "shrink", "far", "collapse", "jitter", "identity"]
FAR = np.array([2e4, 3e4, -1e4], f32)


def bounds(positions):
    allp = np.concatenate([p for p in positions if len(p)])
    return allp.min(axis=0), allp.max(axis=0)


def moving_part(positions):
    """(mesh index, vertex mask) of the part deformations (a) and (d) move."""
    if len(positions) > 1:
        m = max(range(len(positions)), key=lambda i: (len(positions[i]) > 0, i == len(positions) // 2))
        return m, np.ones(len(positions[m]), bool)
    mask = np.zeros(len(positions[0]), bool)
    mask[:max(3, (len(mask) // 6) * 3)] = True
    return 0, mask


def _hash_unit(n, salt):
    """[n][3] float32 in [-1, 1): murmur3's finaliser over the vertex number."""
    h = (np.arange(3 * n, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    for s, m in ((16, 0x85EBCA6B), (13, 0xC2B2AE35)):
        h ^= h >> np.uint64(s)
        h = (h * np.uint64(m)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return ((h >> np.uint64(8)).astype(f32) * f32(2.0 / 16777216.0) - f32(1.0)).reshape(n, 3)


def deform(positions, kind, step=1.0):
    """The per-mesh vertex positions (a list of [V][3] float32) moved; every result is checked to be what `kind` says."""
    positions = [np.ascontiguousarray(p, f32) for p in positions]
    lo, hi = bounds(positions)
    ext = (hi - lo).astype(f32)
    size = f32(max(ext.max(), f32(1e-3)))
    out = [p.copy() for p in positions]
    if kind == "grow":
        m, mask = moving_part(positions)
        out[m][mask] = (positions[m][mask] + np.array([size, f32(0.25) * size, 0], f32) * f32(step)).astype(f32)
        nlo, nhi = bounds(out)
        assert nhi[0] > hi[0] and np.all(nhi - nlo >= ext) and (nhi - nlo)[0] > ext[0]      # the root box grows
        assert any(np.any(p[:, 0] > hi[0]) for p in out)                                    # a vertex outside the old one
    elif kind == "shrink":
        out = [(lo + (p - lo) * f32(0.25)).astype(f32) for p in positions]
        nlo, nhi = bounds(out)
        assert np.all(nhi - nlo <= ext) and (not ext.any() or np.any(nhi - nlo < ext))
        assert np.all(nlo >= lo) and np.all(nhi <= hi)                                      # inside the old bounds
    elif kind == "far":
        out = [(p + FAR).astype(f32) for p in positions]
        assert np.abs(np.concatenate(out)).max() > 100 * max(np.abs(lo).max(), np.abs(hi).max(), 1.0)   # another pad
    elif kind == "collapse":
        m, mask = moving_part(positions)
        out[m][mask] = positions[m][mask][0]
        assert len(np.unique(out[m][mask], axis=0)) == 1
    elif kind == "jitter":
        out = [(p + _hash_unit(len(p), i + 1) * (f32(0.05) * ext)).astype(f32) for i, p in enumerate(positions)]
        d = np.abs(np.concatenate(out) - np.concatenate(positions))
        assert d.max() <= 0.0501 * size and (not ext.any() or d.max() > 0.02 * ext.max())
    else:
        assert kind == "identity"
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(out, positions))
    assert all(np.isfinite(p).all() and p.dtype == f32 for p in out)
    return out


def mesh_inputs():
    """{name: (positions per mesh, triangles per mesh)}"""
    out = {}
    for name in ("Cube", "CornellNightClub", "Monkey"):
        s = scene.load_prebuilt(name)
        out[name] = ([np.asarray(m.positions, f32) for m in s.meshes], [np.asarray(m.triangles, np.int64) for m in s.meshes])
    syn = synthetic_inputs()
    for name in ("sheet", "identical300"):
        t = syn[name]
        out[name] = ([t.reshape(-1, 3).copy()], [np.arange(3 * len(t), dtype=np.int64).reshape(-1, 3)])
    return out


def triangles_of(positions, triangles):
    """[T][3][3] float32 in mesh order, as restir_set_scene flattens them."""
    return np.concatenate([p[t] for p, t in zip(positions, triangles) if len(t)]).astype(f32)


def write_tri(path, tris):
    assert tris.dtype == f32 and tris.shape[1:] == (3, 3)
    with open(path, "wb") as fh:
        fh.write(np.uint32(len(tris)).tobytes() + np.ascontiguousarray(tris).tobytes())


def refit_tool():
    tool = os.path.join(build.OUT, "tools", "refit_check")
    return tool if os.path.exists(tool) else build.build_refit_check()


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    tool = refit_tool()
    d = tmp_path_factory.mktemp("refit")
    rays_args, flat_args, cases = [], [], []
    for name, (pos, tri) in mesh_inputs().items():
        write_tri(str(d / f"{name}.tri"), triangles_of(pos, tri))
        for kind in DEFORMATIONS:
            write_tri(str(d / f"{name}.{kind}.tri"), triangles_of(deform(pos, kind), tri))
            args = [f"{name}.{kind}", str(d / f"{name}.tri"), str(d / f"{name}.{kind}.tri")]
            (flat_args if kind == "collapse" else rays_args).extend(args)
            cases.append(f"{name}.{kind}")
    run = subprocess.run([tool] + rays_args, capture_output=True, text=True)
    more = subprocess.run([tool, "--rays", "0"] + flat_args, capture_output=True, text=True)
    out = run.stdout + more.stdout
    trees, rays = {}, {}
    for line in out.splitlines():
        w = line.split()
        if w and w[0] == "refit":
            trees[(w[1], int(w[3]))] = dict(zip(w[4:-1:2], (int(v) for v in w[5:-1:2])), ok=w[-1] == "ok")
        elif w and w[0] == "rays":
            rays[w[1]] = dict(zip(w[2:-1:2], (int(v) for v in w[3:-1:2])), ok=w[-1] == "ok")
    return cases, trees, rays, (run.returncode, more.returncode), out + run.stderr + more.stderr


def test_refitted_trees_keep_the_invariants_and_prune_no_hit(report):
    cases, trees, rays, codes, out = report
    assert codes == (0, 0) and not re.search(r"^FAIL", out, flags=re.M), out[-4000:]
    assert out.count("PASSED: 0 failures") == 2
    assert set(trees) == {(c, l) for c in cases for l in LEAVES} and all(t["ok"] for t in trees.values())
    assert set(rays) == {c for c in cases if not c.endswith(".collapse")} and all(r["ok"] for r in rays.values())
    for name, r in rays.items():
        assert r["n"] == 100000 and r["occluded"] + r["clear"] == r["n"]
        assert r["occluded"] >= 1000 and r["clear"] >= 1000 and r["closest"] >= 1000, (name, r)


def test_boxes_move_as_the_deformation_says(report):
    cases, trees, _, _, _ = report
    for (case, leaf), t in trees.items():
        kind = case.split(".")[1]
        n = t["nodes"]
        assert n >= 1
        if kind == "identity":
            assert t["equal"] == n and t["grew"] == 0            # build_bvh's nodes bit for bit
        elif kind == "grow":
            assert t["grew"] >= 1 and t["equal"] < n             # the root at least
        elif kind == "shrink":
            assert t["shrank"] == n                              # every box moved, none wider on any axis
        elif kind == "far":
            assert t["equal"] == 0

