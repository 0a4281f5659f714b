"""csrc/bvh.cpp on its own, on the CPU: the flattened tree's invariants and the ray walks' pruning against brute force.

tools/bvh_check (tests/cpp/bvh_check.cpp, built by romis_amd.build with the host compiler over csrc/bvh.cpp; no device
code) reads the triangle files written here and, for bvh.max_leaf in {1, 2, 3, 5, 15, 16, 255, 0, 1000}, checks that

  - tri_order is a permutation, every triangle lies in exactly one leaf, no leaf exceeds the clamped max_leaf;
  - every node's box contains its subtree's vertices with the pad, and lies inside its parent's;
  - every miss link is greater than its node's index and names the next subtree in preorder (the root's: num_nodes) --
    so a walk's node index only grows and any ray, a NaN one included, ends after at most num_nodes steps;
  - quantize_nodes' boxes, dequantized, contain the float boxes, its link / first / count fields round-trip, and it
    reports ok exactly while the fields fit (leaves of < 16 triangles within the first 4,096; < 65,536 nodes);

and for 10^5 hashed rays per scene (shadow rays built as visible() builds them -- generic, one and two exact zero
direction components, zero length (a NaN direction), ending on a surface, at a vertex, inside a triangle, a subnormal
component, 5e-4 and 1e19 long, single NaN components -- and the same rays as closest-hit rays) over the trees of
max_leaf 2, 3, 15 and 16, that the leaves accepted by the restated occluded / occluded_q walks hold every triangle the
exact test hits, and that the restated closest() returns brute force's (t, triangle) with the lowest-index tie rule.

Inputs: every prebuilt scene, 0 / 1 / 2 triangles, 300 identical triangles (the count / 2 split), zero-area triangles
(three equal vertices; collinear vertices along an axis), an axis-aligned coplanar sheet (flat boxes), and the nightclub
translated by (2e4, 3e4, -1e4).

Collinear vertices in general position ("slivers") get the invariants alone.  Their det = e1 . (d x e2) is the rounding
error of a zero, the exact test's u, v, t are quotients of such errors, and it reports hits at distances unrelated to
where the triangle lies: over these 48 triangles brute force differs from the walk (ray 16911: t = 0.41666669 on
triangle 36 against 0.51416016 on triangle 25).  No box can promise to contain such a hit; the pruning argument, and
the device's equality with the brute-force oracle, hold for triangles with an area.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from romis_amd import build, scene

LEAVES = [1, 2, 3, 5, 15, 16, 255, 0, 1000]
RAY_FAMILIES = 11
SLIVERS = "slivers"   # collinear vertices in general position: the invariants alone (see the docstring)
f32 = np.float32


def scene_triangles(s):
    """[T][3][3] float32, mesh order (the order restir_set_scene flattens them in)."""
    parts = [np.asarray(m.positions, f32)[np.asarray(m.triangles, np.int64)] for m in s.meshes if len(m.triangles)]
    return np.concatenate(parts) if parts else np.zeros((0, 3, 3), f32)


def synthetic_inputs():
    rng = np.random.default_rng(11)
    one = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], f32)
    two = np.concatenate([one, one[:, ::-1] + f32(0.5)])
    point = rng.uniform(-1, 1, (24, 1, 3)).astype(f32).repeat(3, axis=1)            # three equal vertices
    a, d = rng.uniform(-1, 1, (2, 24, 1, 3)).astype(f32)
    line = np.concatenate([a, a + d, a + d * f32(2)], axis=1)                         # collinear vertices
    along = d * np.eye(3, dtype=f32)[np.arange(24) % 3][:, None, :]                   # ... along one axis: det == 0 exactly
    axis_line = np.concatenate([a, a + along, a + along * f32(2)], axis=1)
    g = np.arange(13, dtype=f32) / f32(12)
    x0, z0 = (v.reshape(-1) for v in np.meshgrid(g[:-1], g[:-1], indexing="ij"))
    h, y = f32(1.0 / 12.0), np.full_like(x0, f32(0.5))
    p00, p10 = np.stack([x0, y, z0], -1), np.stack([x0 + h, y, z0], -1)
    p01, p11 = np.stack([x0, y, z0 + h], -1), np.stack([x0 + h, y, z0 + h], -1)
    sheet = np.concatenate([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)])
    night = scene_triangles(scene.load_prebuilt("CornellNightClub"))
    return {"empty": np.zeros((0, 3, 3), f32), "one": one, "two": two, "identical300": one.repeat(300, axis=0),
            "zero_area": np.concatenate([point, axis_line]).astype(f32), SLIVERS: np.concatenate([point, line]).astype(f32),
            "sheet": sheet.astype(f32),
            "nightclub_translated": (night + np.array([2e4, 3e4, -1e4], f32)).astype(f32)}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """bvh_check's lines over every input: ({(input, max_leaf): tree fields}, {input: ray fields}, stdout)."""
    tool = os.path.join(build.OUT, "tools", "bvh_check")
    if not os.path.exists(tool):
        tool = build.build_bvh_check()
    inputs = {n: scene_triangles(scene.load_prebuilt(n)) for n in scene.prebuilt_names()}
    inputs.update(synthetic_inputs())
    d = tmp_path_factory.mktemp("bvh")
    paths = []
    for name, tris in inputs.items():
        assert tris.dtype == f32 and tris.shape[1:] == (3, 3) and np.isfinite(tris).all()
        paths.append(str(d / f"{name}.tri"))
        with open(paths[-1], "wb") as fh:
            fh.write(np.uint32(len(tris)).tobytes() + np.ascontiguousarray(tris).tobytes())
    run = subprocess.run([tool] + [p for p in paths if SLIVERS not in p], capture_output=True, text=True)
    if run.returncode == 0:
        more = subprocess.run([tool, "--rays", "0"] + [p for p in paths if SLIVERS in p], capture_output=True, text=True)
        run = subprocess.CompletedProcess(run.args, more.returncode, more.stdout + run.stdout, more.stderr + run.stderr)
    trees, rays = {}, {}
    for line in run.stdout.splitlines():
        w = line.split()
        if w and w[0] == "tree":
            trees[(w[1][:-4], int(w[3]))] = dict(zip(w[4:-1:2], (int(v) for v in w[5:-1:2])), ok=w[-1] == "ok")
        elif w and w[0] == "rays":
            rays[w[1][:-4]] = dict(zip(w[2:-1:2], (int(v) for v in w[3:-1:2])), ok=w[-1] == "ok")
    return inputs, trees, rays, run


def test_checker_passes(report):
    inputs, trees, rays, run = report
    assert run.returncode == 0 and run.stdout.rstrip().endswith("PASSED: 0 failures"), run.stdout[-4000:] + run.stderr[-2000:]
    assert not re.search(r"^FAIL", run.stdout, flags=re.M)
    assert set(trees) == {(n, l) for n in inputs for l in LEAVES} and all(t["ok"] for t in trees.values())
    assert set(rays) == {n for n, t in inputs.items() if len(t) and n != SLIVERS} and all(r["ok"] for r in rays.values())


def test_trees_have_the_shapes_the_checks_assume(report):
    """The inputs reach what they were made for: leaves as large as the clamp allows, node counts that fall as the leaf
    grows, quantized nodes exactly below 16 triangles per leaf."""
    inputs, trees, _, _ = report
    for name, tris in inputs.items():
        T = len(tris)
        for leaf in LEAVES:
            t = trees[(name, leaf)]
            clamped = min(max(leaf, 1), 255)
            assert t["triangles"] == T and t["largest_leaf"] <= clamped
            if T == 0:
                assert t["nodes"] == 0 and t["q_ok"] == 0
                continue
            if clamped == 1:
                assert t["nodes"] == 2 * T - 1
            if T <= clamped:
                assert t["nodes"] == 1 and t["largest_leaf"] == T
            assert t["q_ok"] == (1 if t["largest_leaf"] < 16 else 0), (name, leaf, t)
        counts = [trees[(name, l)]["nodes"] for l in (1, 2, 3, 5, 15, 16, 255)]
        assert counts == sorted(counts, reverse=True), (name, counts)
        assert trees[(name, 0)]["nodes"] == trees[(name, 1)]["nodes"] and trees[(name, 1000)]["nodes"] == trees[(name, 255)]["nodes"]
    # 300 identical triangles: no SAH split exists, the range is halved down to the leaf size
    assert trees[("identical300", 1)]["nodes"] == 599 and trees[("identical300", 16)]["largest_leaf"] == 10
    for name in ("Monkey", "sheet", "identical300"):
        assert trees[(name, 16)]["q_ok"] == 0 or trees[(name, 16)]["largest_leaf"] < 16
    assert trees[("Monkey", 255)]["q_ok"] == 0 and trees[("Monkey", 15)]["q_ok"] == 1


def test_rays_reach_the_cases_they_were_hashed_for(report):
    inputs, _, rays, _ = report
    for name, r in rays.items():
        n = r["n"]
        assert n == 100000
        assert r["zero_component"] >= 2 * n // RAY_FAMILIES and r["nan"] >= n // RAY_FAMILIES - 1, (name, r)
        assert r["subnormal"] >= (n + RAY_FAMILIES - 8) // RAY_FAMILIES, (name, r)
        assert r["occluded"] + r["clear"] == n
    for name in ("CornellNightClub", "Monkey", "CubeTextured", "CornellBox", "sheet", "nightclub_translated", "identical300"):
        r = rays[name]
        assert r["occluded"] >= 1000 and r["clear"] >= 1000 and r["closest"] >= 1000, (name, r)
    assert rays["zero_area"]["occluded"] == 0 and rays["zero_area"]["closest"] == 0
    # closest-hit ties (two triangles at one t: shared edges, the identical triangles) take the lowest-index rule
    assert rays["identical300"]["ties"] == rays["identical300"]["closest"] >= 1000
