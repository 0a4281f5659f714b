#!/usr/bin/env python3
"""What a frame costs when the scene changes before it: a whole restir_set_scene against restir_update_meshes (device
refit) and restir_set_lights.  Not the headline bench (bench.py).

    python scripts/update_bench.py [--parent-tree PATH] [--reps 5] [--iters 40] [--out profiles/dynamic/update.json]

Scenes: the nightclub with 128 point lights at 1920 x 1080 with C3's features (two passes, temporal reuse, the grid
threaded through), and Monkey at 512 x 512.  Per scene and mode, wall time per iteration of "change the scene, render one
frame, read the image back":

    set_scene_parent   restir_set_scene(moved scene) + frame, in a built checkout of the parent commit (--parent-tree; skipped without)
    set_scene          the same on this tree's library
    update_meshes      restir_update_meshes(the moved mesh) + frame
    set_lights         restir_set_lights(moved lights) + frame
    still              the frame alone (nothing changes)

Each (scene, mode) runs in --reps processes of its own, interleaved mode by mode so that drift lands on all alike; a
process warms up, then times --iters iterations and reports their median.  The record holds, per (scene, mode), the
median over the processes and their spread (max - min).  The moved mesh alternates between two positions, so every
iteration changes the geometry.  (The refit launches' own time is not in here: the library exposes no events for it.)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {
    "nightclub_1080p_c3": dict(scene="nightclub_128pt", size=(1920, 1080), mesh=9, step=(0.0, 0.4, 0.3),
                               features=dict(num_samples_in_reservoir=1, spatial_resampling_passes=2, temporal_reuse=1)),
    "monkey_512": dict(scene="Monkey", size=(512, 512), mesh=0, step=(0.04, -0.03, 0.02),
                       features=dict(num_samples_in_reservoir=1, spatial_resampling_passes=2, temporal_reuse=1)),
}
MODES = ["set_scene_parent", "set_scene", "update_meshes", "set_lights", "still"]


def child(name, mode, iters, warmup, tree):
    import dataclasses

    if tree:   # the package (and its library) of another checkout
        sys.path[:] = [os.path.abspath(tree)] + [p for p in sys.path if os.path.abspath(p or ".") != ROOT]

    import numpy as np

    from romis_amd import _abi, restir, scene
    cfg = SCENES[name]
    w, h = cfg["size"]
    s = scene.bench_scene(cfg["scene"])
    cam = scene.cornell_framed_camera(w, h) if cfg["scene"] == "Monkey" else scene.camera_for(cfg["scene"], w, h)
    f = _abi.default_features(**cfg["features"])
    m = cfg["mesh"]
    base = np.ascontiguousarray(s.meshes[m].positions, np.float32)
    moved = [base, (base + np.asarray(cfg["step"], np.float32)).astype(np.float32)]
    scenes = [scene.Scene([dataclasses.replace(x, positions=p) if i == m else x for i, x in enumerate(s.meshes)], s.lights, s.name)
              for p in moved]
    lights = [s.lights, []]
    for l in s.lights:
        q = _abi.Light.from_buffer_copy(l)
        q.p0[:] = [q.p0[0] + 0.11, q.p0[1] - 0.07, q.p0[2] + 0.05]
        lights[1].append(q)
    r = restir.Renderer(0)
    r.set_scene(s)
    prev = None
    times = []
    for it in range(warmup + iters):
        t0 = time.perf_counter()
        if mode.startswith("set_scene"):
            r.set_scene(scenes[it & 1])
        elif mode == "update_meshes":
            r.update_meshes({m: (moved[it & 1], None)})
        elif mode == "set_lights":
            r.set_lights(lights[it & 1])
        _, prev = r.render_restir(prev if f.temporal_reuse else None, cam, w, h, f)
        if it >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    info = r.scene_info()
    r.close()
    print(json.dumps({"scene": name, "mode": mode, "ms_median": statistics.median(times), "ms_min": min(times),
                      "iters": iters, "nodes": info.num_nodes, "tris": info.num_tris, "bvh_lds_bytes": info.bvh_lds_bytes}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (set_scene_parent)")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic", "update.json"))
    ap.add_argument("--child", nargs=2, metavar=("SCENE", "MODE"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.iters, args.warmup, args.tree)
        return 0
    modes = [m for m in MODES if m != "set_scene_parent" or args.parent_tree]
    runs = {}
    for name in SCENES:
        for rep in range(args.reps):
            for mode in modes:
                extra = ["--tree", args.parent_tree] if mode == "set_scene_parent" else []
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, mode, "--iters", str(args.iters),
                                      "--warmup", str(args.warmup)] + extra, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    sys.stderr.write(out.stdout + out.stderr)
                    return 1   # a failed run ends the measurement: nothing more is started
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                runs.setdefault((name, mode), []).append(rec)
                print(json.dumps(rec), flush=True)
    result = {"reps": args.reps, "iters": args.iters, "what": "wall ms per (scene change + one frame + image read-back)", "scenes": {}}
    for (name, mode), recs in runs.items():
        med = [x["ms_median"] for x in recs]
        result["scenes"].setdefault(name, {"nodes": recs[0]["nodes"], "tris": recs[0]["tris"],
                                           "bvh_lds_bytes": recs[0]["bvh_lds_bytes"], "modes": {}})
        result["scenes"][name]["modes"][mode] = {"ms_median": statistics.median(med), "ms_spread": max(med) - min(med), "runs": med}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["scenes"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
