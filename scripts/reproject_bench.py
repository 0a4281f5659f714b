#!/usr/bin/env python3
"""What motion-compensated temporal reuse costs, and what it buys (results: profiles/reproject/).

Cost.  The C3 workload of bench.py (nightclub, 128 point lights, 1080p, N = 1, M = 32, k = 5, r = 10, two biased passes,
temporal reuse) under a camera that yaws 0.1 degrees per frame: no read-back, one synchronise at the end.  Three arms,
each `--runs` processes of their own, interleaved a b c a b c ...:
  a  same-pixel temporal frames on another build of the library (--parent-tree: a checkout of the parent commit with
     its library built)
  b  the same frames on this tree
  c  Renderer.reproject + the frame on this tree
Per arm the median and the spread (min, max) of ms per frame; c - b is the cost of the feature.

    python scripts/reproject_bench.py --parent-tree ../parent --out profiles/reproject/cost.json

Quality (--quality): the mean absolute error of frame 8 of a 64 x 36 sequence yawing 2 degrees per frame against the mean
of 256 independent still frames at the final camera, for same-pixel and for reprojected reuse (and for no reuse).

    python scripts/reproject_bench.py --quality --out profiles/reproject/quality.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def night_camera(scene, w, h, yaw):
    return scene.make_camera(30.0, 25.0, (2.57, 1.23, -1.35), (10.3, yaw, 0.0), w, h)


def worker(args):
    """One arm in this process: prints {"ms_per_frame": ...}."""
    sys.path.insert(0, args.tree)
    from romis_amd import _abi, restir, scene
    W, H = args.width, args.height
    f = _abi.default_features(initial_light_samples=32, num_samples_in_reservoir=1, num_neighbours_to_sample=5,
                              spatial_resample_radius=10, spatial_resampling_passes=2, temporal_reuse=1)
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene("nightclub_128pt"))
    r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
    cams = [night_camera(scene, W, H, 30.0 + 0.1 * k) for k in range(args.warmup + args.steps)]
    prev = None

    def frame(k):
        nonlocal prev
        if args.worker == "reproject" and prev is not None:
            prev = r.reproject(prev, cams[k - 1], cams[k])
        _, prev = r.render_restir(prev, cams[k], W, H, f, want_rgb=False)

    for k in range(args.warmup):
        frame(k)
    r.synchronize()
    t0 = time.perf_counter()
    for k in range(args.warmup, args.warmup + args.steps):
        frame(k)
    r.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"arm": args.worker, "tree": os.path.abspath(args.tree), "ms_per_frame": dt / args.steps * 1e3}), flush=True)
    prev = None
    r.close()


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs_ms": [round(v, 4) for v in ms]}


def cost(args):
    arms = [("b_same_pixel", "same", ROOT), ("c_reproject", "reproject", ROOT)]
    if args.parent_tree:
        arms.insert(0, ("a_parent_same_pixel", "same", os.path.abspath(args.parent_tree)))
    ms = {name: [] for name, _, _ in arms}
    for _ in range(args.runs):
        for name, mode, tree in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--tree", tree, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--width", str(args.width), "--height", str(args.height)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=120).stdout
            ms[name].append(json.loads(out.strip().splitlines()[-1])["ms_per_frame"])
    rec = {"workload": f"C3 features, nightclub 128 point lights, {args.width}x{args.height}, yaw 0.1 deg / frame, "
                       f"{args.steps} frames after {args.warmup}, {args.runs} interleaved processes per arm",
           "arms": {name: summary(v) for name, v in ms.items()}}
    b, c = rec["arms"]["b_same_pixel"], rec["arms"]["c_reproject"]
    rec["reproject_cost_ms"] = round(c["median_ms"] - b["median_ms"], 4)
    if args.parent_tree:
        a = rec["arms"]["a_parent_same_pixel"]
        rec["b_within_a_spread"] = a["min_ms"] <= b["median_ms"] <= a["max_ms"]
    return rec


def quality(args):
    import numpy as np
    sys.path.insert(0, ROOT)
    from romis_amd import _abi, restir, scene
    W, H, frames, stills, step = 64, 36, 8, 256, 2.0
    f = _abi.default_features(initial_light_samples=32, num_samples_in_reservoir=1, num_neighbours_to_sample=5,
                              spatial_resample_radius=10, spatial_resampling_passes=2, temporal_reuse=1)
    f0 = _abi.Features.from_buffer_copy(f)
    f0.temporal_reuse = 0
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene("nightclub_128pt"))
    cams = [night_camera(scene, W, H, 30.0 + step * k) for k in range(frames + 1)]
    r.set_seed(_abi.RESTIR_DEFAULT_SEED, 1000)
    ref = np.zeros((H, W, 3), np.float64)
    for _ in range(stills):
        ref += r.render_restir(None, cams[frames], W, H, f0, want_grid=False)[0]
    ref /= stills
    rec = {"workload": f"nightclub 128 point lights, {W}x{H}, yaw {step} deg / frame, frame {frames} against the mean of "
                       f"{stills} independent still frames (no reuse across frames) at its camera; C3 features"}
    for mode in ("none", "same_pixel", "reprojected"):
        errs = []
        for trial in range(8):   # eight independent sequences (frame indices apart)
            r.set_seed(_abi.RESTIR_DEFAULT_SEED, 100 * trial)
            prev, rgb = None, None
            for k in range(frames + 1):
                if mode == "none":
                    prev = None
                elif mode == "reprojected" and prev is not None:
                    prev = r.reproject(prev, cams[k - 1], cams[k])
                rgb, prev = r.render_restir(prev, cams[k], W, H, f)
            errs.append(float(np.abs(rgb.astype(np.float64) - ref).mean()))
        rec[mode] = {"mean_abs_error": round(statistics.mean(errs), 6), "min": round(min(errs), 6), "max": round(max(errs), 6)}
    r.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["same", "reproject"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built (arm a)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    rec = quality(args) if args.quality else cost(args)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
