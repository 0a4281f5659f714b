#!/usr/bin/env python3
"""What a displayed frame costs: render one frame and get its image to the host, by each way out of the library.
Not the headline bench (bench.py).

    python scripts/present_bench.py [--parent-tree PATH] [--reps 5] [--iters 200] [--out profiles/present/present.json]

Scene: the nightclub with 128 point lights at 1920 x 1080 over a still camera, once with C2's features (one pass, no
temporal reuse) and once with C3's (two passes, temporal reuse, the grid threaded through).  Arms, wall ms per displayed
frame:

    a  restir_render(..., out_rgb) in a built checkout of the parent commit (--parent-tree; skipped without)
    b  the same call on this tree's library
    c  restir_render(..., NULL), then restir_download_rgba8
    d  restir_render(..., NULL), restir_image_begin(RGBA8), then wait for and release the PREVIOUS frame's snapshot:
       two snapshots in flight
    e  as d with RGB32F
    f  restir_render(..., NULL) only, one restir_synchronize at the end (total / frames): the frame alone

Every arm re-uses one host buffer, allocated and touched before the timed frames (the Python binding's render_restir
would allocate a fresh image per call).  Each (features, arm) runs in --reps processes of its own, interleaved arm by
arm so that drift lands on all alike; a process warms up, then times --iters frames and reports their median.  The
record holds, per (features, arm), the median over the processes, their minimum and maximum, and the bars of the
feature's issue: b within a's min-max, d's median below a's minimum.  --arms a,b --reps 15 repeats the two forms of the
one call more often, to tell a difference between the trees from the spread of five runs.  (The conversion kernel's
own time and the copy's GB/s are not in here: the library exposes no events for them.)
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

SIZE = (1920, 1080)
SETS = {
    "c2": dict(num_samples_in_reservoir=1, spatial_resampling_passes=1, temporal_reuse=0),
    "c3": dict(num_samples_in_reservoir=1, spatial_resampling_passes=2, temporal_reuse=1),
}
ARMS = ["a", "b", "c", "d", "e", "f"]


def child(name, arm, iters, warmup, tree):
    if tree:   # the package (and its library) of another checkout
        sys.path[:] = [os.path.abspath(tree)] + [p for p in sys.path if os.path.abspath(p or ".") != ROOT]

    import ctypes as C

    import numpy as np

    from romis_amd import _abi, restir, scene
    w, h = SIZE
    f = _abi.default_features(**SETS[name])
    cam = scene.camera_for("nightclub_128pt", w, h)
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene("nightclub_128pt"))
    temporal = bool(f.temporal_reuse)
    # one host buffer per arm, allocated and touched once: the arms time the read-back, not numpy's allocation
    rgb = np.ones((h, w, 3), np.float32)
    rgba = np.ones((h, w, 4), np.uint8)
    rgb_ptr, rgba_ptr = rgb.ctypes.data_as(C.POINTER(C.c_float)), rgba.ctypes.data_as(C.POINTER(C.c_uint8))

    def render(prev, out):   # restir_render itself: the binding's render_restir allocates its image per call
        nxt = C.c_void_p()
        restir.check(r.lib, r.lib.restir_render(r.ctx, C.byref(cam), C.byref(f), w, h, None, prev.handle if prev is not None else None,
                                                C.byref(nxt) if temporal else None, out), "restir_render")
        return restir.ReservoirGrid(r.lib, nxt) if temporal else None

    prev = None
    pending = None
    times = []
    t_all = 0.0
    for it in range(warmup + iters):
        if it == warmup and arm == "f":
            r.synchronize()
            t_all = time.perf_counter()
        t0 = time.perf_counter()
        if arm in ("a", "b"):
            prev = render(prev, rgb_ptr)
        else:
            prev = render(prev, None)
            if arm == "c":
                restir.check(r.lib, r.lib.restir_download_rgba8(r.ctx, rgba_ptr, w * h), "restir_download_rgba8")
            elif arm in ("d", "e"):
                im = r.present("rgba8" if arm == "d" else "rgb32f")
                if pending is not None:
                    pending.wait()      # the displayed frame: the previous one's pinned bytes
                    pending.release()
                pending = im
        if it >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    if pending is not None:
        pending.wait()
        pending.release()
    r.synchronize()
    if arm == "f":
        per = (time.perf_counter() - t_all) * 1e3 / iters
        times = [per]
    del prev
    r.close()
    print(json.dumps({"set": name, "arm": arm, "ms_median": statistics.median(times), "ms_min": min(times), "iters": iters}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (arm a)")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present", "present.json"))
    ap.add_argument("--arms", default=None, help="a subset, e.g. a,b (more --reps of the two forms of one call)")
    ap.add_argument("--child", nargs=2, metavar=("SET", "ARM"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.iters, args.warmup, args.tree)
        return 0
    arms = [a for a in ARMS if (a != "a" or args.parent_tree) and (not args.arms or a in args.arms.split(","))]
    runs = {}
    for name in SETS:
        for rep in range(args.reps):
            for arm in arms:
                extra = ["--tree", args.parent_tree] if arm == "a" else []
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, arm, "--iters", str(args.iters),
                                      "--warmup", str(args.warmup)] + extra, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    sys.stderr.write(out.stdout + out.stderr)
                    return 1   # a failed run ends the measurement: nothing more is started
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                runs.setdefault((name, arm), []).append(rec)
                print(json.dumps(rec), flush=True)
    result = {"reps": args.reps, "iters": args.iters, "image": list(SIZE),
              "what": "wall ms per displayed frame (render one 1080p nightclub frame, still camera, and get its image to the host)",
              "arms": {"a": "parent commit: restir_render(..., out_rgb)", "b": "this tree: restir_render(..., out_rgb)",
                       "c": "restir_render(..., NULL) + restir_download_rgba8",
                       "d": "restir_render(..., NULL) + restir_image_begin(RGBA8) + wait for the previous frame's snapshot",
                       "e": "as d with RGB32F", "f": "restir_render(..., NULL) only, one synchronise at the end"},
              "sets": {}}
    for (name, arm), recs in runs.items():
        med = [x["ms_median"] for x in recs]
        result["sets"].setdefault(name, {"features": SETS[name], "arms": {}})
        result["sets"][name]["arms"][arm] = {"ms_median": statistics.median(med), "ms_min": min(med), "ms_max": max(med), "runs": med}
    for name, s in result["sets"].items():
        a = s["arms"]
        s["bars"] = {}
        if "a" in a and "b" in a:
            s["bars"]["b_within_a_min_max"] = a["a"]["ms_min"] <= a["b"]["ms_median"] <= a["a"]["ms_max"]
        if "a" in a and "d" in a:
            s["bars"]["d_median_below_a_min"] = a["d"]["ms_median"] < a["a"]["ms_min"]
        if "d" in a and "f" in a:
            s["d_minus_f_ms"] = a["d"]["ms_median"] - a["f"]["ms_median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["sets"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
