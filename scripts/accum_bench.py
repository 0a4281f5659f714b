#!/usr/bin/env python3
"""What accumulating frames on the device costs a still view (restir_accum_*).  Not the headline bench (bench.py).

    python scripts/accum_bench.py [--parent-tree PATH] [--reps 5] [--iters 400] [--out profiles/accum/accum.json]

Scene: the nightclub with 128 point lights at 1920 x 1080 over a still camera, once with C2's features (one pass, no
temporal reuse) and once with C3's (two passes, temporal reuse, the grid threaded through), tone mapping off.  Arms,
wall ms per frame of a loop that only enqueues and synchronises once at the end (total / frames):

    a  restir_render(..., NULL) in a built checkout of the parent commit (--parent-tree; skipped without)
    b  the same loop on this tree's library
    c  b plus restir_accum_add after every frame, without the variance (36 B per pixel)
    d  b plus restir_accum_add with the variance (60 B per pixel)
    e  restir_render_accumulate, 256 frames with the variance, including the resolve

Each (features, arm) runs in --reps processes of its own, interleaved arm by arm so that drift lands on all alike; a
process warms up, then times --iters frames.  Arms b, c and d also report the still view's cache counters after the
loop, and c and d the time of a device-to-device hipMemcpyAsync moving the add's total bytes, read plus written (a copy
of half of them), measured in the same process: the yardstick for a stream kernel.  The record holds, per (features,
arm), the median over the processes with their minimum and maximum, the bars of the feature's issue -- b within a's
min-max, c's and d's counters equal to b's -- and the per-add costs c - b and d - b next to the copies.  (The stats
kernel's own time and whether the state stays in the Infinity Cache between frames are not in here.)
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
    "c2": dict(num_samples_in_reservoir=1, spatial_resampling_passes=1, temporal_reuse=0, enable_tone_mapping=0),
    "c3": dict(num_samples_in_reservoir=1, spatial_resampling_passes=2, temporal_reuse=1, enable_tone_mapping=0),
}
ARMS = ["a", "b", "c", "d", "e"]
ACCUMULATE_FRAMES = 256
BYTES_PER_PIXEL = {"c": 36, "d": 60}   # the add's traffic: the image read, each state plane read and written


def copy_ms(nbytes, iters):
    """ms per device-to-device hipMemcpyAsync of nbytes (it reads nbytes and writes nbytes)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    src, dst = C.c_void_p(), C.c_void_p()
    for p in (src, dst):
        if hip.hipMalloc(C.byref(p), nbytes) != 0:
            raise RuntimeError("hipMalloc failed")

    def run(n):
        for _ in range(n):
            if hip.hipMemcpyAsync(dst, src, nbytes, 3, None) != 0:   # hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpyAsync failed")
        if hip.hipDeviceSynchronize() != 0:
            raise RuntimeError("hipDeviceSynchronize failed")
    run(20)
    t0 = time.perf_counter()
    run(iters)
    ms = (time.perf_counter() - t0) * 1e3 / iters
    hip.hipFree(src)
    hip.hipFree(dst)
    return ms


def child(name, arm, iters, warmup, tree):
    if tree:   # the package (and its library) of another checkout
        sys.path[:] = [os.path.abspath(tree)] + [p for p in sys.path if os.path.abspath(p or ".") != ROOT]

    import ctypes as C

    from romis_amd import _abi, restir, scene
    w, h = SIZE
    f = _abi.default_features(**SETS[name])
    cam = scene.camera_for("nightclub_128pt", w, h)
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene("nightclub_128pt"))
    temporal = bool(f.temporal_reuse)
    rec = {"set": name, "arm": arm, "iters": iters}

    def render(prev):
        nxt = C.c_void_p()
        restir.check(r.lib, r.lib.restir_render(r.ctx, C.byref(cam), C.byref(f), w, h, None, prev.handle if prev is not None else None,
                                                C.byref(nxt) if temporal else None, None), "restir_render")
        return restir.ReservoirGrid(r.lib, nxt) if temporal else None

    if arm == "e":
        r.render_accumulated(cam, w, h, f, warmup, want_rgb=False)   # the caches and the buffers stand
        r.synchronize()
        t0 = time.perf_counter()
        _, stats = r.render_accumulated(cam, w, h, f, ACCUMULATE_FRAMES, want_rgb=False)   # (its stats synchronise)
        r.synchronize()
        rec["ms"] = (time.perf_counter() - t0) * 1e3 / ACCUMULATE_FRAMES
        rec["iters"] = ACCUMULATE_FRAMES
        rec["est_mse"] = stats.est_mse
    else:
        if arm in ("c", "d"):
            r.accum_begin(variance=arm == "d")
        prev = None
        t0 = 0.0
        for it in range(warmup + iters):
            if it == warmup:
                r.synchronize()
                t0 = time.perf_counter()
            prev = render(prev)
            if arm in ("c", "d"):
                r.accum_add()
        r.synchronize()
        rec["ms"] = (time.perf_counter() - t0) * 1e3 / iters
        del prev
        if arm != "a":
            rec["counters"] = dict(gbuf_reuses=r.gbuf_reuses(), shadow_list_frames=r.shadow_list_frames(),
                                   shadow_vis_frames=r.shadow_vis_frames(), shadow_vis_builds=r.shadow_vis_builds(),
                                   phat_frames=r.phat_frames(), phat_builds=r.phat_builds())
        if arm in ("c", "d"):
            rec["copy_bytes"] = w * h * BYTES_PER_PIXEL[arm] // 2
            rec["copy_ms"] = copy_ms(rec["copy_bytes"], iters)
    r.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (arm a)")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum", "accum.json"))
    ap.add_argument("--arms", default=None, help="a subset, e.g. b,c,d")
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
              "what": "wall ms per frame of an enqueue-only loop over a still 1080p nightclub view, one synchronise at the end",
              "arms": {"a": "parent commit: restir_render(..., NULL)", "b": "this tree: restir_render(..., NULL)",
                       "c": "b + restir_accum_add without the variance", "d": "b + restir_accum_add with the variance",
                       "e": f"restir_render_accumulate, {ACCUMULATE_FRAMES} frames with the variance, including the resolve"},
              "sets": {}}
    for (name, arm), recs in runs.items():
        ms = [x["ms"] for x in recs]
        s = result["sets"].setdefault(name, {"features": SETS[name], "arms": {}})
        s["arms"][arm] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": ms}
        if "counters" in recs[0]:
            s["arms"][arm]["counters"] = recs[0]["counters"]
            s["arms"][arm]["counters_equal_in_every_run"] = all(x["counters"] == recs[0]["counters"] for x in recs)
        if "copy_ms" in recs[0]:
            cp = [x["copy_ms"] for x in recs]
            s["arms"][arm]["copy"] = {"bytes_copied": recs[0]["copy_bytes"], "ms_median": statistics.median(cp), "ms_min": min(cp),
                                      "ms_max": max(cp)}
    for name, s in result["sets"].items():
        a = s["arms"]
        s["bars"] = {}
        if "a" in a and "b" in a:
            s["bars"]["b_within_a_min_max"] = a["a"]["ms_min"] <= a["b"]["ms_median"] <= a["a"]["ms_max"]
        for arm in ("c", "d"):
            if arm in a and "b" in a:
                s["bars"][f"{arm}_counters_equal_b"] = a[arm]["counters"] == a["b"]["counters"]
                add = a[arm]["ms_median"] - a["b"]["ms_median"]
                s[f"add_{arm}_minus_b_ms"] = add
                s[f"add_{arm}_over_copy"] = add / a[arm]["copy"]["ms_median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["sets"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
