#!/usr/bin/env python3
"""What the exact image costs, and what it says about the estimators (restir_render_exact, restir_error_get).  Not the
headline bench (bench.py); nothing here is a pass / fail bar.

    python scripts/exact_bench.py [--reps 5] [--iters 50] [--frames 1024] [--out profiles/exact/exact.json]

Scene: the nightclub with 128 point lights at 1920 x 1080 over a still camera, tone mapping off.

(a) cost.  Wall ms per restir_render_exact(..., out_rgb = NULL) of a loop that only enqueues and synchronises once at the
    end, in --reps processes of their own, interleaved with (b)'s runs: median (min - max).  The call's two launches
    are inside the library, on a stream the script cannot record events into, so the split is taken from the library's
    own events instead of the script's: k_primary's event time over the same view through restir_stage_primary (the
    same kernel, the same launch shape), and k_exact = the call's wall time minus that.
(b) error against the exact image.  For C2's features, C3's (each frame's grid the next one's predecessor) and C2 with the
    unbiased combination and both visibility checks: frames 0, 1, ... of the still view are added to an accumulation,
    and after n = 1, 4, 16, 64, 256, 1024 of them the record holds est_mse (restir_accum_stats_get, from n = 2) beside
    the mean's true mse, bias, rel_mse, mae and max_abs against the exact image (restir_error_get), and
    bias2 = mse - est_mse: the squared bias where the frames are independent (with temporal reuse they are not, and
    the difference holds their correlation too).  The first frame's own figures are n = 1's.  Everything is reduced on
    the device; only structs come back.
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
NAME = "nightclub_128pt"
C2 = dict(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5, spatial_resample_radius=10,
          spatial_reuse=1, spatial_resampling_passes=1, temporal_reuse=0, enable_tone_mapping=0)
SETS = {
    "c2": C2,
    "c3": dict(C2, spatial_resampling_passes=2, temporal_reuse=1),
    "c2_unbiased_vis": dict(C2, unbiased_combination=1, spatial_reuse_visibility_check=1, initial_samples_visibility_check=1),
}
CHECKPOINTS = [1, 4, 16, 64, 256, 1024]


def new_renderer():
    from romis_amd import restir, scene
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene(NAME))
    r.set_seed(0x5EED, 0)
    return r, scene.camera_for(NAME, *SIZE)


def child_cost(iters, warmup):
    from romis_amd import _abi
    w, h = SIZE
    r, cam = new_renderer()
    f = _abi.default_features(enable_tone_mapping=0)
    for _ in range(warmup):
        r.render_exact(cam, w, h, f, download=False)
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r.render_exact(cam, w, h, f, download=False)
    r.synchronize()
    rec = {"what": "cost", "iters": iters, "exact_ms": (time.perf_counter() - t0) * 1e3 / iters}
    # k_primary over the same view, by the library's events
    r.stage_configure(w, h, 1)
    for _ in range(warmup):
        r.stage_primary(cam)
    r.enable_timing(True)
    r.set_tuning("timing.mask", -1)
    r.reset_timings()
    for _ in range(iters):
        r.stage_primary(cam)
    ms, n = r.timings()["primary"]
    r.enable_timing(False)
    rec["primary_ms"] = ms / max(n, 1)
    rec["primary_launches"] = int(n)
    rec["k_exact_ms"] = rec["exact_ms"] - rec["primary_ms"]
    r.close()
    print(json.dumps(rec))


def child_table(name, frames):
    from romis_amd import _abi
    w, h = SIZE
    r, cam = new_renderer()
    f = _abi.default_features(**SETS[name])
    r.render_exact(cam, w, h, _abi.default_features(enable_tone_mapping=0), download=False)
    r.reference_set()
    r.accum_begin(True)
    rows, prev = [], None
    t0 = time.perf_counter()
    for n in range(1, frames + 1):
        _, prev = r.render_restir(prev if f.temporal_reuse else None, cam, w, h, f, want_rgb=False, want_grid=bool(f.temporal_reuse))
        r.accum_add()
        if n in CHECKPOINTS:
            e = r.error("accum")
            row = dict(n=n, mse=e.mse, bias=e.bias, rel_mse=e.rel_mse, mae=e.mae, max_abs=e.max_abs, nonfinite=e.nonfinite,
                       ref_mean=e.ref_mean)
            if n >= 2:
                s = r.accum_stats()
                row.update(est_mse=s.est_mse, bias2=e.mse - s.est_mse)
            rows.append(row)
    wall = time.perf_counter() - t0
    r.close()
    print(json.dumps({"what": "table", "set": name, "features": SETS[name], "rows": rows, "wall_s": wall}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=CHECKPOINTS[-1])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact", "exact.json"))
    ap.add_argument("--child", nargs="+", metavar="WHAT")
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "cost":
            child_cost(args.iters, args.warmup)
        else:
            child_table(args.child[1], args.frames)
        return 0

    def run(extra, limit):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup),
                              "--frames", str(args.frames), "--child"] + extra, capture_output=True, text=True, timeout=limit)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            return None   # a failed run ends the measurement: nothing more is started
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        print(json.dumps(rec), flush=True)
        return rec

    cost, tables = [], {}
    names = list(SETS)
    for rep in range(args.reps):
        rec = run(["cost"], 120)
        if rec is None:
            return 1
        cost.append(rec)
        if rep < len(names):   # the table runs, interleaved with the cost runs
            rec = run(["table", names[rep]], 400)
            if rec is None:
                return 1
            tables[names[rep]] = rec
    for name in names[args.reps:]:
        rec = run(["table", name], 400)
        if rec is None:
            return 1
        tables[name] = rec

    def spread(key):
        v = [c[key] for c in cost]
        return {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "runs": v}

    result = {
        "image": list(SIZE), "scene": NAME, "reps": args.reps, "iters": args.iters,
        "cost": {"what": "restir_render_exact(..., NULL): wall ms per call of an enqueue-only loop, one synchronise at the end; "
                         "primary = k_primary's event time over the same view through restir_stage_primary; k_exact = the difference",
                 "exact": spread("exact_ms"), "primary": spread("primary_ms"), "k_exact": spread("k_exact_ms")},
        "table": {"what": "the mean of n accumulated frames of the still view against the exact image, tone mapping off: est_mse "
                          "(restir_accum_stats_get), true mse / bias / rel_mse / mae / max_abs (restir_error_get), bias2 = mse - est_mse",
                  "sets": tables},
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
