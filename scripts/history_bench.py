#!/usr/bin/env python3
"""What the reprojected image history costs and what it gains (restir_history_* next to restir_denoise_lum).  Not the
headline bench (bench.py); nothing here is a pass / fail bar.

    python scripts/history_bench.py [--reps 5] [--frames 1000] [--out profiles/history/history.json]
    python scripts/history_bench.py --quality [--half] [--out profiles/history/quality.json]
    python scripts/history_bench.py --ab PARENT_TREE [--rounds 5] [--out profiles/history/bench_ab.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/history_bench.py --child trace
    python scripts/history_bench.py --steps-from DIR [--out profiles/history/kernels.json]
    ... --gather nearest|bilinear|both on the loop, the trace child and --quality: restir_history_gather_set's mode.  "both"
    runs the two modes side by side -- the loop's history arms per mode, interleaved; the trace child's twelve frames once
    per mode in one process, so that --steps-from reports both instantiations of k_history_advance from one run; one
    --quality process per mode -- and every record names its mode (profiles/history_bilinear/).

Scene: the nightclub with 128 point lights at 1920 x 1080, the camera yawing 0.1 degree per frame
(scripts/reproject_bench.py's motion), C2's features (one pass, no temporal reuse) and C3's (two passes, temporal reuse,
the grid threaded through without reprojection).  Every child process runs under a time limit of its own, and the first
one that fails ends the measurement: nothing more is started.

(1) the loop.  Wall ms per displayed frame of an enqueue-only loop that ends in restir_image_begin / wait (rgba8), --reps
    processes per arm, the arms interleaved: (a) render + present; (b) render + restir_denoise_lum SPATIAL + present;
    (c) render + restir_history_advance + restir_history_denoise + present; (c') as (c) with tuning history.var_fused = 0,
    the variance plane's three-launch variant; (d) as (c) with restir_history_resolve in place of the denoise.  Median
    (min - max).
(2) --steps-from: per-launch microseconds of k_history_* from a kernel trace of --child trace; the child itself prints the
    event-timed microseconds of a device-to-device copy that moves the 156 bytes per pixel k_history_advance moves.
(3) --quality: true mse, rel_mse, mae and bias against restir_render_exact of each frame's own view at frames 4, 16 and
    64 of the moving sequence, for the raw frame, restir_denoise_lum SPATIAL, the history's mean and
    restir_history_denoise; max_frames in {8, 16, 32, 64} x spatial_below in {2, 4, 8}; C2 and C3; one process per
    configuration.  --half: at frame 64 also the host filter with the variance plane as it is and scaled by 1/2.
(4) --ab: bench.py C2 / C3 of this tree against a built checkout of the parent commit, one process each, trees interleaved,
    the order within a pair alternating.
"""
import argparse
import csv
import glob
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
YAW_STEP = 0.1
C2 = dict(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5, spatial_resample_radius=10,
          spatial_reuse=1, spatial_resampling_passes=1, temporal_reuse=0, enable_tone_mapping=0)
SETS = {"c2": C2, "c3": dict(C2, spatial_resampling_passes=2, temporal_reuse=1)}
ARMS = ["present", "spatial", "history", "history_three", "history_resolve"]
CAPS = [8, 16, 32, 64]
BELOWS = [2, 4, 8]
AT = [4, 16, 64]
OUT_DIR = os.path.join(ROOT, "profiles", "history")
GATHERS = {"nearest": 0, "bilinear": 1}   # RESTIR_HISTORY_GATHER_*


def new_renderer():
    from romis_amd import restir, scene
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene(NAME))
    r.set_seed(0x5EED, 0)
    return r


def camera(k):
    """the nightclub's camera yawed by k steps (scripts/reproject_bench.py's night_camera)"""
    from romis_amd import scene
    return scene.make_camera(30.0, 25.0, (2.57, 1.23, -1.35), (10.3, 30.0 + YAW_STEP * k, 0.0), *SIZE)


def render_loop(r, f):
    import ctypes as C

    from romis_amd import restir
    w, h = SIZE
    temporal = bool(f.temporal_reuse)

    def render(cam, prev):
        nxt = C.c_void_p()
        restir.check(r.lib, r.lib.restir_render(r.ctx, C.byref(cam), C.byref(f), w, h, None, prev.handle if prev is not None else None,
                                                C.byref(nxt) if temporal else None, None), "restir_render")
        return restir.ReservoirGrid(r.lib, nxt) if temporal else None
    return render


def child_loop(cfg, arm, frames, warmup, gather):
    from romis_amd import _abi
    w, h = SIZE
    r = new_renderer()
    r.history_gather(GATHERS[gather])
    f = _abi.default_features(**SETS[cfg])
    tone = _abi.default_features()
    render = render_loop(r, f)
    cams = [camera(k) for k in range(frames + warmup)]
    if arm.startswith("history"):
        r.history_begin()
    if arm == "history_three":
        r.set_tuning("history.var_fused", 0)   # the variance plane's other variant: spatial everywhere, then selected
    prev = None
    t0 = None
    for k, cam in enumerate(cams):
        if k == warmup:
            r.synchronize()
            t0 = time.perf_counter()
        prev = render(cam, prev)
        if arm == "spatial":
            r.denoise_lum(cam, w, h, tone=tone, download=False)
        elif arm in ("history", "history_three"):
            r.history_advance(cam, w, h)
            r.history_denoise(tone=tone, download=False)
        elif arm == "history_resolve":
            r.history_advance(cam, w, h)
            r.history_resolve(tone)
        with r.present("rgba8") as im:
            im.wait()
    r.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / frames
    print(json.dumps({"what": "loop", "cfg": cfg, "arm": arm, "gather": gather, "frames": frames, "ms_per_frame": ms,
                      "guide_builds": r.denoise_guide_builds()}))
    r.close()


def child_trace(gathers):
    """a short history loop per gather mode for a kernel trace, and device-to-device copies of the bytes a nearest advance
    moves"""
    import torch

    from romis_amd import _abi
    w, h = SIZE
    r = new_renderer()
    f = _abi.default_features(**C2)
    render = render_loop(r, f)
    for gather in gathers:
        r.history_gather(GATHERS[gather])
        r.history_begin()
        for k in range(12):
            cam = camera(k)
            render(cam, None)
            r.history_advance(cam, w, h)
            r.history_denoise(download=False)
        r.synchronize()
        r.history_end()
    r.close()
    half = w * h * 156 // 2   # a copy reads and writes its bytes: half the advance's traffic each way
    a = torch.empty(half, dtype=torch.uint8, device="cuda")
    b = torch.empty(half, dtype=torch.uint8, device="cuda")
    us = []
    for _ in range(24):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    print(json.dumps({"what": "trace", "copy_bytes_each_way": half, "copy_us": summary(us[4:])}))


def figures(e):
    return dict(mse=e.mse, rel_mse=e.rel_mse, mae=e.mae, bias=e.bias, max_abs=e.max_abs, nonfinite=e.nonfinite)


def child_quality(cfg, caps, belows, half, gather):
    """per (max_frames, spatial_below) one moving sequence of max(AT) frames; the four arms' figures at every frame of AT.
    half: at frame max(AT) also the host filter over the downloaded history with the variance plane as it is and scaled by
    1/2 (what the cap's over-statement could cost), against the downloaded exact image"""
    import numpy as np

    from romis_amd import _abi, restir, scene
    w, h = SIZE
    r = new_renderer()
    f = _abi.default_features(**SETS[cfg])
    render = render_loop(r, f)
    miss = len(scene.bench_scene(NAME).meshes)
    r.history_gather(GATHERS[gather])
    for cap in caps:
        for below in belows:
            hp = restir.history_params(max_frames=cap, spatial_below=below)
            r.set_seed(0x5EED, 0)
            r.history_begin(hp)
            prev = None
            for k in range(max(AT)):
                cam = camera(k)
                prev = render(cam, prev)
                r.history_advance(cam, w, h)
                if k + 1 not in AT:
                    continue
                rec = {"what": "quality", "cfg": cfg, "gather": gather, "max_frames": cap, "spatial_below": below, "frame": k + 1}
                raw = r.download_rgb(w, h)
                exact = r.render_exact(cam, w, h, f)   # consumes no frame index, leaves the frame path's caches
                r.reference_set()
                rec["raw"] = figures(restir.error_measure(raw, exact))
                r.history_resolve(None)
                rec["history_mean"] = figures(r.error("image"))
                r.history_denoise(download=False)
                rec["history_denoise"] = figures(r.error("image"))
                if cap == caps[0] and below == belows[0]:   # the spatial arm does not depend on the history's parameters
                    r.stage_configure(w, h, 1)
                    r.upload(_abi.BUF_RGB, raw)
                    r.denoise_lum(cam, w, h, download=False)
                    rec["spatial"] = figures(r.error("image"))
                mean, S, n = r.history_state()
                rec["n_mean"] = float(n.mean())
                rec["n_below"] = float((n < below).mean())
                if half and k + 1 == max(AT) and (cap, below) == (32, 4):
                    r.stage_configure(w, h, 1)
                    r.stage_primary(cam)
                    n_t, p_mat = r.download(_abi.BUF_GBUF_N_T), r.download(_abi.BUF_GBUF_P_MAT)
                    p = restir.denoise_lum_params()
                    var = restir.history_variance_host(mean, S, n, n_t, p_mat, miss, hp, p.geo)
                    for label, scale in (("host_full", 1.0), ("host_half", 0.5)):
                        out = restir.denoise_lum_host(mean, n_t, p_mat, miss, p, var=var * np.float32(scale))[0]
                        rec[label] = figures(restir.error_measure(out, exact))
                print(json.dumps(rec), flush=True)
    r.close()


def run_child(args, limit=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {args} ended with {p.returncode}: nothing more is started")
    return [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def bench_ab(parent, rounds, out):
    """bench.py C2 / C3, one process each, parent tree / this tree interleaved, the order within a pair alternating"""
    runs = {c: {"parent": [], "this": []} for c in ("c2", "c3")}
    for rnd in range(rounds):
        for cfg in runs:
            order = [("parent", parent), ("this", ROOT)]
            if rnd % 2:
                order.reverse()
            for label, tree in order:
                o = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20",
                                    "--config", cfg, "--no-cpu-baseline", "--no-cpu-stages"], cwd=tree, capture_output=True, text=True,
                                   timeout=300)
                if o.returncode != 0:
                    sys.stderr.write(o.stdout[-2000:] + o.stderr[-2000:])
                    raise SystemExit("a bench.py run failed: nothing more is started")
                runs[cfg][label].append(json.loads(o.stdout.strip().splitlines()[-1])["ms_per_step"])
                print(rnd, cfg, label, runs[cfg][label][-1], flush=True)
    res = {"what": "bench.py --gpus 1 --steps 200 --warmup 20 --config <c> --no-cpu-baseline --no-cpu-stages ms_per_step, one process "
                   f"each, parent commit / this tree interleaved, the order within a pair alternating, {rounds} rounds", "configs": {}}
    for cfg, r in runs.items():
        p, t = summary(r["parent"]), summary(r["this"])
        res["configs"][cfg] = {"parent": p, "this": t, "this_median_within_parent_min_max": p["min"] <= t["median"] <= p["max"]}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["configs"]))


def steps_from(d):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    per = {}
    for row in rows:
        name = row.get("Kernel_Name", "")
        if "k_history_advance" in name:   # the instantiation: <1u> demangled, ILj1E mangled
            tail = name.split("k_history_advance", 1)[1]
            name = "k_history_advance<bilinear>" if tail.startswith(("<1", "ILj1E")) else "k_history_advance<nearest>"
        key = next((k for k in ("k_history_advance<bilinear>", "k_history_advance<nearest>", "k_history_resolve", "k_history_var_fused", "k_history_var", "k_denoise_var_spatial", "k_denoise_level")
                    if k in name), None)
        if key:
            per.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(summary(v[2:] if len(v) > 4 else v), unit="us") for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cfgs", default="c2,c3")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--caps", default=",".join(map(str, CAPS)))
    ap.add_argument("--belows", default=",".join(map(str, BELOWS)))
    ap.add_argument("--half", action="store_true", help="with --quality: the host filter with the variance plane scaled by 1/2")
    ap.add_argument("--ab", metavar="PARENT_TREE", help="bench.py of this tree against a built checkout of the parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps-from")
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--gather", choices=["nearest", "bilinear", "both"], default="nearest", help="restir_history_gather_set's mode")
    ap.add_argument("--out")
    a = ap.parse_args()
    gathers = ["nearest", "bilinear"] if a.gather == "both" else [a.gather]
    if a.child:
        kind = a.child[0]
        if kind == "loop":
            child_loop(a.child[1], a.child[2], int(a.child[3]), int(a.child[4]), gathers[0])
        elif kind == "trace":
            child_trace(gathers)
        elif kind == "quality":
            child_quality(a.child[1], [int(v) for v in a.child[2].split(",")], [int(v) for v in a.child[3].split(",")], a.child[4] == "1",
                          gathers[0])
        return
    os.makedirs(OUT_DIR, exist_ok=True)
    if a.ab:
        return bench_ab(os.path.abspath(a.ab), a.rounds, a.out or os.path.join(OUT_DIR, "bench_ab.json"))
    if a.steps_from:
        res, out = {"kernels": steps_from(a.steps_from), "bytes_per_pixel": 156, "size": SIZE}, a.out or os.path.join(OUT_DIR, "kernels.json")
    elif a.quality:
        recs = []
        for cfg in a.cfgs.split(","):
            for g in gathers:
                recs += run_child(["--child", "quality", cfg, a.caps, a.belows, "1" if a.half else "0", "--gather", g], limit=900)
                print(json.dumps(recs[-1])[:300], flush=True)
        res, out = {"quality": recs, "size": SIZE, "yaw_step_deg": YAW_STEP, "gather": a.gather}, a.out or os.path.join(OUT_DIR, "quality.json")
    else:
        runs = {}
        # one mode: every arm, keyed cfg/arm as before; both: the baseline and the two history arms per mode, keyed cfg/arm/mode
        arms = [(arm, gathers[0]) for arm in ARMS] if len(gathers) == 1 else \
            [("present", "nearest")] + [(arm, g) for arm in ("history", "history_resolve") for g in gathers]
        for rep in range(a.reps):
            for cfg in a.cfgs.split(","):
                for arm, g in (arms if rep % 2 == 0 else arms[::-1]):
                    rec = run_child(["--child", "loop", cfg, arm, str(a.frames), str(a.warmup), "--gather", g])[0]
                    key = f"{cfg}/{arm}" if len(gathers) == 1 or arm == "present" else f"{cfg}/{arm}/{g}"
                    runs.setdefault(key, []).append(rec["ms_per_frame"])
                    print(json.dumps(rec), flush=True)
        res = {"loop_ms_per_frame": {k: summary(v) for k, v in runs.items()}, "size": SIZE, "frames": a.frames, "yaw_step_deg": YAW_STEP,
               "gather": a.gather}
        out = a.out or os.path.join(OUT_DIR, "history.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
