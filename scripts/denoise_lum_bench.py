#!/usr/bin/env python3
"""What the variance-guided luminance term costs and what it gains (restir_denoise_lum next to restir_denoise).  Not the
headline bench (bench.py); nothing here is a pass / fail bar.  scripts/denoise_bench.py stays as it is: its recorded
figures remain reproducible.

    python scripts/denoise_lum_bench.py [--reps 5] [--iters 200] [--out profiles/denoise_lum/denoise_lum.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/denoise_lum_bench.py --child trace
    python scripts/denoise_lum_bench.py --steps-from DIR [--out profiles/denoise_lum/kernels.json]
    python scripts/denoise_lum_bench.py --ab PARENT_TREE [--rounds 5] [--out profiles/denoise_lum/bench_ab.json]

Scene: the nightclub with 128 point lights at 1920 x 1080 over a still camera, C2's features (one pass, no temporal
reuse) and C3's (two passes, temporal reuse, the grid threaded through).  Every child process runs under a time limit
of its own, and the first one that fails ends the measurement: nothing more is started.

(1) the call.  Wall ms per restir_denoise_lum(..., NULL) of an enqueue-only loop on a still view at 1 .. 5 levels, for
    RESTIR_DENOISE_VAR_SPATIAL (each call filters the call before's output) and RESTIR_DENOISE_VAR_ACCUM (an open
    accumulation of four C2 frames), and in the same process restir_denoise's at the same level count; --reps processes
    per (source, levels): median (min - max).  level_ms = (ms at 5 levels - ms at 1) / 4 for each of the three.
(2) --steps-from: per-launch microseconds of every k_denoise_* kernel from a kernel trace of --child trace, the level
    kernels per step.
(3) quality against the exact image (restir_render_exact, restir_error_get; tone mapping off): true mse, rel_mse, mae and
    bias of one frame (SPATIAL) and of the means of 4, 16 and 64 frames (ACCUM), at 1 .. 5 levels and sigma_lum in
    {1, 2, 4, 8}, with restir_denoise at 1 .. 5 levels and the raw input as the other arms; C2 and C3.
(4) --ab: bench.py C2 / C3 of this tree against a checkout of the parent commit (built beforehand), one process each,
    trees interleaved and the order within a pair alternating.
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
C2 = dict(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5, spatial_resample_radius=10,
          spatial_reuse=1, spatial_resampling_passes=1, temporal_reuse=0, enable_tone_mapping=0)
SETS = {"c2": C2, "c3": dict(C2, spatial_resampling_passes=2, temporal_reuse=1)}
SOURCES = ["spatial", "accum"]
LEVELS = [1, 2, 3, 4, 5]
SIGMAS = [1.0, 2.0, 4.0, 8.0]
MEANS = [1, 4, 16, 64]
ACCUM_FRAMES = 4
TRACE_CALLS = 10
OUT_DIR = os.path.join(ROOT, "profiles", "denoise_lum")


def new_renderer():
    from romis_amd import restir, scene
    r = restir.Renderer(0)
    r.set_scene(scene.bench_scene(NAME))
    r.set_seed(0x5EED, 0)
    return r, scene.camera_for(NAME, *SIZE)


def renderer_loop(r, cam, f):
    """render(prev) -> next grid: restir_render itself, without an image handed back"""
    import ctypes as C

    from romis_amd import restir
    w, h = SIZE
    temporal = bool(f.temporal_reuse)

    def render(prev):
        nxt = C.c_void_p()
        restir.check(r.lib, r.lib.restir_render(r.ctx, C.byref(cam), C.byref(f), w, h, None, prev.handle if prev is not None else None,
                                                C.byref(nxt) if temporal else None, None), "restir_render")
        return restir.ReservoirGrid(r.lib, nxt) if temporal else None
    return render


def lum_params(source, levels, sigma=None):
    from romis_amd import _abi, restir
    return restir.denoise_lum_params(iterations=levels, sigma_lum=sigma,
                                     variance_source=_abi.RESTIR_DENOISE_VAR_ACCUM if source == "accum" else _abi.RESTIR_DENOISE_VAR_SPATIAL)


def timed(r, call, iters, warmup):
    for _ in range(warmup):
        call()
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def child_call(source, levels, iters, warmup):
    from romis_amd import _abi, restir
    w, h = SIZE
    r, cam = new_renderer()
    render = renderer_loop(r, cam, _abi.default_features(**C2))
    if source == "accum":
        r.accum_begin(True)
        for _ in range(ACCUM_FRAMES):
            render(None)
            r.accum_add()
    else:
        render(None)
    p, q = lum_params(source, levels), restir.denoise_params(iterations=levels)
    rec = {"what": "call", "source": source, "levels": levels, "iters": iters}
    rec["lum_ms"] = timed(r, lambda: r.denoise_lum(cam, w, h, params=p, download=False), iters, warmup)
    rec["denoise_ms"] = timed(r, lambda: r.denoise(cam, w, h, params=q, download=False), iters, warmup)
    rec["lum_ms_again"] = timed(r, lambda: r.denoise_lum(cam, w, h, params=p, download=False), iters, warmup)
    rec["guide_builds"] = r.denoise_guide_builds()
    r.close()
    print(json.dumps(rec))


def figures(e):
    return dict(mse=e.mse, rel_mse=e.rel_mse, mae=e.mae, bias=e.bias, max_abs=e.max_abs, nonfinite=e.nonfinite)


def child_quality(name):
    from romis_amd import _abi, restir
    w, h = SIZE
    r, cam = new_renderer()
    render = renderer_loop(r, cam, _abi.default_features(**SETS[name]))
    r.render_exact(cam, w, h, _abi.default_features(enable_tone_mapping=0), download=False)
    r.reference_set()
    rows = []
    r.accum_begin(True)
    prev = None
    for n in range(1, max(MEANS) + 1):
        prev = render(prev)
        r.accum_add()
        if n not in MEANS:
            continue
        source = "spatial" if n == 1 else "accum"
        rows.append(dict(n=n, arm="raw", **figures(r.error("accum"))))
        for levels in LEVELS:
            r.accum_resolve(None)   # the mean of n frames, linear, as the image
            r.denoise(cam, w, h, params=restir.denoise_params(iterations=levels), download=False)
            rows.append(dict(n=n, arm="denoise", levels=levels, **figures(r.error("image"))))
            for sigma in SIGMAS:
                if source == "spatial":
                    r.accum_resolve(None)
                r.denoise_lum(cam, w, h, params=lum_params(source, levels, sigma), download=False)
                rows.append(dict(n=n, arm="lum", source=source, levels=levels, sigma_lum=sigma, **figures(r.error("image"))))
    r.accum_end()
    del prev
    rec = {"what": "quality", "set": name, "rows": rows, "guide_builds": r.denoise_guide_builds()}
    r.close()
    print(json.dumps(rec))


def child_trace():
    """the launches a kernel trace is taken of: per round one SPATIAL call, one ACCUM call and one restir_denoise call, each at
    five levels, over an accumulation of four C2 frames"""
    from romis_amd import _abi, restir
    w, h = SIZE
    r, cam = new_renderer()
    render = renderer_loop(r, cam, _abi.default_features(**C2))
    r.accum_begin(True)
    for _ in range(ACCUM_FRAMES):
        render(None)
        r.accum_add()
    for _ in range(TRACE_CALLS):
        render(None)
        r.denoise_lum(cam, w, h, params=lum_params("spatial", 5), download=False)
        r.denoise_lum(cam, w, h, params=lum_params("accum", 5), download=False)
        r.denoise(cam, w, h, params=restir.denoise_params(iterations=5), download=False)
    r.synchronize()
    r.accum_end()
    r.close()


def steps_from(trace_dir):
    """per-launch microseconds of the k_denoise_* kernels from a rocprofv3 kernel trace of child_trace: a call's level
    launches follow each other, step 1, 2, 4, 8, 16"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda q: int(q["Start_Timestamp"]))
    us = lambda q: (int(q["End_Timestamp"]) - int(q["Start_Timestamp"])) / 1e3   # noqa: E731

    def med(v):
        return {"launches": len(v), "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}

    out = {"what": f"rocprofv3 --kernel-trace, {TRACE_CALLS} rounds of (SPATIAL, ACCUM, restir_denoise) at five levels, the first "
                   "round left out: microseconds per launch", "kernels": {}}
    kinds = {"level_lum": lambda n: "k_denoise_level<true>" in n or "k_denoise_levelILb1" in n,
             "level": lambda n: "k_denoise_level<false>" in n or "k_denoise_levelILb0" in n,
             "var_spatial": lambda n: "k_denoise_var_spatial" in n, "var_accum": lambda n: "k_denoise_var_accum" in n,
             "guides": lambda n: "k_denoise_guides" in n}
    for kind, match in kinds.items():
        v = [us(q) for q in rows if match(q["Kernel_Name"])]
        if not v:
            continue
        if kind == "level_lum":     # 10 launches per round: SPATIAL's five, then ACCUM's five
            out["kernels"][kind] = {str(1 << i): med(v[10 + i::10] + v[15 + i::10]) for i in range(5)}
        elif kind == "level":
            out["kernels"][kind] = {str(1 << i): med(v[5 + i::5]) for i in range(5)}
        else:
            out["kernels"][kind] = med(v[1:] if len(v) > 1 else v)
    return out


def write(path, result):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def spread(v):
    return {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "runs": v}


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
                    return 1   # a failed run ends the measurement
                rec = json.loads(o.stdout.strip().splitlines()[-1])
                runs[cfg][label].append(rec["ms_per_step"])
                print(rnd, cfg, label, rec["ms_per_step"], flush=True)
    result = {"what": "bench.py --gpus 1 --steps 200 --warmup 20 --config <c> --no-cpu-baseline --no-cpu-stages ms_per_step, one process "
                      f"each, parent commit / this tree interleaved, the order within a pair alternating, {rounds} rounds", "configs": {}}
    for cfg, r in runs.items():
        p, t = spread(r["parent"]), spread(r["this"])
        result["configs"][cfg] = {"parent": p, "this": t,
                                  "this_median_within_parent_min_max": p["ms_min"] <= t["ms_median"] <= p["ms_max"]}
    write(out, result)
    print(json.dumps({c: (v["parent"]["ms_median"], v["this"]["ms_median"]) for c, v in result["configs"].items()}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps-from", default=None, metavar="DIR", help="write the per-kernel launch times of a kernel trace")
    ap.add_argument("--ab", default=None, metavar="PARENT_TREE", help="bench.py of this tree against a built checkout of the parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip", nargs="*", default=[], choices=["call", "quality"])
    ap.add_argument("--child", nargs="+", metavar="WHAT")
    args = ap.parse_args()
    if args.child:
        what = args.child[0]
        if what == "call":
            child_call(args.child[1], int(args.child[2]), args.iters, args.warmup)
        elif what == "quality":
            child_quality(args.child[1])
        else:
            child_trace()
        return 0
    if args.steps_from:
        result = steps_from(args.steps_from)
        write(args.out or os.path.join(OUT_DIR, "kernels.json"), result)
        print(json.dumps(result["kernels"]))
        return 0
    if args.ab:
        return bench_ab(os.path.abspath(args.ab), args.rounds, args.out or os.path.join(OUT_DIR, "bench_ab.json"))

    def run(extra, limit):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup),
                              "--child"] + extra, capture_output=True, text=True, timeout=limit)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            return None   # a failed run ends the measurement: nothing more is started
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        print(json.dumps(rec)[:300], flush=True)
        return rec

    from romis_amd import restir
    d = restir.denoise_lum_params()
    result = {"image": list(SIZE), "scene": NAME, "reps": args.reps, "iters": args.iters,
              "defaults": {"iterations": d.geo.iterations, "normal_power_log2": d.geo.normal_power_log2,
                           "sigma_plane": d.geo.sigma_plane, "sigma_lum": d.sigma_lum}}
    if "quality" not in args.skip:
        quality = {}
        for name in SETS:
            rec = run(["quality", name], 400)
            if rec is None:
                return 1
            quality[name] = rec
        result["quality"] = {"what": "against the exact image, tone mapping off: the mean of n frames raw (arm raw), under "
                                     "restir_denoise (arm denoise) and under restir_denoise_lum (arm lum: SPATIAL at n = 1, ACCUM beyond)",
                             "sets": quality}
    if "call" not in args.skip:
        calls = {}
        for _ in range(args.reps):
            for source in SOURCES:
                for levels in LEVELS:
                    rec = run(["call", source, str(levels)], 200)
                    if rec is None:
                        return 1
                    calls.setdefault((source, levels), []).append(rec)
        table = {"what": "wall ms per call of an enqueue-only loop on a still view; lum = restir_denoise_lum, denoise = restir_denoise in "
                         "the same process, lum_again = restir_denoise_lum once more after it", "sources": {}}
        for (source, levels), recs in calls.items():
            table["sources"].setdefault(source, {})[str(levels)] = {k: spread([x[k + "_ms"] for x in recs]) for k in ("lum", "denoise")}
            table["sources"][source][str(levels)]["lum_again"] = spread([x["lum_ms_again"] for x in recs])
        for source, t in table["sources"].items():
            t["level_ms"] = {k: (t["5"][k]["ms_median"] - t["1"][k]["ms_median"]) / 4.0 for k in ("lum", "denoise")}
            t["level_ratio"] = t["level_ms"]["lum"] / t["level_ms"]["denoise"]
        result["call"] = table
    write(args.out or os.path.join(OUT_DIR, "denoise_lum.json"), result)
    return 0


if __name__ == "__main__":
    sys.exit(main())
