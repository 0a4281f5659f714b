#!/usr/bin/env python3
"""What denoising the displayed frame costs and what it gains (restir_denoise).  Not the headline bench (bench.py);
nothing here is a pass / fail bar.

    python scripts/denoise_bench.py [--reps 5] [--iters 300] [--out profiles/denoise/denoise.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/denoise_bench.py --child trace
    python scripts/denoise_bench.py --steps-from DIR [--out ...]      # adds the per-launch times of each step

Scene: the nightclub with 128 point lights at 1920 x 1080 over a still camera, with C2's features (one pass, no temporal
reuse) and C3's (two passes, temporal reuse, the grid threaded through).

(a) the viewer's loop.  Wall ms per displayed frame, total / frames of a loop with one synchronise at the end, of
        render     restir_render(..., NULL) alone, tone mapping off
        present    render with tone mapping on, present as rgba8 (the previous frame's bytes waited for)
        denoise    render with tone mapping off, restir_denoise with the tone fields and the default parameters, present
    each (features, arm) in --reps processes of its own, interleaved arm by arm: median (min - max).
(b) the call.  Wall ms per restir_denoise(..., NULL) of an enqueue-only loop over a still view at 1 .. 5 iterations (each
    call filters the call before's output; the guides stand), in --reps processes each, and in the same process the time
    of a device-to-device hipMemcpyAsync that moves what one level moves -- per pixel the colour read (12 B) and written
    (12 B), the two guide records (32 B) and t (4 B): 60 B, a copy of 30 B -- the yardstick for a kernel bound by memory.
    level_ms = (ms at 5 iterations - ms at 1) / 4.
(c) quality against the exact image (restir_render_exact, restir_error_get; tone mapping off): true mse, rel_mse, mae and
    bias of the mean of n = 1 .. 8 and 16 frames, raw, and of the mean of 1, 4 and 16 frames denoised at 1 .. 5
    iterations; at one frame also a sweep of normal_power_log2 x sigma_plane at 2 iterations.
(d) equal time, from (a) and (c): one denoised frame against the mean of as many raw frames as a loop without the
    denoiser renders in the same wall time, n = floor(denoise / render) (at least 1), and of one frame more.
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
LOOP_ARMS = ["render", "present", "denoise"]
ITERATIONS = [1, 2, 3, 4, 5]
RAW_N = [1, 2, 3, 4, 5, 6, 7, 8, 16]
DENOISED_N = [1, 4, 16]
SWEEP_POWER = [0, 2, 5, 7]
SWEEP_SIGMA = [0.003, 0.01, 0.03, 0.1]
LEVEL_BYTES_PER_PIXEL = 60
TRACE_CALLS = 20


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


def child_loop(name, arm, iters, warmup):
    from romis_amd import _abi
    w, h = SIZE
    r, cam = new_renderer()
    f = _abi.default_features(**dict(SETS[name], enable_tone_mapping=1 if arm == "present" else 0))
    tone = _abi.default_features()
    render = renderer_loop(r, cam, f)
    prev = pending = None
    t0 = 0.0
    for it in range(warmup + iters):
        if it == warmup:
            r.synchronize()
            t0 = time.perf_counter()
        prev = render(prev)
        if arm == "denoise":
            r.denoise(cam, w, h, tone=tone, download=False)
        if arm != "render":
            im = r.present("rgba8")
            if pending is not None:
                pending.wait()      # the displayed frame: the previous one's pinned bytes
                pending.release()
            pending = im
    if pending is not None:
        pending.wait()
        pending.release()
    r.synchronize()
    rec = {"what": "loop", "set": name, "arm": arm, "iters": iters, "ms": (time.perf_counter() - t0) * 1e3 / iters,
           "guide_builds": r.denoise_guide_builds()}
    del prev
    r.close()
    print(json.dumps(rec))


def child_call(iterations, iters, warmup):
    from romis_amd import _abi, restir
    w, h = SIZE
    r, cam = new_renderer()
    renderer_loop(r, cam, _abi.default_features(**C2))(None)
    p = restir.denoise_params(iterations=iterations)
    for _ in range(warmup):
        r.denoise(cam, w, h, params=p, download=False)
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r.denoise(cam, w, h, params=p, download=False)
    r.synchronize()
    rec = {"what": "call", "iterations": iterations, "iters": iters, "ms": (time.perf_counter() - t0) * 1e3 / iters,
           "guide_builds": r.denoise_guide_builds()}
    r.close()
    rec["copy_bytes"] = w * h * LEVEL_BYTES_PER_PIXEL // 2
    rec["copy_ms"] = copy_ms(rec["copy_bytes"], iters)
    print(json.dumps(rec))


def figures(e):
    return dict(mse=e.mse, rel_mse=e.rel_mse, mae=e.mae, bias=e.bias, max_abs=e.max_abs, nonfinite=e.nonfinite)


def child_quality(name):
    from romis_amd import _abi, restir
    w, h = SIZE
    r, cam = new_renderer()
    f = _abi.default_features(**SETS[name])
    render = renderer_loop(r, cam, f)
    r.render_exact(cam, w, h, _abi.default_features(enable_tone_mapping=0), download=False)
    r.reference_set()
    ref_mean = r.error("image").ref_mean
    raw, denoised, sweep = [], [], []
    r.accum_begin(False)
    prev = None
    for n in range(1, max(RAW_N) + 1):
        prev = render(prev)
        r.accum_add()
        if n in RAW_N:
            raw.append(dict(n=n, **figures(r.error("accum"))))
        if n in DENOISED_N:
            for it in ITERATIONS:
                r.accum_resolve(None)   # the mean of n frames, linear, as the image
                r.denoise(cam, w, h, params=restir.denoise_params(iterations=it), download=False)
                denoised.append(dict(n=n, iterations=it, **figures(r.error("image"))))
        if n == 1:
            for power in SWEEP_POWER:
                for sigma in SWEEP_SIGMA:
                    r.accum_resolve(None)
                    r.denoise(cam, w, h, params=restir.denoise_params(2, power, sigma), download=False)
                    sweep.append(dict(normal_power_log2=power, sigma_plane=sigma, iterations=2, **figures(r.error("image"))))
    r.accum_end()
    del prev
    rec = {"what": "quality", "set": name, "ref_mean": ref_mean, "raw": raw, "denoised": denoised, "sweep": sweep,
           "guide_builds": r.denoise_guide_builds()}
    r.close()
    print(json.dumps(rec))


def child_trace():
    """the launches a kernel trace is taken of: C2 frames, each denoised at five iterations"""
    from romis_amd import _abi, restir
    w, h = SIZE
    r, cam = new_renderer()
    render = renderer_loop(r, cam, _abi.default_features(**C2))
    p = restir.denoise_params(iterations=5)
    for _ in range(TRACE_CALLS):
        render(None)
        r.denoise(cam, w, h, params=p, tone=_abi.default_features(), download=False)
    r.synchronize()
    r.close()


def steps_from(trace_dir):
    """per-launch microseconds of k_denoise_guides and of each step of k_denoise_level from a rocprofv3 kernel trace:
    the level launches of one call follow each other, step 1, 2, 4, 8, 16"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda q: int(q["Start_Timestamp"]))
    us = lambda q: (int(q["End_Timestamp"]) - int(q["Start_Timestamp"])) / 1e3
    levels = [us(q) for q in rows if "k_denoise_level" in q["Kernel_Name"]]
    guides = [us(q) for q in rows if "k_denoise_guides" in q["Kernel_Name"]]
    if len(levels) != 5 * TRACE_CALLS:
        raise SystemExit(f"{len(levels)} level launches in the trace, {5 * TRACE_CALLS} expected")
    out = {"what": f"rocprofv3 --kernel-trace, {TRACE_CALLS} calls at five iterations after C2 frames, the first call left out: "
                   "microseconds per launch, median (min - max)", "steps": {}}
    for i in range(5):
        v = levels[5 + i::5]
        out["steps"][str(1 << i)] = {"us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    out["guides"] = {"launches": len(guides), "us": guides}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "denoise.json"))
    ap.add_argument("--steps-from", default=None, metavar="DIR", help="add the per-step launch times of a kernel trace to --out")
    ap.add_argument("--child", nargs="+", metavar="WHAT")
    args = ap.parse_args()
    if args.child:
        what = args.child[0]
        if what == "loop":
            child_loop(args.child[1], args.child[2], args.iters, args.warmup)
        elif what == "call":
            child_call(int(args.child[1]), args.iters, args.warmup)
        elif what == "quality":
            child_quality(args.child[1])
        else:
            child_trace()
        return 0
    if args.steps_from:
        with open(args.out) as fh:
            result = json.load(fh)
        result["steps"] = steps_from(args.steps_from)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        print(json.dumps(result["steps"]))
        return 0

    def run(extra, limit):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup),
                              "--child"] + extra, capture_output=True, text=True, timeout=limit)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            return None   # a failed run ends the measurement: nothing more is started
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        print(json.dumps(rec)[:400], flush=True)
        return rec

    from romis_amd import restir
    default_iterations = restir.denoise_params().iterations
    loops, calls, quality = {}, {}, {}
    for rep in range(args.reps):
        for name in SETS:
            for arm in LOOP_ARMS:
                rec = run(["loop", name, arm], 200)
                if rec is None:
                    return 1
                loops.setdefault((name, arm), []).append(rec)
        for it in ITERATIONS:
            rec = run(["call", str(it)], 200)
            if rec is None:
                return 1
            calls.setdefault(it, []).append(rec)
    for name in SETS:
        rec = run(["quality", name], 400)
        if rec is None:
            return 1
        quality[name] = rec

    def spread(recs, key="ms"):
        v = [x[key] for x in recs]
        return {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "runs": v}

    result = {"image": list(SIZE), "scene": NAME, "reps": args.reps, "iters": args.iters,
              "loop": {"what": "wall ms per displayed frame, total / frames, one synchronise at the end: render = restir_render(..., NULL); "
                               "present = render (tone mapped) + present rgba8; denoise = render (linear) + restir_denoise (tone fields, "
                               "defaults) + present rgba8", "sets": {}},
              "call": {"what": "wall ms per restir_denoise(..., NULL) of an enqueue-only loop on a still view; copy = a device-to-device "
                               "hipMemcpyAsync of 30 B per pixel (one level moves 60 B per pixel, read plus written)", "iterations": {}},
              "quality": {"what": "against the exact image, tone mapping off: the mean of n frames raw, and denoised", "sets": quality},
              "equal_time": {}}
    for (name, arm), recs in loops.items():
        s = result["loop"]["sets"].setdefault(name, {"features": SETS[name], "arms": {}})
        s["arms"][arm] = spread(recs)
        s["arms"][arm]["guide_builds"] = recs[0]["guide_builds"]
    for name, s in result["loop"]["sets"].items():
        a = s["arms"]
        s["denoise_minus_present_ms"] = a["denoise"]["ms_median"] - a["present"]["ms_median"]
        ratio = a["denoise"]["ms_median"] / a["render"]["ms_median"]
        n = max(1, int(ratio))
        q = quality[name]
        result["equal_time"][name] = {
            "denoise_loop_over_render_loop": ratio,
            "raw_frames_in_the_same_time": n,
            "raw_mean": next(x for x in q["raw"] if x["n"] == min(n, 8)),
            "raw_mean_of_one_frame_more": next(x for x in q["raw"] if x["n"] == min(n + 1, 8)),
            "one_frame_denoised": next(x for x in q["denoised"] if x["n"] == 1 and x["iterations"] == default_iterations)}
    for it, recs in calls.items():
        c = spread(recs)
        c["copy"] = dict(spread(recs, "copy_ms"), bytes_copied=recs[0]["copy_bytes"])
        c["guide_builds"] = recs[0]["guide_builds"]
        result["call"]["iterations"][str(it)] = c
    ci = result["call"]["iterations"]
    result["call"]["level_ms"] = (ci["5"]["ms_median"] - ci["1"]["ms_median"]) / 4.0
    result["call"]["level_over_copy"] = result["call"]["level_ms"] / ci["3"]["copy"]["ms_median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"loop": result["loop"]["sets"], "level_ms": result["call"]["level_ms"], "equal_time": result["equal_time"]})[:3000])
    return 0


if __name__ == "__main__":
    sys.exit(main())
