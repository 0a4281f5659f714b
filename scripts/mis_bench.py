#!/usr/bin/env python3
"""Time R-MIS / R-OMIS renders (renderRMIS / renderROMIS, render.cpp:64-265) on the GPU against the oracle's CPU
restatement (OpenMP) on the same host.  One JSON object per line; not the headline bench (bench.py).

    python scripts/mis_bench.py [--width 1920 --height 1080] [--cpu-width 320 --cpu-height 180] [--reps 3]
    python scripts/mis_bench.py --no-cpu --tiles 4x2      # + every screen tile alone (restir_render_mis_tile)

--tiles TXxTY: after the whole frame, each tile of the even split is rendered alone on the same GPU, in turn (ghost ring =
the resample radius; same warm-up, minimum over --reps).  The stitched tiles must equal the whole frame word for word,
else the script exits non-zero.  implied_efficiency_no_transfer = whole_ms / (n * max_tile_ms): what n GPUs rendering one
tile each would gain over one GPU, had they this GPU's tile times -- no gather, no second GPU is in the figure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from romis_amd import _abi, restir, scene  # noqa: E402

CASES = {
    "rmis_equal": dict(ray_trace_mode=_abi.MODE_RMIS),
    "rmis_balance": dict(ray_trace_mode=_abi.MODE_RMIS, mis_weight_rmis=_abi.MIS_BALANCE),
    "romis_direct": dict(ray_trace_mode=_abi.MODE_ROMIS),
    "romis_progressive_n6": dict(ray_trace_mode=_abi.MODE_ROMIS, use_progressive_romis=1, num_samples_in_reservoir=6),
}
SEED = _abi.RESTIR_DEFAULT_SEED
MIS_SAMPLE_BUDGET = 4 << 30   # restir.cpp kMisSampleBudget


def device_bytes(f, width, height, view, owned):
    """Device bytes of one render's buffers, as restir.cpp sizes them (ensure_work, ensure_mis, the image): the G-buffer,
    both reservoir grids and debug planes by view pixels; neighbourhoods, accumulators, R-OMIS per-sample scratch and
    the image by owned pixels.  (Scene tables and a textured scene's texCoord plane not counted.)"""
    vpx, opx = view[0] * view[1], owned[0] * owned[1]
    N, k, r = f.num_samples_in_reservoir, f.num_neighbours_to_sample, f.spatial_resample_radius
    out = {"gbuffer": vpx * 32, "reservoirs_and_debug": 2 * vpx * N * (16 + 16 + 8)}
    cap = k + 1
    if f.neighbour_selection_strategy not in (_abi.NEIGHBOURS_RANDOM, _abi.NEIGHBOURS_SIMILAR):
        cap = max(cap, min(2 * r + 1, width) * min(2 * r + 1, height))
    romis = f.ray_trace_mode == _abi.MODE_ROMIS
    T = k + 1
    out["neighbourhoods"] = (1 + cap) * opx * 4
    out["accumulators"] = (T * T + 6 * T + 3 if romis else 3) * opx * 4
    out["sample_scratch"] = 0
    if romis:
        per = (T + 3) * opx * 4
        n = max(1, min(T * N, MIS_SAMPLE_BUDGET // per))
        n = min(n, max(1, ((1 << 31) - 1) // max(opx, 1)))
        out["sample_scratch"] = n * per
    out["image"] = opx * 12
    out["total"] = sum(out.values())
    return out


def timed(render, reps):
    """(min seconds over reps, the last image) of render()."""
    t, img = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        img = render()
        t.append(time.perf_counter() - t0)
    return min(t), img


def kernel_ms(r, render):
    """RESTIR_K_* milliseconds of one render() (event-timed, outside the wall-clock figures)."""
    r.enable_timing(True)
    r.reset_timings()
    render()
    ms = {k: round(v[0], 4) for k, v in r.timings().items() if v[1]}
    r.enable_timing(False)
    return ms


def tiles_record(r, cam, f, W, H, tx, ty, reps, whole_s, whole_img):
    n = tx * ty
    radius = f.spatial_resample_radius
    stitched = np.zeros((H, W, 3), np.float32)
    per_tile, ms, tile_k = [], [], []
    for q in range(n):
        t = restir.tile_plan(W, H, tx, ty, q, radius)

        def render(t=t):
            r.set_seed(SEED, 0)
            return r.render_mis(cam, W, H, f, tile=t)
        render()   # warm-up (allocation at this tile's size)
        r.synchronize()
        s, img = timed(render, reps)
        r0 = H - (t.y0 + t.height)
        stitched[r0:r0 + t.height, t.x0:t.x0 + t.width] = img
        ms.append(round(s * 1e3, 3))
        tile_k.append(kernel_ms(r, render))
        per_tile.append({"rank": q, "owned": [t.x0, t.y0, t.width, t.height], "view": [t.gx0, t.gy0, t.gwidth, t.gheight],
                         "ms": ms[-1], "view_over_owned_px": round(t.gwidth * t.gheight / (t.width * t.height), 4),
                         "kernel_ms": tile_k[-1]})
    diff = int((stitched.view(np.uint32) != whole_img.view(np.uint32)).sum())
    worst = int(np.argmax(ms))
    tw = restir.tile_plan(W, H, tx, ty, max(range(n), key=lambda q: per_tile[q]["view"][2] * per_tile[q]["view"][3]), radius)
    view_px = sum(p["view"][2] * p["view"][3] for p in per_tile)
    return {"tiles": [tx, ty], "tile_ms": ms, "max_tile_ms": max(ms), "slowest_tile": worst,
            "largest_tile_over_whole_time": round(max(ms) / (whole_s * 1e3), 4),
            "implied_efficiency_no_transfer": round(whole_s * 1e3 / (n * max(ms)), 4),
            "view_over_owned_px": round(view_px / (W * H), 4), "stitched_words_differing": diff, "per_tile": per_tile,
            "device_bytes_whole": device_bytes(f, W, H, (W, H), (W, H)),
            "device_bytes_largest_tile": device_bytes(f, W, H, (tw.gwidth, tw.gheight), (tw.width, tw.height))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="nightclub_128pt")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cpu-width", type=int, default=320)
    ap.add_argument("--cpu-height", type=int, default=180)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--tiles", default=None, metavar="TXxTY", help="also render every tile of this even split alone")
    args = ap.parse_args()
    tiles = tuple(int(v) for v in args.tiles.lower().split("x")) if args.tiles else None
    if tiles is not None and (len(tiles) != 2 or min(tiles) < 1):
        ap.error("--tiles takes TXxTY, e.g. 4x2")
    sc = scene.bench_scene(args.scene)
    r = restir.Renderer(0)
    r.set_scene(sc)
    osc = None
    mismatch = False
    for name, kw in CASES.items():
        f = _abi.default_features(**kw)   # reference defaults: N = 2 (unless set), k = 5, r = 10, 5 iterations
        cam = scene.camera_for(args.scene, args.width, args.height)

        def whole():
            if tiles is not None:
                r.set_seed(SEED, 0)   # the tiles are compared with this frame
            return r.render_mis(cam, args.width, args.height, f)
        whole()   # warm-up (allocation, code load)
        r.synchronize()
        gpu_s, whole_img = timed(whole, args.reps)
        rec = {"case": name, "scene": args.scene, "image": [args.width, args.height], "N": f.num_samples_in_reservoir,
               "k": f.num_neighbours_to_sample, "iterations": f.max_iterations_mis, "gpu_ms": round(gpu_s * 1e3, 3),
               "gpu_mpx_per_s": round(args.width * args.height / gpu_s / 1e6, 2)}
        if tiles is not None:
            rec["kernel_ms"] = kernel_ms(r, whole)
            rec.update(tiles_record(r, cam, f, args.width, args.height, tiles[0], tiles[1], args.reps, gpu_s, whole_img))
            mismatch = mismatch or rec["stitched_words_differing"] != 0
        if not args.no_cpu:
            from oracle import pyoracle
            osc = osc or pyoracle.OracleScene(sc)
            cw, ch = args.cpu_width, args.cpu_height
            ccam = scene.camera_for(args.scene, cw, ch)
            threads = min(16, os.cpu_count() or 1)
            t0 = time.perf_counter()
            pyoracle.render_mis(osc, ccam, f, cw, ch, threads=threads)
            cpu_s = time.perf_counter() - t0
            rec.update({"cpu_sample": [cw, ch], "cpu_threads": threads, "cpu_s": round(cpu_s, 3),
                        "cpu_mpx_per_s": round(cw * ch / cpu_s / 1e6, 4),
                        "gpu_over_cpu": round((args.width * args.height / gpu_s) / (cw * ch / cpu_s), 1)})
        print(json.dumps(rec), flush=True)
    r.close()
    if mismatch:
        print("mis_bench: stitched tiles differ from the whole frame", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
