"""Probe: the ceiling of running C2 still-view frames side by side on one GPU (DESIGN.md §6 "RIS look-ahead", step 0).

Two contexts render the same still view, each past ris.phat_after, their frames issued alternately with no
synchronisation between them: each context's stream holds RIS -> last pass in order, and the two streams are free to
co-run.  The aggregate time per frame of the pair, against the serial frame of one context, bounds what any overlap of
RIS with the last pass can gain.  Rounds are interleaved serial / pair / serial / ...; throughput only.

    python scripts/inflight_probe.py [--rounds 5] [--steps 200] [--tune KEY=VALUE ...] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romis_amd import _abi, restir, scene  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sc = scene.bench_scene("nightclub_128pt")
    cam = scene.camera_for("nightclub_128pt", W, H)
    f = _abi.default_features(initial_light_samples=32, num_samples_in_reservoir=1, num_neighbours_to_sample=5,
                              spatial_resample_radius=10, spatial_resampling_passes=1, spatial_reuse=1, temporal_reuse=0)
    rs = []
    for i in range(2):
        r = restir.Renderer(0)
        for kv in args.tune:
            key, val = kv.split("=", 1)
            r.set_tuning(key, int(val))
        r.set_scene(sc)
        r.set_seed(_abi.RESTIR_DEFAULT_SEED, 1000 * i)
        rs.append(r)

    def frames(ctxs, n):   # n frames per context, alternated; ms per frame over all of them
        for r in ctxs:
            r.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            for r in ctxs:
                r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)
        for r in ctxs:
            r.synchronize()
        return (time.perf_counter() - t0) / (n * len(ctxs)) * 1e3

    frames(rs, args.warmup)   # both past ris.phat_after (and final.vis_after): the steady still frame
    serial, pair = [], []
    for _ in range(args.rounds):
        serial.append(round(frames(rs[:1], args.steps), 5))
        pair.append(round(frames(rs, args.steps), 5))
    for r in rs:
        r.close()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = max(serial) - min(serial)
    out = {"what": "C2 1920x1080 nightclub_128pt still view, ms per frame; pair = two contexts' frames alternated, "
                   "aggregate over both", "steps": args.steps, "rounds": args.rounds, "tune": args.tune,
           "serial_ms": serial, "pair_ms": pair, "serial_median": med(serial), "pair_median": med(pair),
           "serial_spread": round(spread, 5), "gain_ms": round(med(serial) - med(pair), 5),
           "bar_ms": round(3 * spread, 5), "clears_bar": med(serial) - med(pair) > 3 * spread}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
