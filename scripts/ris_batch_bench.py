#!/usr/bin/env python3
"""RIS batch (DESIGN.md §6 "RIS batch"): step 0's ceiling and the two cadence forms, on the C2 still view.

ceiling: the one-key table kernel against the two-key one, each alone -- frames.ahead_serial=1 puts every look-ahead
launch behind the frame's last pass, so no kernel runs beside another and the HIP-event time of a launch is the
kernel's own.  t1 = us per launch with frames.batch=1, t2 with frames.batch=2 (every launch past the warm-up is a
batch).  The saving per frame in series is t1 - t2 / 2; the bar is three times the spread of the one-key frame time
(frames.batch=1, nothing serialised: the parent's frame), as scripts/inflight_probe.py uses.

forms: wall-clock ms per frame with nothing timed and nothing serialised, frames.batch=1 / form 0 (a batch when no
result waits) / form 1 (a batch when one result waits).

Rounds are interleaved over the variants in one process and one context.

    python scripts/ris_batch_bench.py [--rounds 5] [--steps 200] [--out-dir profiles/ris_batch]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romis_amd import _abi, restir, scene  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()

    sc = scene.bench_scene("nightclub_128pt")
    cam = scene.camera_for("nightclub_128pt", W, H)
    f = _abi.default_features(initial_light_samples=32, num_samples_in_reservoir=1, num_neighbours_to_sample=5,
                              spatial_resample_radius=10, spatial_resampling_passes=1, spatial_reuse=1, temporal_reuse=0)
    r = restir.Renderer(0)
    r.set_scene(sc)
    r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
    r.set_tuning("timing.mask", -1)
    r.set_tuning("timing.every", 1)

    def run(knobs, timed):
        """ms per frame over --steps frames of the steady still view under `knobs`; timed: and us per RIS launch"""
        for k, v in knobs.items():
            r.set_tuning(k, v)
        for _ in range(args.warmup):   # past ris.phat_after, frames.ahead_after and frames.batch_after
            r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)
        r.synchronize()
        r.reset_timings()
        r.enable_timing(timed)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)
        r.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        r.enable_timing(False)
        kt = r.timings() if timed else {}
        us = {k: (round(v[0] / v[1] * 1e3, 2), v[1]) for k, v in kt.items() if v[1]}
        return round(ms, 5), us

    one = {"frames.batch": 1, "frames.batch_form": 0, "frames.ahead_serial": 0}
    variants = {
        "one_key_alone": ({**one, "frames.ahead_serial": 1}, True),
        "two_keys_alone": ({"frames.batch": 2, "frames.batch_form": 0, "frames.ahead_serial": 1}, True),
        "batch_1": (one, False),
        "form_a": ({"frames.batch": 2, "frames.batch_form": 0, "frames.ahead_serial": 0}, False),
        "form_b": ({"frames.batch": 2, "frames.batch_form": 1, "frames.ahead_serial": 0}, False),
    }
    res = {name: {"ms_per_frame": [], "ris_us_per_launch": [], "ris_launches": [], "last_pass_us": []} for name in variants}
    for _ in range(args.rounds):
        for name, (knobs, timed) in variants.items():
            ms, us = run(knobs, timed)
            res[name]["ms_per_frame"].append(ms)
            if timed:
                res[name]["ris_us_per_launch"].append(us["primary_ris"][0])
                res[name]["ris_launches"].append(us["primary_ris"][1])
                res[name]["last_pass_us"].append(us["spatial"][0])
    r.close()

    med = statistics.median
    t1, t2 = med(res["one_key_alone"]["ris_us_per_launch"]), med(res["two_keys_alone"]["ris_us_per_launch"])
    base = res["batch_1"]["ms_per_frame"]
    spread = max(base) - min(base)
    ceiling = {"what": "C2 1920x1080 nightclub_128pt still view, table built; each RIS launch alone (frames.ahead_serial=1), HIP-event "
                       "us per launch, medians over interleaved rounds; spread: max - min of the one-key frame (frames.batch=1, "
                       "look-ahead beside the last pass) in the same rounds",
               "rounds": args.rounds, "steps": args.steps,
               "t1_us": t1, "t2_us": t2, "t1_rounds": res["one_key_alone"]["ris_us_per_launch"],
               "t2_rounds": res["two_keys_alone"]["ris_us_per_launch"],
               "launches_per_round": {"one_key": res["one_key_alone"]["ris_launches"], "two_keys": res["two_keys_alone"]["ris_launches"]},
               "last_pass_alone_us": med(res["one_key_alone"]["last_pass_us"]),
               "saving_per_frame_in_series_us": round(t1 - t2 / 2, 2),
               "one_key_frame_ms": base, "one_key_frame_spread_ms": round(spread, 5), "bar_us": round(3e3 * spread, 2),
               "clears_bar": (t1 - t2 / 2) > 3e3 * spread,
               "serial_frame_ms": {"one_key": med(res["one_key_alone"]["ms_per_frame"]), "two_keys": med(res["two_keys_alone"]["ms_per_frame"])}}
    forms = {"what": "C2 still view, wall-clock ms per frame over --steps frames, nothing timed, interleaved rounds: frames.batch=1, "
                     "form a (a batch when no result waits), form b (a batch when one result waits)",
             "rounds": args.rounds, "steps": args.steps}
    for name in ("batch_1", "form_a", "form_b"):
        v = res[name]["ms_per_frame"]
        forms[name] = {"ms_per_frame": v, "median": med(v), "min": min(v), "max": max(v)}
    forms["better"] = "form_b" if forms["form_b"]["median"] < forms["form_a"]["median"] else "form_a"
    print(json.dumps({"ceiling": ceiling, "forms": forms}))
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        for name, obj in (("ceiling.json", ceiling), ("forms.json", forms)):
            with open(os.path.join(args.out_dir, name), "w") as fh:
                fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
