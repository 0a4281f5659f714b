"""Count, in a rocprofv3 kernel trace of the plain C2 bench, the last-pass launches that overlap an RIS launch in time.

    python scripts/ris_ahead_overlap.py <kernel_trace.csv> [--out FILE]

A steady still-view frame is k_gbuf_ris_n1_lds_pt_phat (RIS) and k_spatial1hg_t2_final_vis (the fused last pass).  Run
in series no last pass overlaps an RIS launch; with the RIS look-ahead frame f's last pass runs beside
frame f + 1's RIS.  For each last-pass launch: the time it shares with any RIS launch (start / end timestamps, ns), the
share of its own duration that is, and whether the two ran on different streams.  Also the mean durations of both
kernels (stretched when they co-run) and the period from one RIS start to the next over the steady launches.  With the
RIS batch a launch of k_gbuf_ris_n1_lds_pt_phat_batch2 serves two frames: it counts as an RIS launch here, and its own
count and mean duration are reported beside the RIS launches per frame (per last pass).
"""
import argparse
import csv
import json

RIS, LAST = "k_gbuf_ris_n1_lds_pt_phat", "k_spatial1hg_t2_final_vis"
BATCH = "k_gbuf_ris_n1_lds_pt_phat_batch2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ris, last, batch = [], [], []
    with open(args.trace, newline="") as fh:
        for row in csv.DictReader(fh):
            rec = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row.get("Stream_Id", row.get("Queue_Id")))
            if row["Kernel_Name"] in (RIS, BATCH):
                ris.append(rec)
                if row["Kernel_Name"] == BATCH:
                    batch.append(rec)
            elif row["Kernel_Name"] == LAST:
                last.append(rec)
    ris.sort()
    last.sort()
    overlapping = other_stream = 0
    shared_ns = own_ns = 0
    for s, e, stream in last:
        best = 0
        for rs, re_, rstream in ris:
            if rs >= e:
                break
            ov = min(e, re_) - max(s, rs)
            if ov > 0:
                best += ov
                if rstream != stream:
                    other_stream += 1
        overlapping += 1 if best > 0 else 0
        shared_ns += best
        own_ns += e - s
    mean = lambda v: sum(v) / len(v) if v else 0.0
    starts = [s for s, _, _ in ris]
    periods = sorted(b - a for a, b in zip(starts, starts[1:]))
    out = {"trace": args.trace, "ris_kernel": RIS, "last_pass_kernel": LAST, "ris_launches": len(ris),
           "last_pass_launches": len(last), "last_pass_launches_overlapping_an_ris_launch": overlapping,
           "overlaps_with_an_ris_launch_on_another_stream": other_stream,
           "share_of_last_pass_time_beside_ris": round(shared_ns / own_ns, 4) if own_ns else 0.0,
           "ris_mean_us": round(mean([e - s for s, e, _ in ris]) / 1e3, 2),
           "last_pass_mean_us": round(mean([e - s for s, e, _ in last]) / 1e3, 2),
           "ris_start_to_start_median_us": round(periods[len(periods) // 2] / 1e3, 2) if periods else 0.0,
           "batch_kernel": BATCH, "batch_launches": len(batch),
           "batch_mean_us": round(mean([e - s for s, e, _ in batch]) / 1e3, 2),
           "ris_launches_per_last_pass": round(len(ris) / len(last), 4) if last else 0.0}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
