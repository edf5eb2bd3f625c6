#!/usr/bin/env python3
"""Reduce the two rocprofv3 traces that explain scripts/odo_odom_ab.py's flagged-path deficit to one
JSON record: per timed step, the span from the first kernel to the end of k_odo_finish, the time of
each kernel, the idle time inside the span, the gap between the LM's end and k_odo_finish's start,
and the traced copies. The traces are one run per variant, each of its own:

  rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR/prof_base -o base \\
      -- python scripts/odo_odom_ab.py --only base --rounds 6
  rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR/prof_odom -o odom \\
      -- python scripts/odo_odom_ab.py --only odom --rounds 6
  python scripts/odo_odom_trace.py DIR --build-id ID --out profiles/odo_odom_trace_ID.json

A step ends with k_odo_finish; a round is 7 steps (2 warm-up, 5 timed); the first round (code-object
loads, allocations) is left out.
"""
import argparse
import collections
import csv
import glob
import json
import os

FRAMES, WARMUP = 7, 2
SMALL_COPY_NS = 20000


def _one(dirname: str, name: str):
    hits = glob.glob(os.path.join(dirname, "**", name), recursive=True)
    if len(hits) != 1:
        raise SystemExit(f"{dirname}: expected one {name}, found {len(hits)}")
    return hits[0]


def reduce(dirname: str, tag: str) -> dict:
    rows = list(csv.DictReader(open(_one(dirname, f"{tag}_kernel_trace.csv"))))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], []
    for r in rows:
        cur.append(r)
        if "k_odo_finish" in r["Kernel_Name"]:
            steps.append(cur)
            cur = []
    per = collections.defaultdict(float)
    n = span = busy = gap = 0
    lm_max = 0
    for i, st in enumerate(steps):
        if i < FRAMES or i % FRAMES < WARMUP:
            continue
        n += 1
        span += int(st[-1]["End_Timestamp"]) - int(st[0]["Start_Timestamp"])
        for r in st:
            d = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("llsr::", "").split("<")[0]
            per[k] += d
            busy += d
        lm = [r for r in st if "k_s2s_lm" in r["Kernel_Name"]][-1]
        lm_max = max(lm_max, int(lm["End_Timestamp"]) - int(lm["Start_Timestamp"]))
        gap += int(st[-1]["Start_Timestamp"]) - int(lm["End_Timestamp"])
    if not n:
        raise SystemExit(f"{dirname}: no timed step found")
    copies = list(csv.DictReader(open(_one(dirname, f"{tag}_memory_copy_trace.csv"))))
    dur = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in copies]
    small = [d for d in dur if d < SMALL_COPY_NS]
    us = lambda v: round(v / n / 1e3, 1)  # noqa: E731
    top = dict(sorted(((k, us(v)) for k, v in per.items()), key=lambda kv: -kv[1])[:8])
    top["k_odo_finish"] = us(per["k_odo_finish"])
    return {"steps_traced": len(steps), "timed_steps_averaged": n,
            "per_step_us": {"first_kernel_to_k_odo_finish_end": us(span), "kernels_busy": us(busy),
                            "idle_in_span": us(span - busy), "gap_lm_end_to_k_odo_finish_start": us(gap),
                            "kernels": top},
            "k_s2s_lm_max_us": round(lm_max / 1e3, 1),
            "copies": dict(collections.Counter(r["Direction"] for r in copies)),
            "small_copies": {"count": len(small), "mean_us": round(sum(small) / max(1, len(small)) / 1e3, 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", help="holds prof_base/ and prof_odom/")
    ap.add_argument("--build-id", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    base = reduce(os.path.join(args.dir, "prof_base"), "base")
    odom = reduce(os.path.join(args.dir, "prof_odom"), "odom")
    b, o = base["per_step_us"], odom["per_step_us"]
    rec = {"what": "rocprofv3 --kernel-trace --memory-copy-trace --stats, one run per variant of "
                   "scripts/odo_odom_ab.py --only base|odom --rounds 6, reduced by scripts/odo_odom_trace.py",
           "build_id": args.build_id, "base": base, "odom": odom,
           "odom_minus_base_us_per_step": {
               "span": round(o["first_kernel_to_k_odo_finish_end"] - b["first_kernel_to_k_odo_finish_end"], 1),
               "k_s2s_lm": round(o["kernels"].get("k_s2s_lm", 0.0) - b["kernels"].get("k_s2s_lm", 0.0), 1),
               "k_odo_finish": round(o["kernels"]["k_odo_finish"] - b["kernels"]["k_odo_finish"], 1),
               "gap_lm_end_to_k_odo_finish_start": round(o["gap_lm_end_to_k_odo_finish_start"] -
                                                         b["gap_lm_end_to_k_odo_finish_start"], 1),
               "idle_in_span": round(o["idle_in_span"] - b["idle_in_span"], 1)}}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["odom_minus_base_us_per_step"]))


if __name__ == "__main__":
    main()
