#!/usr/bin/env python3
"""What llsr_pg_optimize costs on the device against the host graph: the 723 recorded
key poses of tests/golden/result_0318.npz, one loop 722 -> 691 (the candidate §16 reports for that
map) whose constraint is the recorded relative pose moved by 0.5 m and 2 degrees, for P = 1 and P = 64
copies. The time is llsr_pg_report.ms — HIP events around the whole call on the device (copies in, the
passes, copies out), wall time on the host — as the median of --reps fresh graphs after one warm-up.

    python scripts/pose_graph_time.py [--out profiles/pose_graph_time.json] [--reps 5] [--sizes 1,64]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))
import llsr  # noqa: E402
from llsr import PoseGraph  # noqa: E402


def gtsam6(s):
    return np.array([s[2], s[0], s[1], s[5], s[3], s[4]], np.float32)


def build(P, poses, device, frm=722, to=691):
    g = PoseGraph(P, len(poses), 1, 2 * len(poses) + (frm - to), device=device)
    pf, pt = gtsam6(poses[frm]), gtsam6(poses[to])
    pt[0] += 0.5
    pt[5] += np.radians(2.0)
    for p in range(P):
        g.append(p, poses)
        g.add_loop(p, frm, to, pf, pt, 0.3)
    return g


def measure(P, poses, device, reps):
    ms, rep0, out = [], None, None
    for k in range(reps + 1):  # the first is the warm-up
        g = build(P, poses, device)
        reps_ = g.optimize()
        if k:
            ms.append(reps_[0]["ms"])
        rep0, out = reps_[0], g.poses(P - 1)
        assert all(r["state"] == rep0["state"] and r["iterations"] == rep0["iterations"] for r in reps_)
        g.close()
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
            "state": rep0["state"], "iterations": rep0["iterations"], "error_before": rep0["error_before"],
            "error_after": rep0["error_after"]}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_graph_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,64")
    a = ap.parse_args()
    import torch
    poses = np.load(os.path.join(REPO, "tests", "golden", "result_0318.npz"))["key_poses"].astype(np.float32)
    res = {"build_id": llsr.build_id(), "device": torch.cuda.get_device_name(0), "keyframes": len(poses),
           "loop": [722, 691], "variance": 0.3, "reps": a.reps,
           "timing": "llsr_pg_report.ms of fresh graphs after one warm-up: HIP events around the whole call on the "
                     "device, wall time on the host; median, min and max of reps", "sizes": {}}
    for P in (int(x) for x in a.sizes.split(",")):
        dev, dp = measure(P, poses, 0, a.reps)
        host, hp = measure(P, poses, None, a.reps)
        res["sizes"][str(P)] = {"device": dev, "host": host, "poses_bit_equal": dp.tobytes() == hp.tobytes(),
                                "host_over_device": host["ms"] / dev["ms"],
                                "largest_correction_m": float(np.abs(dp[:, :3] - poses[:, :3]).max())}
        print(P, json.dumps(res["sizes"][str(P)]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
